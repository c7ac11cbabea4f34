// kernels_score_mesh.h -- the map scored against a labelled triangle mesh (include/ratsdf_score_mesh.h) for gfx950:
// the build of a mesh set (bounds and validation -> references per cell -> scan -> scatter into a dense grid of cells)
// and the join "every selected voxel -> its nearest kept triangle" with the counts that follow from it.
//
// The join walks the selection list of k_score_labels, one 256-thread workgroup per map block at a time, and the same
// rings of cells around the block (kernels_score.h): a cell references every kept triangle whose axis-aligned box meets
// it, each ring's references are resolved to 48-byte triangle records and staged in LDS in chunks of kMeshChunk.
// A pair (voxel, triangle) costs about ten times a pair (voxel, point), and only a few percent of a block's voxels are
// selected, so the workgroup first compacts its selected voxels (a block scan of the two flags per thread) and spreads
// the product (S selected voxels) x (staged triangles) over its lanes: with S <= 256, lane l works for voxel l % S on
// the triangles j = l / S, l / S + K, ... of a chunk, K = 256 / S; with S > 256 a lane holds two voxels and every
// triangle.  A lane keeps the minimum of the 64-bit key (dist2 bits << 32 | original index) -- dist2 >= 0, so the key
// orders as the contract's (dist2, index), whatever the order of the reduction -- and the K lanes of a voxel meet in an
// LDS integer minimum after every ring, because the stop test needs the voxel's best.  A staged record is read at one
// address by every lane of a wave when S >= 64 (a broadcast); a triangle referenced from several cells of a walk is
// staged more than once, which a minimum does not notice.  -DRATSDF_SCORE_MESH_PLAIN builds the other layout for the
// A/B of DESIGN 4 "Label score against a mesh": no compaction, two voxels per lane as in k_score_labels.
//
// The grid only accelerates.  The closest point q of a triangle is clamped to the triangle's box, so dist2 is at least
// the squared distance from the voxel to that box along any axis, up to the rounding of one subtraction and one
// product (2^-22 relative).  After ring r every triangle that has not been looked at has its box, along some axis, at
// least r whole cells beyond the block's extent (up to cell * 2^-28 of double rounding, as for points), so the point
// score's bound (r * cell * (1 - 1e-5))^2, rounded down, ends the walk with the same margin.
#pragma once
#include "kernels_score.h"

namespace ratsdf {

#ifndef RATSDF_SCORE_MESH_CHUNK
#define RATSDF_SCORE_MESH_CHUNK 256
#endif
constexpr int kMeshChunk = RATSDF_SCORE_MESH_CHUNK;  // 48-byte triangle records per LDS chunk (256: 12 KiB)
constexpr int kMeshLanes = 8;                        // lanes that share the cells of one triangle's box in the build
constexpr int kMeshMaxRing = 192;                    // never reached with max_dist <= 64 * cell: a guard, not a contract
constexpr unsigned long long kMeshNoKey = ~0ull;

// the device side of a mesh set, by value
struct MeshGrid {
  const float4* rec;      // three per ORIGINAL triangle index, written for kept ones: {a, index bits}, {b, 0}, {c, 0}
  const uint32_t* start;  // cells + 1 words: where each cell's references start
  const uint32_t* ref;    // original indices of kept triangles, sorted by cell
  const uint8_t* label;   // one byte per original triangle index: the label of its first vertex
  double ox, oy, oz, cell;
  int cx, cy, cz;
};

// Triangle t of the caller's arrays: 0 -- an index outside [0, nv) (nothing is loaded through it), 1 -- dropped
// (a non-finite coordinate, or two vertices equal in all three coordinates), 2 -- kept.  i[] are its three indices.
__device__ inline int mesh_load(const float* xyz, size_t nv, const int32_t* tri, size_t t, int32_t i[3], float a[3],
                                float b[3], float c[3]) {
  i[0] = tri[3 * t], i[1] = tri[3 * t + 1], i[2] = tri[3 * t + 2];
  if ((size_t)(uint32_t)i[0] >= nv || (size_t)(uint32_t)i[1] >= nv || (size_t)(uint32_t)i[2] >= nv) return 0;
  bool finite = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    a[k] = xyz[3 * (size_t)i[0] + k], b[k] = xyz[3 * (size_t)i[1] + k], c[k] = xyz[3 * (size_t)i[2] + k];
    finite = finite && score_finite(a[k]) && score_finite(b[k]) && score_finite(c[k]);
  }
  if (!finite) return 1;
  const bool same = (a[0] == b[0] && a[1] == b[1] && a[2] == b[2]) || (a[0] == c[0] && a[1] == c[1] && a[2] == c[2]) ||
                    (b[0] == c[0] && b[1] == c[1] && b[2] == c[2]);
  return same ? 1 : 2;
}

// the cells a kept triangle's box meets: lo[] .. hi[] per axis, inside the grid
__device__ inline void mesh_box_cells(const MeshGrid& g, const float a[3], const float b[3], const float c[3],
                                      int lo[3], int hi[3]) {
  const double o[3] = {g.ox, g.oy, g.oz};
  const int n[3] = {g.cx, g.cy, g.cz};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    lo[k] = score_cell(fminf(fminf(a[k], b[k]), c[k]), o[k], g.cell, n[k]);
    hi[k] = score_cell(fmaxf(fmaxf(a[k], b[k]), c[k]), o[k], g.cell, n[k]);
  }
}

// out: [0..2] smallest, [3..5] largest coordinate of the kept triangles' vertices as score_ord words (initialised to
// ~0 / 0), [6] vertex labels above 2, [7] triangles with an index outside [0, nv), [8] kept, [9] mixed triangles
__global__ __launch_bounds__(256) void k_mesh_bounds(const float* xyz, const uint8_t* labels, size_t nv,
                                                     const int32_t* tri, size_t nt, uint32_t* out) {
  __shared__ uint32_t s[10];
  if (threadIdx.x < 10) s[threadIdx.x] = threadIdx.x < 3 ? 0xFFFFFFFFu : 0u;
  __syncthreads();
  uint32_t lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u}, bad_label = 0, bad_index = 0,
           kept = 0, mixed = 0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nv; i += (size_t)gridDim.x * 256)
    bad_label += labels[i] > 2u;
  for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < nt; t += (size_t)gridDim.x * 256) {
    int32_t i[3];
    float a[3], b[3], c[3];
    const int what = mesh_load(xyz, nv, tri, t, i, a, b, c);
    bad_index += what == 0;
    if (what != 2) continue;
    ++kept;
    const uint32_t l0 = labels[i[0]];
    mixed += labels[i[1]] != l0 || labels[i[2]] != l0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const uint32_t oa = score_ord(__float_as_uint(a[k])), ob = score_ord(__float_as_uint(b[k])),
                     oc = score_ord(__float_as_uint(c[k]));
      lo[k] = min(min(lo[k], oa), min(ob, oc));
      hi[k] = max(max(hi[k], oa), max(ob, oc));
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    atomicMin(&s[k], lo[k]);
    atomicMax(&s[3 + k], hi[k]);
  }
  atomicAdd(&s[6], bad_label);
  atomicAdd(&s[7], bad_index);
  atomicAdd(&s[8], kept);  // (at most 2^26 triangles)
  atomicAdd(&s[9], mixed);
  __syncthreads();
  if (threadIdx.x < 3) atomicMin(&out[threadIdx.x], s[threadIdx.x]);
  else if (threadIdx.x < 6) atomicMax(&out[threadIdx.x], s[threadIdx.x]);
  else if (threadIdx.x < 10) atomicAdd(&out[threadIdx.x], s[threadIdx.x]);
}

// *refs += the references the grid g would hold: per kept triangle the product of its box's cell spans
__global__ __launch_bounds__(256) void k_mesh_refs(const float* xyz, size_t nv, const int32_t* tri, size_t nt,
                                                   MeshGrid g, unsigned long long* refs) {
  __shared__ unsigned long long s;
  if (threadIdx.x == 0) s = 0ull;
  __syncthreads();
  unsigned long long mine = 0ull;
  for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < nt; t += (size_t)gridDim.x * 256) {
    int32_t i[3];
    float a[3], b[3], c[3];
    if (mesh_load(xyz, nv, tri, t, i, a, b, c) != 2) continue;
    int lo[3], hi[3];
    mesh_box_cells(g, a, b, c, lo, hi);
    mine += (unsigned long long)(hi[0] - lo[0] + 1) * (unsigned long long)(hi[1] - lo[1] + 1) *
            (unsigned long long)(hi[2] - lo[2] + 1);
  }
  if (mine) atomicAdd(&s, mine);
  __syncthreads();
  if (threadIdx.x == 0 && s) atomicAdd(refs, s);
}

// kMeshLanes lanes share a triangle's cells.  kFill == false: cnt[cell] += 1 per reference.  kFill == true: the
// references are written behind g.start (fill[] counts what a cell holds so far; the order inside a cell is whatever
// the atomics give: no result depends on it), and the triangle's first lane writes its record and its label byte.
// (`n_refs` guards the store: the caller's arrays must not change while the set is built, but if they do nothing is
// written outside the references)
template <bool kFill>
__global__ __launch_bounds__(256) void k_mesh_cells(const float* xyz, const uint8_t* labels, size_t nv,
                                                    const int32_t* tri, size_t nt, MeshGrid g, uint32_t* cnt,
                                                    uint32_t* ref, float4* rec, uint8_t* tlabel, uint32_t n_refs) {
  for (size_t w = (size_t)blockIdx.x * 256 + threadIdx.x; w < nt * kMeshLanes; w += (size_t)gridDim.x * 256) {
    const size_t t = w / kMeshLanes;
    const uint32_t sub = (uint32_t)(w % kMeshLanes);
    int32_t i[3];
    float a[3], b[3], c[3];
    if (mesh_load(xyz, nv, tri, t, i, a, b, c) != 2) continue;
    int lo[3], hi[3];
    mesh_box_cells(g, a, b, c, lo, hi);
    if (kFill && sub == 0) {
      rec[3 * t] = make_float4(a[0], a[1], a[2], __uint_as_float((uint32_t)t));
      rec[3 * t + 1] = make_float4(b[0], b[1], b[2], 0.f);
      rec[3 * t + 2] = make_float4(c[0], c[1], c[2], 0.f);
      tlabel[t] = labels[i[0]];
    }
    const uint32_t nx = (uint32_t)(hi[0] - lo[0] + 1), ny = (uint32_t)(hi[1] - lo[1] + 1),
                   nz = (uint32_t)(hi[2] - lo[2] + 1);
    const uint32_t cells = nx * ny * nz;  // (at most 2^24: the whole grid)
    for (uint32_t j = sub; j < cells; j += kMeshLanes) {
      const uint32_t x = j % nx, y = (j / nx) % ny, z = j / (nx * ny);
      const uint32_t cell = (uint32_t)(((lo[2] + (int)z) * g.cy + (lo[1] + (int)y)) * g.cx + (lo[0] + (int)x));
      if (kFill) {
        const uint32_t slot = g.start[cell] + atomicAdd(&cnt[cell], 1u);
        if (slot < n_refs) ref[slot] = (uint32_t)t;
      } else {
        atomicAdd(&cnt[cell], 1u);
      }
    }
  }
}

__device__ __forceinline__ float mesh_dot(float ux, float uy, float uz, float vx, float vy, float vz) {
  return __fadd_rn(__fadd_rn(__fmul_rn(ux, vx), __fmul_rn(uy, vy)), __fmul_rn(uz, vz));
}
__device__ __forceinline__ float mesh_clamp(float q, float a, float b, float c) {
  const float lo = fminf(fminf(a, b), c), hi = fmaxf(fmaxf(a, b), c);
  return q < lo ? lo : (q > hi ? hi : q);
}

// dist2 of the header: voxel position p, triangle A, B, C (their w words are not coordinates)
__device__ __forceinline__ float mesh_dist2(float px, float py, float pz, const float4 A, const float4 B,
                                            const float4 C) {
  const float abx = __fsub_rn(B.x, A.x), aby = __fsub_rn(B.y, A.y), abz = __fsub_rn(B.z, A.z);
  const float acx = __fsub_rn(C.x, A.x), acy = __fsub_rn(C.y, A.y), acz = __fsub_rn(C.z, A.z);
  const float apx = __fsub_rn(px, A.x), apy = __fsub_rn(py, A.y), apz = __fsub_rn(pz, A.z);
  const float d1 = mesh_dot(abx, aby, abz, apx, apy, apz), d2 = mesh_dot(acx, acy, acz, apx, apy, apz);
  float qx = A.x, qy = A.y, qz = A.z;
  if (!(d1 <= 0.f && d2 <= 0.f)) {
    const float bpx = __fsub_rn(px, B.x), bpy = __fsub_rn(py, B.y), bpz = __fsub_rn(pz, B.z);
    const float d3 = mesh_dot(abx, aby, abz, bpx, bpy, bpz), d4 = mesh_dot(acx, acy, acz, bpx, bpy, bpz);
    if (d3 >= 0.f && d4 <= d3) {
      qx = B.x, qy = B.y, qz = B.z;
    } else {
      const float vc = __fsub_rn(__fmul_rn(d1, d4), __fmul_rn(d3, d2));
      if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) {
        const float v = __fdiv_rn(d1, __fsub_rn(d1, d3));
        qx = __fadd_rn(A.x, __fmul_rn(v, abx)), qy = __fadd_rn(A.y, __fmul_rn(v, aby));
        qz = __fadd_rn(A.z, __fmul_rn(v, abz));
      } else {
        const float cpx = __fsub_rn(px, C.x), cpy = __fsub_rn(py, C.y), cpz = __fsub_rn(pz, C.z);
        const float d5 = mesh_dot(abx, aby, abz, cpx, cpy, cpz), d6 = mesh_dot(acx, acy, acz, cpx, cpy, cpz);
        if (d6 >= 0.f && d5 <= d6) {
          qx = C.x, qy = C.y, qz = C.z;
        } else {
          const float vb = __fsub_rn(__fmul_rn(d5, d2), __fmul_rn(d1, d6));
          if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) {
            const float w = __fdiv_rn(d2, __fsub_rn(d2, d6));
            qx = __fadd_rn(A.x, __fmul_rn(w, acx)), qy = __fadd_rn(A.y, __fmul_rn(w, acy));
            qz = __fadd_rn(A.z, __fmul_rn(w, acz));
          } else {
            const float va = __fsub_rn(__fmul_rn(d3, d6), __fmul_rn(d5, d4));
            const float e1 = __fsub_rn(d4, d3), e2 = __fsub_rn(d5, d6);
            if (va <= 0.f && e1 >= 0.f && e2 >= 0.f) {
              const float w = __fdiv_rn(e1, __fadd_rn(e1, e2));
              qx = __fadd_rn(B.x, __fmul_rn(w, __fsub_rn(C.x, B.x)));
              qy = __fadd_rn(B.y, __fmul_rn(w, __fsub_rn(C.y, B.y)));
              qz = __fadd_rn(B.z, __fmul_rn(w, __fsub_rn(C.z, B.z)));
            } else {
              const float den = __fdiv_rn(1.f, __fadd_rn(__fadd_rn(va, vb), vc));
              const float v = __fmul_rn(vb, den), w = __fmul_rn(vc, den);
              qx = __fadd_rn(__fadd_rn(A.x, __fmul_rn(abx, v)), __fmul_rn(acx, w));
              qy = __fadd_rn(__fadd_rn(A.y, __fmul_rn(aby, v)), __fmul_rn(acy, w));
              qz = __fadd_rn(__fadd_rn(A.z, __fmul_rn(abz, v)), __fmul_rn(acz, w));
            }
          }
        }
      }
    }
  }
  qx = mesh_clamp(qx, A.x, B.x, C.x), qy = mesh_clamp(qy, A.y, B.y, C.y), qz = mesh_clamp(qz, A.z, B.z, C.z);
  const float dx = __fsub_rn(qx, px), dy = __fsub_rn(qy, py), dz = __fsub_rn(qz, pz);
  return mesh_dot(dx, dy, dz, dx, dy, dz);
}

// the minimum of the key (dist2 bits << 32 | index) among the triangles with dist2 <= md2 (a NaN never is)
__device__ __forceinline__ void mesh_take(float d2, uint32_t idx, float md2, unsigned long long& best) {
  const unsigned long long k = ((unsigned long long)__float_as_uint(d2) << 32) | idx;
  if (d2 <= md2 && k < best) best = k;
}

// one voxel's place in the counts (LDS, laid out like ratsdf_label_score) and its per-voxel record
__device__ __forceinline__ int2 mesh_voxel(bool selected, unsigned long long key, float prob, const uint8_t* tlabel,
                                           const ScoreArgs& a, uint32_t* cnt) {
  if (!selected) return make_int2(-1, 0x7FC00000);
  atomicAdd(&cnt[1], 1u);
  if (key == kMeshNoKey) {
    atomicAdd(&cnt[2], 1u);
    return make_int2(-2, 0x7FC00000);
  }
  const uint32_t label = tlabel[(uint32_t)key];
  if (label == 0u) {
    atomicAdd(&cnt[3], 1u);
  } else {
    const bool high = label == 2u, pred = prob > a.p_cutoff;
    atomicAdd(&cnt[4 + (pred ? (high ? 0 : 1) : (high ? 2 : 3))], 1u);
    const int bin = prob >= 1.0f ? 255 : prob > 0.0f ? (int)(prob * 256.0f) : 0;
    atomicAdd(&cnt[8 + (high ? 256 : 0) + bin], 1u);
  }
  return make_int2((int)(uint32_t)key, (int)(uint32_t)(key >> 32));
}

// Blocks b = blockIdx.x, blockIdx.x + gridDim.x, ... of the selection list (the order of k_download: per-voxel record
// 512 b + v belongs to voxel v of block b).  `score` has been zeroed on the stream.
__global__ __launch_bounds__(kScoreWG) void k_score_mesh(Pool pool, const VisItem* sel, const uint32_t* n_sel,
                                                        float vs, MeshGrid g, ScoreArgs a, unsigned long long* score,
                                                        int2* per_voxel, long long capacity, long long* count) {
  __shared__ float4 recs[3 * kMeshChunk];
  __shared__ unsigned long long key[2 * kScoreWG];  // per voxel of the block: its best so far
  __shared__ uint32_t seg_start[2 * kScoreWG], seg_off[2 * kScoreWG];
  __shared__ uint32_t scan_lds[32];
  __shared__ uint32_t cnt[kScoreWords];
#ifndef RATSDF_SCORE_MESH_PLAIN
  __shared__ uint16_t list[2 * kScoreWG];  // the block's selected voxels
#endif
  const int tid = threadIdx.x;
  const uint32_t n = *n_sel;
  for (int i = tid; i < kScoreWords; i += kScoreWG) cnt[i] = 0u;
  if (blockIdx.x == 0 && tid == 0) {
    score[0] = (unsigned long long)n * 512ull;
    *count = (long long)n * 512ll;
  }
  __syncthreads();
  for (uint32_t b = blockIdx.x; b < n; b += gridDim.x) {  // uniform
    const VisItem it = sel[b];
    const int g0x = (int16_t)(it.x << 3), g0y = (int16_t)(it.y << 3), g0z = (int16_t)(it.z << 3);
    const size_t vi = ((size_t)it.idx << 9) + tid;
    const float t0 = pool.tsdf[vi], t1 = pool.tsdf[vi + 256];
    const bool sel0 = fabsf(t0) < a.tsdf_below && (pool.rgbw[vi] >> 24) >= a.min_weight;
    const bool sel1 = fabsf(t1) < a.tsdf_below && (pool.rgbw[vi + 256] >> 24) >= a.min_weight;
    key[tid] = kMeshNoKey;
    key[tid + kScoreWG] = kMeshNoKey;
    // the voxels this lane works for (v0, v1: -1 for none), on the triangles part, part + parts, ... of a chunk
    int v0 = -1, v1 = -1;
    uint32_t part = 0, parts = 1, S = 0;
#ifdef RATSDF_SCORE_MESH_PLAIN
    S = (uint32_t)__syncthreads_or(sel0 || sel1);
    v0 = sel0 ? tid : -1;
    v1 = sel1 ? tid + kScoreWG : -1;
#else
    {
      const uint32_t at = block_exclusive_scan((uint32_t)sel0 + (uint32_t)sel1, scan_lds, &S);
      if (sel0) list[at] = (uint16_t)tid;
      if (sel1) list[at + (uint32_t)sel0] = (uint16_t)(tid + kScoreWG);
      __syncthreads();
      if (S > (uint32_t)kScoreWG) {
        v0 = list[tid];
        if ((uint32_t)(tid + kScoreWG) < S) v1 = list[tid + kScoreWG];
      } else if (S) {
        parts = (uint32_t)kScoreWG / S;
        if ((uint32_t)tid < parts * S) {
          part = (uint32_t)tid / S;
          v0 = list[(uint32_t)tid - part * S];
        }
      }
    }
#endif
    const float q0x = (float)(g0x + (v0 & 7)) * vs, q0y = (float)(g0y + ((v0 >> 3) & 7)) * vs,
                q0z = (float)(g0z + ((v0 >> 6) & 7)) * vs;
    const float q1x = (float)(g0x + (v1 & 7)) * vs, q1y = (float)(g0y + ((v1 >> 3) & 7)) * vs,
                q1z = (float)(g0z + ((v1 >> 6) & 7)) * vs;
    unsigned long long k0 = kMeshNoKey, k1 = kMeshNoKey;
    if (S) {  // uniform
      // the cells the block's extent reaches, per axis (not clamped to the grid)
      const int lox = score_cell_open((float)g0x * vs, g.ox, g.cell),
                hix = score_cell_open((float)(g0x + 7) * vs, g.ox, g.cell);
      const int loy = score_cell_open((float)g0y * vs, g.oy, g.cell),
                hiy = score_cell_open((float)(g0y + 7) * vs, g.oy, g.cell);
      const int loz = score_cell_open((float)g0z * vs, g.oz, g.cell),
                hiz = score_cell_open((float)(g0z + 7) * vs, g.oz, g.cell);
      for (int r = 0;; ++r) {  // uniform
        // the cube of radius r and the one before it, clipped to the grid
        const int X0 = max(lox - r, 0), X1 = min(hix + r, g.cx - 1), Y0 = max(loy - r, 0), Y1 = min(hiy + r, g.cy - 1),
                  Z0 = max(loz - r, 0), Z1 = min(hiz + r, g.cz - 1);
        const int iX0 = max(lox - r + 1, 0), iX1 = min(hix + r - 1, g.cx - 1), iY0 = max(loy - r + 1, 0),
                  iY1 = min(hiy + r - 1, g.cy - 1), iZ0 = max(loz - r + 1, 0), iZ1 = min(hiz + r - 1, g.cz - 1);
        if (X0 <= X1 && Y0 <= Y1 && Z0 <= Z1) {
          const int ny = Y1 - Y0 + 1, nrows = ny * (Z1 - Z0 + 1);
          for (int row0 = 0; row0 < nrows; row0 += kScoreWG) {  // uniform: a row of cells per thread
            uint32_t s0 = 0, c0 = 0, s1 = 0, c1 = 0;
            const int i = row0 + tid;
            if (i < nrows) {
              const int y = Y0 + i % ny, z = Z0 + i / ny;
              const uint32_t base = (uint32_t)((z * g.cy + y) * g.cx);
              int a0 = X0, a1 = X1, b0 = 1, b1 = 0;  // the row's new cells: [a0, a1] and [b0, b1]
              if (r > 0 && y >= iY0 && y <= iY1 && z >= iZ0 && z <= iZ1) {
                a1 = min(iX0 - 1, X1);
                b0 = max(iX1 + 1, X0);
                b1 = X1;
              }
              if (a0 <= a1) {
                s0 = g.start[base + a0];
                c0 = g.start[base + a1 + 1] - s0;
              }
              if (b0 <= b1) {
                s1 = g.start[base + b0];
                c1 = g.start[base + b1 + 1] - s1;
              }
            }
            uint32_t total = 0;
            // (its two barriers stand between the last chunk's readers of the run tables and the writes below)
            const uint32_t ex = block_exclusive_scan(c0 + c1, scan_lds, &total);
            seg_start[2 * tid] = s0;
            seg_start[2 * tid + 1] = s1;
            seg_off[2 * tid] = ex;
            seg_off[2 * tid + 1] = ex + c0;
            __syncthreads();
            for (uint32_t k = 0; k < total; k += kMeshChunk) {  // uniform
              const uint32_t m = min((uint32_t)kMeshChunk, total - k);
              for (uint32_t j = tid; j < m; j += kScoreWG) {
                const uint32_t pos = k + j;
                uint32_t lo = 0, hi = 2 * kScoreWG;  // the last segment that starts at or before pos
                while (hi - lo > 1) {
                  const uint32_t mid = (lo + hi) >> 1;
                  if (seg_off[mid] <= pos) lo = mid; else hi = mid;
                }
                const size_t t = g.ref[seg_start[lo] + (pos - seg_off[lo])];
                recs[3 * j] = g.rec[3 * t];
                recs[3 * j + 1] = g.rec[3 * t + 1];
                recs[3 * j + 2] = g.rec[3 * t + 2];
              }
              __syncthreads();
              if (v0 >= 0) {
                for (uint32_t j = part; j < m; j += parts) {
                  const float4 A = recs[3 * j], B = recs[3 * j + 1], C = recs[3 * j + 2];
                  const uint32_t idx = __float_as_uint(A.w);
                  mesh_take(mesh_dist2(q0x, q0y, q0z, A, B, C), idx, a.md2, k0);
                  if (v1 >= 0) mesh_take(mesh_dist2(q1x, q1y, q1z, A, B, C), idx, a.md2, k1);
                }
              }
#ifdef RATSDF_SCORE_MESH_PLAIN
              else if (v1 >= 0) {
                for (uint32_t j = 0; j < m; ++j) {
                  const float4 A = recs[3 * j], B = recs[3 * j + 1], C = recs[3 * j + 2];
                  mesh_take(mesh_dist2(q1x, q1y, q1z, A, B, C), __float_as_uint(A.w), a.md2, k1);
                }
              }
#endif
              __syncthreads();
            }
          }
        }
        if (parts > 1) {  // uniform: the lanes of a voxel meet
          if (v0 >= 0 && k0 != kMeshNoKey) atomicMin(&key[v0], k0);
          __syncthreads();
          if (v0 >= 0) k0 = key[v0];
        }
        const double reach = (double)r * g.cell * (1.0 - 1e-5);
        const float bound = __double2float_rd(reach * reach);
        const bool done = (v0 < 0 || (k0 != kMeshNoKey ? __uint_as_float((uint32_t)(k0 >> 32)) : a.md2) < bound) &&
                          (v1 < 0 || (k1 != kMeshNoKey ? __uint_as_float((uint32_t)(k1 >> 32)) : a.md2) < bound);
        const bool whole = X0 == 0 && Y0 == 0 && Z0 == 0 && X1 == g.cx - 1 && Y1 == g.cy - 1 && Z1 == g.cz - 1;
        if (__syncthreads_and(done) || whole || r >= kMeshMaxRing) break;
      }
    }
    if (v0 >= 0 && k0 != kMeshNoKey) atomicMin(&key[v0], k0);
    if (v1 >= 0 && k1 != kMeshNoKey) atomicMin(&key[v1], k1);
    __syncthreads();
    const int2 r0 = mesh_voxel(sel0, key[tid], pool.segm[vi], g.label, a, cnt);
    const int2 r1 = mesh_voxel(sel1, key[tid + kScoreWG], pool.segm[vi + 256], g.label, a, cnt);
    const long long o = (long long)b * 512 + tid;
    if (per_voxel) {
      if (o < capacity) per_voxel[o] = r0;
      if (o + 256 < capacity) per_voxel[o + 256] = r1;
    }
  }
  __syncthreads();
  for (int i = 1 + tid; i < kScoreWords; i += kScoreWG)
    if (cnt[i]) atomicAdd(&score[i], (unsigned long long)cnt[i]);
}

}  // namespace ratsdf
