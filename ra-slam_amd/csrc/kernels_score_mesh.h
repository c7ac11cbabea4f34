// kernels_score_mesh.h -- the map scored against a labelled triangle mesh (include/ratsdf_score_mesh.h) for gfx950:
// the build of a mesh set (bounds and validation -> references per cell -> scan -> scatter into a dense grid of cells)
// and the join "every selected voxel -> its nearest kept triangle" with the counts that follow from it.
//
// The join walks the selection list of k_score_labels, one 256-thread workgroup per map block at a time, and the rings
// of cells around the block with the same function (score_walk, kernels_score.h): a cell references every kept triangle
// whose axis-aligned box meets it, each ring's references are resolved to 48-byte triangle records and staged in LDS in
// chunks of kMeshChunk.
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
// The grid only accelerates, and score_walk's argument for where the walk may stop holds with a triangle's box in the
// place of a point: the closest point q of a triangle is clamped to the triangle's box, so dist2 is at least the
// squared distance from the voxel to that box along any axis, up to the rounding of one subtraction and one product
// (2^-22 relative, a point's margin), and a triangle that has not been looked at after ring r has its box, along some
// axis, at least r whole cells beyond the block's extent.
#pragma once
#include "kernels_score.h"

namespace ratsdf {

#ifndef RATSDF_SCORE_MESH_CHUNK
#define RATSDF_SCORE_MESH_CHUNK 256
#endif
constexpr int kMeshChunk = RATSDF_SCORE_MESH_CHUNK;  // 48-byte triangle records per LDS chunk (256: 12 KiB)
constexpr int kMeshLanes = 8;                        // lanes that share the cells of one triangle's box in the build
constexpr unsigned long long kMeshNoKey = ~0ull;
#ifdef RATSDF_SCORE_MESH_PLAIN
constexpr bool kMeshPlain = true;
#else
constexpr bool kMeshPlain = false;
#endif

// the device side of a mesh set, by value
struct MeshGrid : CellGrid {
  const float4* rec;      // three per ORIGINAL triangle index, written for kept ones: {a, index bits}, {b, 0}, {c, 0}
  const uint32_t* ref;    // original indices of kept triangles, sorted by cell
  const uint8_t* label;   // one byte per original triangle index: the label of its first vertex
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

// the dist2 that the voxel of key k has still to beat (score_walk's best): its own, md2 while it has no match
__device__ __forceinline__ float mesh_to_beat(unsigned long long k, float md2) {
  return k != kMeshNoKey ? __uint_as_float((uint32_t)(k >> 32)) : md2;
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
    if (kMeshPlain) {
      S = (uint32_t)__syncthreads_or(sel0 || sel1);
      v0 = sel0 ? tid : -1;
      v1 = sel1 ? tid + kScoreWG : -1;
    } else {
      __shared__ uint16_t list[2 * kScoreWG];  // the block's selected voxels
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
    const float q0x = (float)(g0x + (v0 & 7)) * vs, q0y = (float)(g0y + ((v0 >> 3) & 7)) * vs,
                q0z = (float)(g0z + ((v0 >> 6) & 7)) * vs;
    const float q1x = (float)(g0x + (v1 & 7)) * vs, q1y = (float)(g0y + ((v1 >> 3) & 7)) * vs,
                q1z = (float)(g0z + ((v1 >> 6) & 7)) * vs;
    unsigned long long k0 = kMeshNoKey, k1 = kMeshNoKey;
    if (S)  // uniform
      score_walk<kMeshChunk>(
          g, g0x, g0y, g0z, vs, seg_start, seg_off, scan_lds,
          [&](uint32_t pos, uint32_t j) {
            const size_t t = g.ref[pos];
            recs[3 * j] = g.rec[3 * t];
            recs[3 * j + 1] = g.rec[3 * t + 1];
            recs[3 * j + 2] = g.rec[3 * t + 2];
          },
          [&](uint32_t m) {
            if (v0 >= 0) {
              for (uint32_t j = part; j < m; j += parts) {
                const float4 A = recs[3 * j], B = recs[3 * j + 1], C = recs[3 * j + 2];
                const uint32_t idx = __float_as_uint(A.w);
                mesh_take(mesh_dist2(q0x, q0y, q0z, A, B, C), idx, a.md2, k0);
                if (v1 >= 0) mesh_take(mesh_dist2(q1x, q1y, q1z, A, B, C), idx, a.md2, k1);
              }
            } else if (kMeshPlain && v1 >= 0) {  // (only that layout has lanes that hold a second voxel alone)
              for (uint32_t j = 0; j < m; ++j) {
                const float4 A = recs[3 * j], B = recs[3 * j + 1], C = recs[3 * j + 2];
                mesh_take(mesh_dist2(q1x, q1y, q1z, A, B, C), __float_as_uint(A.w), a.md2, k1);
              }
            }
          },
          [&] {
            if (parts > 1) {  // uniform: the lanes of a voxel meet
              if (v0 >= 0 && k0 != kMeshNoKey) atomicMin(&key[v0], k0);
              __syncthreads();
              if (v0 >= 0) k0 = key[v0];
            }
            return fmaxf(v0 >= 0 ? mesh_to_beat(k0, a.md2) : -1.f, v1 >= 0 ? mesh_to_beat(k1, a.md2) : -1.f);
          });
    if (v0 >= 0 && k0 != kMeshNoKey) atomicMin(&key[v0], k0);
    if (v1 >= 0 && k1 != kMeshNoKey) atomicMin(&key[v1], k1);
    __syncthreads();
    const unsigned long long e0 = key[tid], e1 = key[tid + kScoreWG];
    const int2 r0 = score_voxel(sel0, e0 != kMeshNoKey, (int)(uint32_t)e0, (uint32_t)(e0 >> 32), pool.segm[vi],
                                g.label, a, cnt);
    const int2 r1 = score_voxel(sel1, e1 != kMeshNoKey, (int)(uint32_t)e1, (uint32_t)(e1 >> 32), pool.segm[vi + 256],
                                g.label, a, cnt);
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
