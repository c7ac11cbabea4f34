// kernels_score.h -- the map scored against labelled points (include/ratsdf_score.h) for gfx950: the build of a label
// set (bounds -> count -> scan -> scatter into a dense grid of cells) and the join "every selected voxel -> its nearest
// labelled point" with the counts that follow from it.
//
// The join runs one 256-thread workgroup per map block at a time, two voxels per thread (v and v + 256: the same x
// and y, z four apart, so dx * dx + dy * dy is computed once).  The 512 voxels of a block span 8 voxel sizes -- one
// cell of the default grid -- and therefore share their candidate cells: the workgroup walks the cube of cells around
// the block ring by ring (Chebyshev radius r), copies each ring's points into LDS in chunks of kScoreChunk 16-byte
// records and every thread scans the chunk for its two voxels.  An LDS read of a record is one address for the whole
// wave (a broadcast: no bank conflict), so the inner loop is one ds_read_b128 and eleven fp32 operations per point and
// thread; points are fetched from memory once per block, not once per voxel.
//
// The grid only accelerates: the result is defined by the fp32 d2 of each pair (ratsdf_score.h).  The walk over the
// rings, which the mesh join (kernels_score_mesh.h) shares, and the argument for where it may stop are score_walk's.
#pragma once
#include "kernels_mesh.h"

namespace ratsdf {

constexpr int kScoreWG = 256;
#ifndef RATSDF_SCORE_CHUNK
#define RATSDF_SCORE_CHUNK 1024
#endif
constexpr int kScoreChunk = RATSDF_SCORE_CHUNK;  // 16-byte records per LDS chunk (1024: 16 KiB; DESIGN 4 "Label score")
constexpr int kScoreMaxRing = 192;   // of both joins; never reached with max_dist <= 64 * cell: a guard, not a contract
constexpr int kScoreWords = 520;     // int64 words of ratsdf_label_score
constexpr int kOpenCell = 1 << 30;   // cell indices of query positions are clamped to +- this

// the dense grid of cells of a set (of points, or of a mesh's triangles): what score_walk reads
struct CellGrid {
  const uint32_t* start;   // cells + 1 words: where each cell's records start in the list sorted by cell
  double ox, oy, oz, cell;
  int cx, cy, cz;
};

// the device side of a label set, by value
struct LabelGrid : CellGrid {
  const float4* rec;       // kept points {x, y, z, original index as bits}, sorted by cell
  const uint8_t* label;    // one byte per original index
};

// monotone map of the finite floats (and the infinities) to unsigned words
__device__ __host__ inline uint32_t score_ord(uint32_t bits) {
  return bits ^ ((bits >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __host__ inline uint32_t score_unord(uint32_t o) {
  return o ^ ((o >> 31) ? 0x80000000u : 0xFFFFFFFFu);
}
__device__ inline bool score_finite(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }

// the cell of a coordinate along one axis: floor((p - o) / cell) in double precision, not clamped to the grid ...
__device__ inline int score_cell_open(float p, double o, double cell) {
  double u = floor(((double)p - o) / cell);
  u = u < -(double)kOpenCell ? -(double)kOpenCell : u;
  u = u > (double)kOpenCell ? (double)kOpenCell : u;
  return (int)u;
}
// ... and of a kept point (inside the bounding box by construction; the clamp only keeps memory safe)
__device__ inline int score_cell(float p, double o, double cell, int c) {
  const int u = score_cell_open(p, o, cell);
  return u < 0 ? 0 : u > c - 1 ? c - 1 : u;
}
__device__ inline uint32_t score_point_cell(const CellGrid& g, float x, float y, float z) {
  const int ix = score_cell(x, g.ox, g.cell, g.cx), iy = score_cell(y, g.oy, g.cell, g.cy),
            iz = score_cell(z, g.oz, g.cell, g.cz);
  return (uint32_t)((iz * g.cy + iy) * g.cx + ix);
}

// out: [0..2] smallest, [3..5] largest coordinate of the kept points as score_ord words (initialised to ~0 / 0),
// [6] labels above 2, [8..9] kept points as a 64-bit count
__global__ __launch_bounds__(256) void k_label_bounds(const float* xyz, const uint8_t* labels, size_t n,
                                                      uint32_t* out) {
  __shared__ uint32_t s[8];
  if (threadIdx.x < 8) s[threadIdx.x] = threadIdx.x < 3 ? 0xFFFFFFFFu : 0u;
  __syncthreads();
  uint32_t lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u}, bad = 0, kept = 0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    bad += labels[i] > 2u;
    if (!(score_finite(x) && score_finite(y) && score_finite(z))) continue;
    ++kept;
    const uint32_t o[3] = {score_ord(__float_as_uint(x)), score_ord(__float_as_uint(y)), score_ord(__float_as_uint(z))};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      lo[a] = o[a] < lo[a] ? o[a] : lo[a];
      hi[a] = o[a] > hi[a] ? o[a] : hi[a];
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    atomicMin(&s[a], lo[a]);
    atomicMax(&s[3 + a], hi[a]);
  }
  atomicAdd(&s[6], bad);
  atomicAdd(&s[7], kept);  // (at most 2^26 points)
  __syncthreads();
  if (threadIdx.x < 3) atomicMin(&out[threadIdx.x], s[threadIdx.x]);
  else if (threadIdx.x < 6) atomicMax(&out[threadIdx.x], s[threadIdx.x]);
  else if (threadIdx.x == 6) atomicAdd(&out[6], s[6]);
  else if (threadIdx.x == 7) atomicAdd((unsigned long long*)(out + 8), (unsigned long long)s[7]);
}

__global__ __launch_bounds__(256) void k_label_count(const float* xyz, size_t n, LabelGrid g, uint32_t* cnt) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    if (score_finite(x) && score_finite(y) && score_finite(z)) atomicAdd(&cnt[score_point_cell(g, x, y, z)], 1u);
  }
}

// (the order inside a cell is whatever the atomics give: no result depends on it)
// (`kept` guards the store: the caller's points must not change while the set is built, but if they do nothing is
// written outside the records)
__global__ __launch_bounds__(256) void k_label_scatter(const float* xyz, size_t n, LabelGrid g, uint32_t* fill,
                                                       float4* rec, uint32_t kept) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    if (!(score_finite(x) && score_finite(y) && score_finite(z))) continue;
    const uint32_t c = score_point_cell(g, x, y, z);
    const uint32_t slot = g.start[c] + atomicAdd(&fill[c], 1u);
    if (slot < kept) rec[slot] = make_float4(x, y, z, __uint_as_float((uint32_t)i));
  }
}

struct ScoreArgs {
  float tsdf_below, md2, p_cutoff;
  uint32_t min_weight;
};

// the lexicographic minimum of (d2, index) among the points with d2 <= md2
__device__ __forceinline__ void score_take(float d2, int idx, float md2, float& best, int& bi) {
  if (d2 <= md2 && (d2 < best || (d2 == best && idx < bi))) {
    best = d2;
    bi = idx;
  }
}

// one voxel's place in the counts (LDS, laid out like ratsdf_label_score) and its per-voxel record; `matched`: it has
// a nearest record, of original index `index` at the distance whose square has the bits `d2_bits`
__device__ __forceinline__ int2 score_voxel(bool selected, bool matched, int index, uint32_t d2_bits, float prob,
                                            const uint8_t* labels, const ScoreArgs& a, uint32_t* cnt) {
  if (!selected) return make_int2(-1, 0x7FC00000);
  atomicAdd(&cnt[1], 1u);
  if (!matched) {
    atomicAdd(&cnt[2], 1u);
    return make_int2(-2, 0x7FC00000);
  }
  const uint32_t label = labels[index];
  if (label == 0u) {
    atomicAdd(&cnt[3], 1u);
  } else {
    const bool high = label == 2u, pred = prob > a.p_cutoff;
    atomicAdd(&cnt[4 + (pred ? (high ? 0 : 1) : (high ? 2 : 3))], 1u);
    const int bin = prob >= 1.0f ? 255 : prob > 0.0f ? (int)(prob * 256.0f) : 0;
    atomicAdd(&cnt[8 + (high ? 256 : 0) + bin], 1u);
  }
  return make_int2(index, (int)d2_bits);
}

// The walk of both joins: a workgroup of kScoreWG threads visits the cells around the map block whose first voxel is
// (g0x, g0y, g0z), ring by ring (Chebyshev radius r around the cells the block's extent reaches), until no selected
// voxel of the block can gain from anything further out.  A thread takes a row of a ring's cells and notes the row's
// (at most two) runs of new cells as runs of the list sorted by cell; a block scan lines the runs up, and the ring's
// records go by in chunks of kChunk:
//   stage(pos, j)  record `pos` of the sorted list goes to slot j of the chunk (each slot by one thread)
//   consume(m)     a staged chunk of m records is there for every thread; a barrier follows
//   best()         after a ring, by every thread (it may hold barriers): the largest d2 that a voxel this thread works
//                  for has still to beat -- its best so far, md2 while it has no match -- or a negative number if the
//                  thread works for no voxel
// seg_start, seg_off (2 * kScoreWG words each) and scan_lds (32 words) are LDS for the walk alone.
//
// Where it may stop.  Cell indices are computed in double precision, by the same function when the set is built and
// when it is searched.  After ring r every record that has not been looked at lies, along some axis, at least r whole
// cells beyond the block's extent, up to the rounding of that double arithmetic (at most cell * 2^-28: the grid has at
// most 2^24 cells per axis); the fp32 d2 of a point is within 2^-22 (relative) of the square of its true distance.
// The bound (r * cell * (1 - 1e-5))^2, rounded down to fp32, is below both, so a voxel whose best d2 is strictly below
// it -- or, without a match, whose max_dist^2 is -- cannot gain or tie with anything further out.  The walk ends when
// that holds for every selected voxel, or when the cube covers the whole grid.  max_dist <= 64 * cell bounds the rings
// at 66.
template <int kChunk, class Stage, class Consume, class Best>
__device__ __forceinline__ void score_walk(const CellGrid& g, int g0x, int g0y, int g0z, float vs, uint32_t* seg_start,
                                           uint32_t* seg_off, uint32_t* scan_lds, Stage stage, Consume consume,
                                           Best best) {
  const int tid = threadIdx.x;
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
        for (uint32_t k = 0; k < total; k += kChunk) {  // uniform
          const uint32_t m = min((uint32_t)kChunk, total - k);
          for (uint32_t j = tid; j < m; j += kScoreWG) {
            const uint32_t pos = k + j;
            uint32_t lo = 0, hi = 2 * kScoreWG;  // the last segment that starts at or before pos
            while (hi - lo > 1) {
              const uint32_t mid = (lo + hi) >> 1;
              if (seg_off[mid] <= pos) lo = mid; else hi = mid;
            }
            stage(seg_start[lo] + (pos - seg_off[lo]), j);
          }
          __syncthreads();
          consume(m);
          __syncthreads();
        }
      }
    }
    const double reach = (double)r * g.cell * (1.0 - 1e-5);
    const float bound = __double2float_rd(reach * reach);
    const bool done = best() < bound;
    const bool whole = X0 == 0 && Y0 == 0 && Z0 == 0 && X1 == g.cx - 1 && Y1 == g.cy - 1 && Z1 == g.cz - 1;
    if (__syncthreads_and(done) || whole || r >= kScoreMaxRing) break;
  }
}

// Blocks b = blockIdx.x, blockIdx.x + gridDim.x, ... of the selection list (the order of k_download: per-voxel record
// 512 b + v belongs to voxel v of block b).  `score` has been zeroed on the stream.
__global__ __launch_bounds__(kScoreWG) void k_score_labels(Pool pool, const VisItem* sel, const uint32_t* n_sel,
                                                          float vs, LabelGrid g, ScoreArgs a,
                                                          unsigned long long* score, int2* per_voxel,
                                                          long long capacity, long long* count) {
  __shared__ float4 pts[kScoreChunk];
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
  const int tx = tid & 7, ty = (tid >> 3) & 7, tz = tid >> 6;
  for (uint32_t b = blockIdx.x; b < n; b += gridDim.x) {  // uniform
    const VisItem it = sel[b];
    const int g0x = (int16_t)(it.x << 3), g0y = (int16_t)(it.y << 3), g0z = (int16_t)(it.z << 3);
    const float qx = (float)(g0x + tx) * vs, qy = (float)(g0y + ty) * vs;
    const float qz0 = (float)(g0z + tz) * vs, qz1 = (float)(g0z + tz + 4) * vs;
    const size_t vi = ((size_t)it.idx << 9) + tid;
    const float t0 = pool.tsdf[vi], t1 = pool.tsdf[vi + 256];
    const bool sel0 = fabsf(t0) < a.tsdf_below && (pool.rgbw[vi] >> 24) >= a.min_weight;
    const bool sel1 = fabsf(t1) < a.tsdf_below && (pool.rgbw[vi + 256] >> 24) >= a.min_weight;
    float best0 = __uint_as_float(0x7F800000u), best1 = best0;
    int bi0 = 0x7FFFFFFF, bi1 = 0x7FFFFFFF;
    if (__syncthreads_or(sel0 || sel1))
      score_walk<kScoreChunk>(
          g, g0x, g0y, g0z, vs, seg_start, seg_off, scan_lds, [&](uint32_t pos, uint32_t j) { pts[j] = g.rec[pos]; },
          [&](uint32_t m) {
#pragma unroll 4
            for (uint32_t j = 0; j < m; ++j) {
              const float4 p = pts[j];
              const int idx = (int)__float_as_uint(p.w);
              const float dx = __fsub_rn(p.x, qx), dy = __fsub_rn(p.y, qy);
              const float dz0 = __fsub_rn(p.z, qz0), dz1 = __fsub_rn(p.z, qz1);
              const float dxy = __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy));
              score_take(__fadd_rn(dxy, __fmul_rn(dz0, dz0)), idx, a.md2, best0, bi0);
              score_take(__fadd_rn(dxy, __fmul_rn(dz1, dz1)), idx, a.md2, best1, bi1);
            }
          },
          [&] {
            return fmaxf(sel0 ? (bi0 != 0x7FFFFFFF ? best0 : a.md2) : -1.f,
                         sel1 ? (bi1 != 0x7FFFFFFF ? best1 : a.md2) : -1.f);
          });
    const int2 r0 = score_voxel(sel0, bi0 != 0x7FFFFFFF, bi0, __float_as_uint(best0), pool.segm[vi], g.label, a, cnt);
    const int2 r1 =
        score_voxel(sel1, bi1 != 0x7FFFFFFF, bi1, __float_as_uint(best1), pool.segm[vi + 256], g.label, a, cnt);
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
