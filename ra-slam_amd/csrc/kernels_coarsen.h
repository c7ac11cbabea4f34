// kernels_coarsen.h -- map coarsening (include/ratsdf_coarsen.h): blocks of the lattice of twice the voxel size filled
// from a source map by full weighting over the taps that exist, as block records {tsdf[512] | rgbw[512] | prob[512]}
// that the record path of fusion (fuse_chunk) takes.  No reference counterpart.
//
// One workgroup per coarse block B, lane = coarse voxel.  Coarse voxel D = 8B + local sits on fine voxel 2D, so the 27
// taps of the block's 512 voxels span the fine voxels 16B - 1 .. 16B + 15 per axis: a 17^3 region inside the 3 x 3 x 3
// fine blocks at 2B - 1, of which the low column holds only the halo plane (local index 7) and the upper 2 x 2 x 2 hold
// the centres.
//   * 27 lanes of the first wave make the directory probes side by side; the pool indices sit in LDS (as
//     k_resample_blocks keeps its table).  A fine block outside [-4096, 4095] is absent: a tap never wraps around.
//   * the workgroup stages the 4913 fine voxels into LDS, one 17-voxel row after the other: the tsdf as a float and
//     the weight as a byte, both 0 where the tap is absent (block missing, weight 0 or the fresh voxel) -- so the sum
//     below needs no branch, and a NaN in a voxel that does not count never reaches it.  An absent block reads pool
//     block 0, which exists, and drops the value.
//   * LDS layout: the lanes of a wave step through a row at stride two, and with the dword rows of `ds_read_b32`
//     (32 banks per half wave) a plain row would use every second bank.  So a row keeps its even fine voxels in words
//     0 .. 8 and its odd ones in words 9 .. 16: for one tap offset the 8 x-lanes read 8 consecutive words.  A half wave
//     is 8 x by 4 y, its rows two apart: with a row pitch of 20 words they start at banks 0, 8, 16, 24 -- no conflict.
//     20 * 17 * 17 floats + as many bytes = 28.2 KiB: four workgroups share a CU's 160 KiB.
//   * the 27 taps are summed from LDS in the contract's order; the centre's colour word and probability come from the
//     pool (lines the staging just touched); the record leaves as three plain vector stores, lane = voxel.
// The source map is only read.
#pragma once
#include "kernels_fuse.h"

namespace ratsdf {

constexpr int kCoarsenPitch = 20;                       // words per staged row of 17 fine voxels
constexpr int kCoarsenPlane = kCoarsenPitch * 17;       // ... per plane of 17 rows
constexpr int kCoarsenWords = kCoarsenPlane * 17;       // 5780
constexpr int kCoarsenRegion = 17 * 17 * 17;            // 4913 fine voxels
constexpr int kCoarsenSteps = (kCoarsenRegion + 511) / 512;

// word of fine voxel f (0 .. 16, counted from 16B - 1) within its staged row: even ones first
__device__ inline int coarsen_col(int f) { return (f >> 1) + (f & 1) * 9; }

__global__ __launch_bounds__(512) void k_coarsen_blocks(Table tab, Pool pool, const int16_t* __restrict__ pos,
                                                        uint32_t* __restrict__ out, int32_t* __restrict__ contrib) {
  __shared__ float s_t[kCoarsenWords];
  __shared__ uint8_t s_w[kCoarsenWords];
  __shared__ int32_t s_blk[27];
  const uint32_t b = blockIdx.x;   // (the grid is the list)
  const uint32_t v = threadIdx.x;  // x + 8y + 64z
  const int bx = pos[3 * b], by = pos[3 * b + 1], bz = pos[3 * b + 2];
  if (v < 27u) {
    const int x = 2 * bx - 1 + (int)(v % 3u), y = 2 * by - 1 + (int)((v / 3u) % 3u), z = 2 * bz - 1 + (int)(v / 9u);
    s_blk[v] = block_in_grid(x, y, z) ? lookup_block(tab, x, y, z) : -1;
  }
  __syncthreads();

  // staging: item = fine voxel of the region, x fastest; every load is issued before the first LDS write
  float st[kCoarsenSteps];
  uint32_t sc[kCoarsenSteps];
  bool have[kCoarsenSteps];
#pragma unroll
  for (int k = 0; k < kCoarsenSteps; ++k) {
    const uint32_t item = min((uint32_t)k * 512u + v, (uint32_t)kCoarsenRegion - 1u);  // (the tail repeats the last)
    const uint32_t fx = item % 17u, row = item / 17u, fy = row % 17u, fz = row / 17u;
    const uint32_t tx = fx + 7u, ty = fy + 7u, tz = fz + 7u;  // block of the table = t >> 3, voxel in it = t & 7
    const int32_t blk = s_blk[(tx >> 3) + (ty >> 3) * 3u + (tz >> 3) * 9u];
    have[k] = blk >= 0;
    const size_t at = have[k] ? ((size_t)blk << 9) + (size_t)((tx & 7u) + (ty & 7u) * 8u + (tz & 7u) * 64u) : 0;
    st[k] = pool.tsdf[at];
    sc[k] = pool.rgbw[at];
  }
#pragma unroll
  for (int k = 0; k < kCoarsenSteps; ++k) {
    const uint32_t item = (uint32_t)k * 512u + v;
    if (item < (uint32_t)kCoarsenRegion) {
      const uint32_t fx = item % 17u, row = item / 17u, fy = row % 17u, fz = row / 17u;
      const bool present = have[k] && fuse_contributes(sc[k], __float_as_uint(st[k]));
      const int w = (int)fz * kCoarsenPlane + (int)fy * kCoarsenPitch + coarsen_col((int)fx);
      s_t[w] = present ? st[k] : 0.f;
      s_w[w] = present ? (uint8_t)(sc[k] >> 24) : (uint8_t)0;
    }
  }

  // the centre: fine voxel 2 * local + 1 of the region, in the upper 2 x 2 x 2 of the table
  const int x = (int)(v & 7u), y = (int)((v >> 3) & 7u), z = (int)(v >> 6);
  const int32_t cblk = s_blk[(1 + (x >> 2)) + (1 + (y >> 2)) * 3 + (1 + (z >> 2)) * 9];
  const size_t cat = cblk >= 0 ? ((size_t)cblk << 9) + (size_t)(((2 * x) & 7) + ((2 * y) & 7) * 8 + ((2 * z) & 7) * 64) : 0;
  const uint32_t crgbw = pool.rgbw[cat];
  const uint32_t cprob = __float_as_uint(pool.segm[cat]);
  __syncthreads();

  // the contract of include/ratsdf_coarsen.h, evaluated as written (-ffp-contract=off): oz, oy, ox, ox fastest
  float num = 0.f, den = 0.f;
#pragma unroll
  for (int oz = -1; oz <= 1; ++oz)
#pragma unroll
    for (int oy = -1; oy <= 1; ++oy) {
      const int rowat = (2 * z + 1 + oz) * kCoarsenPlane + (2 * y + 1 + oy) * kCoarsenPitch;
#pragma unroll
      for (int ox = -1; ox <= 1; ++ox) {
        // fine voxel 2x + 1 + ox: the odd one (ox == 0) is word 9 + x, the even ones are words x and x + 1
        const int w = rowat + (ox == 0 ? 9 + x : x + (ox + 1) / 2);
        const float k = (float)((2 - (ox < 0 ? -ox : ox)) * (2 - (oy < 0 ? -oy : oy)) * (2 - (oz < 0 ? -oz : oz)));
        const float c = k * (float)s_w[w];
        num = num + c * s_t[w];
        den = den + c;
      }
    }
  const int cw = (2 * z + 1) * kCoarsenPlane + (2 * y + 1) * kCoarsenPitch + 9 + x;
  const bool ok = s_w[cw] != 0;  // the centre tap is present (a present tap has a weight)
  const float tsdf = num / den;
  uint32_t* rec = out + (size_t)b * 1536u + v;
  rec[0] = ok ? __float_as_uint(tsdf) : 0u;
  rec[512] = ok ? crgbw : 0u;
  rec[1024] = ok ? cprob : 0u;
  const int n_ok = __syncthreads_count(ok);
  if (v == 0u && contrib) contrib[b] = n_ok;
}

}  // namespace ratsdf
