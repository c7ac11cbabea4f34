// kernels_resample.h -- transformed map fusion (include/ratsdf_resample.h): blocks of the DESTINATION lattice filled
// from a source map seen through a rigid pose, as block records {tsdf[512] | rgbw[512] | prob[512]} that the record
// path of fusion (fuse_chunk) takes.  No reference counterpart.
//
// One workgroup per destination block, lane = voxel.  A voxel is a trilinear sample of the source map: a chain of two
// dependent round trips, the directory probe and the voxels, as in k_sample -- but the 512 samples of a block are
// neighbours, so the probes are shared:
//   * the footprint of a destination block in the source lattice is a rotated cube of 7 voxel steps per side plus the
//     +1 corner.  With G's linear part A = I + (R^T - I) / |q|^2 and | |q|^2 - 1 | <= 1e-3 (the entry points refuse
//     anything else) a row of A has 1-norm <= sqrt(3) * 1.003, so along an axis the floors of the block's samples span
//     at most 7 * 1.74 = 12.2 steps: with m = the smallest floor of the block, every corner lies in [m, m + 14], and with
//     m = 8 * base + r, r <= 7, in [8 * base, 8 * base + 21] -- inside the 3 source blocks base .. base + 2.  fp32
//     rounding of g moves a floor by at most one step at the far end of the grid: there are two steps to spare.  So a
//     3 x 3 x 3 table at `base` covers every corner of every voxel.  (A corner outside the table -- impossible by the
//     above -- would read as an absent block, never out of bounds.)
//   * m comes from a minimum over the workgroup (a wave reduction, then one LDS atomic per wave), the 27 probes are made
//     by 27 lanes of the first wave side by side, and the pool indices sit in LDS (as k_marching_cubes keeps its
//     2 x 2 x 2);
//   * every voxel's 8 tsdf loads, 8 rgbw loads and the probability load are issued before any is used.  They are not
//     predicated: a corner that is not needed or whose block is absent reads voxel 0 of pool block 0, which exists, and
//     drops the value (kernels_sample.h explains why a branch around the loads would serialise them);
//   * the record leaves as three plain vector stores, lane = voxel: whole lines per wave and plane.
// The source map is only read.
#pragma once
#include <climits>

#include "kernels_fuse.h"

namespace ratsdf {

__global__ __launch_bounds__(512) void k_resample_blocks(Table tab, Pool pool, Se3 G, const int16_t* __restrict__ pos,
                                                         uint32_t* __restrict__ out, int32_t* __restrict__ contrib) {
  __shared__ int s_min[3];
  __shared__ int32_t s_blk[27];
  const uint32_t b = blockIdx.x;   // (the grid is the list)
  const uint32_t v = threadIdx.x;  // x + 8y + 64z
  const int dx = (int)pos[3 * b] * 8 + (int)(v & 7u), dy = (int)pos[3 * b + 1] * 8 + (int)((v >> 3) & 7u),
            dz = (int)pos[3 * b + 2] * 8 + (int)(v >> 6);
  // the contract of include/ratsdf_resample.h, evaluated as written (-ffp-contract=off)
  const V3 g = se3_apply(G, V3{(float)dx, (float)dy, (float)dz});
  const float lxf = floorf(g.x), lyf = floorf(g.y), lzf = floorf(g.z);
  const bool in_grid = cell_in_grid(lxf, lyf, lzf);
  const int lx = in_grid ? (int)lxf : 0, ly = in_grid ? (int)lyf : 0, lz = in_grid ? (int)lzf : 0;
  if (v < 3u) s_min[v] = INT_MAX;
  __syncthreads();
  {
    int mx = in_grid ? lx : INT_MAX, my = in_grid ? ly : INT_MAX, mz = in_grid ? lz : INT_MAX;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
      mx = min(mx, __shfl_xor(mx, s));
      my = min(my, __shfl_xor(my, s));
      mz = min(mz, __shfl_xor(mz, s));
    }
    if ((v & 63u) == 0u && mx != INT_MAX) {
      atomicMin(&s_min[0], mx);
      atomicMin(&s_min[1], my);
      atomicMin(&s_min[2], mz);
    }
  }
  __syncthreads();
  const bool any = s_min[0] != INT_MAX;  // (uniform) a voxel of the block falls inside the grid
  const int base_x = any ? s_min[0] >> 3 : 0, base_y = any ? s_min[1] >> 3 : 0, base_z = any ? s_min[2] >> 3 : 0;
  if (v < 27u) {
    const int x = base_x + (int)(v % 3u), y = base_y + (int)((v / 3u) % 3u), z = base_z + (int)(v / 9u);
    // (base >= -4096; a block past 4095 holds no voxel of the grid)
    s_blk[v] = any && x <= 4095 && y <= 4095 && z <= 4095 ? lookup_block(tab, x, y, z) : -1;
  }
  __syncthreads();

  const float fx = g.x - lxf, fy = g.y - lyf, fz = g.z - lzf;
  const float ux = 1.f - fx, uy = 1.f - fy, uz = 1.f - fz;
  // corner index i on an axis is needed iff its weight factor is not zero (u for 0, f for 1)
  const bool qx[2] = {in_grid && ux != 0.f, in_grid && fx != 0.f}, qy[2] = {uy != 0.f, fy != 0.f},
             qz[2] = {uz != 0.f, fz != 0.f};
  // per axis and corner index: the block's place in the table (times its stride) and the voxel's offset in the block
  int tx[2], ty[2], tz[2], ox[2], oy[2], oz[2];
  bool ix[2], iy[2], iz[2];  // ... inside the table
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int rx = ((lx + i) >> 3) - base_x, ry = ((ly + i) >> 3) - base_y, rz = ((lz + i) >> 3) - base_z;
    ix[i] = (unsigned)rx < 3u;
    iy[i] = (unsigned)ry < 3u;
    iz[i] = (unsigned)rz < 3u;
    tx[i] = ix[i] ? rx : 0;
    ty[i] = iy[i] ? ry * 3 : 0;
    tz[i] = iz[i] ? rz * 9 : 0;
    ox[i] = (lx + i) & 7;
    oy[i] = ((ly + i) & 7) * 8;
    oz[i] = ((lz + i) & 7) * 64;
  }
  float t[8];
  uint32_t c[8];
  size_t at[8];
  bool need[8], have[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {  // corner k: x + (k >> 2), y + ((k >> 1) & 1), z + (k & 1) -- t000 .. t111
    const int i = k >> 2, j = (k >> 1) & 1, l = k & 1;
    need[k] = qx[i] && qy[j] && qz[l];
    const int32_t blk = s_blk[tx[i] + ty[j] + tz[l]];
    have[k] = need[k] && ix[i] && iy[j] && iz[l] && blk >= 0;
    at[k] = have[k] ? ((size_t)blk << 9) + (size_t)(ox[i] + oy[j] + oz[l]) : 0;
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    t[k] = pool.tsdf[at[k]];
    c[k] = pool.rgbw[at[k]];
  }
  // the nearest voxel: roundf (half away from zero) is floor or floor + 1, always a needed corner
  const int kn = ((roundf(g.x) != lxf) << 2) | ((roundf(g.y) != lyf) << 1) | (int)(roundf(g.z) != lzf);
  size_t an = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k)
    if (k == kn) an = at[k];
  const uint32_t prob = __float_as_uint(pool.segm[an]);

  bool ok = in_grid;
  uint32_t wmin = 255u, cn = 0u;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    if (need[k]) {
      ok = ok && have[k] && fuse_contributes(c[k], __float_as_uint(t[k]));
      wmin = min(wmin, c[k] >> 24);
    } else {
      t[k] = 0.f;  // (not looked at: reads as 0.0f in the formula)
    }
    if (k == kn) cn = c[k];
  }
  const float tsdf = trilinear(t, fx, fy, fz, ux, uy, uz).value;
  uint32_t* rec = out + (size_t)b * 1536u + v;
  rec[0] = ok ? __float_as_uint(tsdf) : 0u;
  rec[512] = ok ? (cn & 0x00FFFFFFu) | (wmin << 24) : 0u;
  rec[1024] = ok ? prob : 0u;
  const int n_ok = __syncthreads_count(ok);
  if (v == 0u && contrib) contrib[b] = n_ok;
}

// A chunk of resampled candidates before fuse_chunk: a block without a contributing voxel is marked done from the
// start (it is never allocated, never looked at again: as k_fuse_unpack treats an entry that names no block); the
// others are counted.
__global__ __launch_bounds__(256) void k_resample_mark(const int32_t* contrib, uint32_t n, uint32_t* done,
                                                       FuseCounters* cnt) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  if (contrib[i] != 0) atomicAdd(&cnt->listed, 1u);  // (one add per wave: the compiler sums the active lanes)
  else atomicOr(&done[i >> 5], 1u << (i & 31u));
}

}  // namespace ratsdf
