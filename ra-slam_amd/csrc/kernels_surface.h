// kernels_surface.h -- oriented surface points of a box of the map (include/ratsdf_surface.h): sign changes of the
// TSDF between neighbouring voxels, as position / normal / probability / colour records in the header's order.  No
// reference counterpart.
//
// One 512-thread workgroup per cell of the box's block grid (x fastest: the cell index IS the header's block order),
// one lane per voxel of the block (lane = x + 8 y + 64 z: the order within the block), run twice:
//   k_surface<false>  count: points of the cell -> cnt[cell]
//   (the exclusive scan of kernels_mesh.h over cnt: where each cell's points start, and the total)
//   k_surface<true>   emit: the same crossings again, each lane's offset from a workgroup scan, records written
// A cell leaves after ONE directory probe when its block is absent, and the emit pass leaves before any probe when the
// cell counted nothing or starts at or beyond the capacity: both passes cost the box's empty space a launch slot.
// (A work list of the allocated blocks that meet the box would save those slots but has to be brought into the
// header's order first -- a sort by position, or a scan of the cell grid all the same; the grid needs neither.)
// The block's neighbourhood of tsdf and "observed" is staged in LDS from the centre block and its up to 26
// neighbours (probed by 26 lanes side by side, as k_marching_cubes probes its 8): local -1 .. 9 per axis for the
// emit pass (the gradient of the upper endpoint reads two voxels into the next block and the lower one's one voxel
// into the block below), 0 .. 8 for the count pass.  Rows are kSurfRow = 24 words apart: a half-wave is 4 rows of
// 8 lanes, and 24 y mod 32 = 0, 24, 16, 8 puts the four rows on disjoint banks whatever the offset of the read
// (rows of 11 or 12 words fold the fourth row onto the first: 2-way); planes need no padding, a half-wave stays in
// one.  The observed flags are bytes under the same index (6 words per row: four rows again on disjoint words).
// Probability and colour are read from the pool, for crossings only.  Barriers between the phases exchange LDS only
// (lds_barrier, kernels_carve.h).  The map is only read: no directory entry, pool word, free-list slot or delta bit
// is written.
#pragma once
#include "kernels_mesh.h"
#include "map_read.h"

namespace ratsdf {

constexpr int kSurfRow = 24, kSurfPlane = 11 * kSurfRow, kSurfVolume = 11 * kSurfPlane;

// d_b(w) of the header for the voxel at LDS index w, sb: the stride of axis b
__device__ inline float surface_diff(const float* s_t, const uint8_t* s_obs, int w, int sb) {
  const bool up = s_obs[w + sb] != 0, dn = s_obs[w - sb] != 0;
  const float tu = s_t[w + sb], td = s_t[w - sb], tw = s_t[w];
  return up && dn ? (tu - td) * 0.5f : up ? tu - tw : dn ? tw - td : 0.f;
}
// Position and normal of the crossing on edge (the voxel at LDS index c, axis a) with factor f, as the header writes
// them: r[0 .. 2] pos, r[3 .. 5] normal.  d0: d_b of the owner; vf: its voxel index.  The one place this arithmetic
// lives: k_surface and k_surface_mesh (kernels_surface_mesh.h) write the same bytes.
__device__ inline void surface_pos_normal(const float* s_t, const uint8_t* s_obs, int c, int a, float f,
                                          const float (&d0)[3], const float (&vf)[3], float vs, float (&r)[6]) {
  const int st = a == 0 ? 1 : a == 1 ? kSurfRow : kSurfPlane;
  const float u = 1.f - f;
  const float g0 = d0[0] * u + surface_diff(s_t, s_obs, c + st, 1) * f;
  const float g1 = d0[1] * u + surface_diff(s_t, s_obs, c + st, kSurfRow) * f;
  const float g2 = d0[2] * u + surface_diff(s_t, s_obs, c + st, kSurfPlane) * f;
  const float len = sqrtf(g0 * g0 + g1 * g1 + g2 * g2);
  const bool flat = len == 0.f || !(fabsf(len) < INFINITY);  // 0, infinite or NaN
  r[3] = flat ? 0.f : g0 / len, r[4] = flat ? 0.f : g1 / len, r[5] = flat ? 0.f : g2 / len;
  r[0] = (a == 0 ? vf[0] + f : vf[0]) * vs;
  r[1] = (a == 1 ? vf[1] + f : vf[1]) * vs;
  r[2] = (a == 2 ? vf[2] + f : vf[2]) * vs;
}

// cnt: points per cell (written by the count pass, read by the emit pass); pos / total: the scan's results; out: 2
// uint4 per point (the 32-byte ratsdf_surface_point)
template <bool kEmit>
__global__ __launch_bounds__(512) void k_surface(Table tab, Pool pool, MapBox b, uint32_t min_weight, float min_prob,
                                                 float vs, uint32_t* __restrict__ cnt,
                                                 const uint32_t* __restrict__ pos, const uint32_t* __restrict__ total,
                                                 uint4* __restrict__ out, long long capacity,
                                                 long long* __restrict__ d_count) {
  __shared__ float s_t[kSurfVolume];
  __shared__ uint8_t s_obs[kSurfVolume];
  __shared__ int32_t s_nb[27];  // pool index of block (dx, dy, dz) in {-1, 0, 1}^3 at dx + 1 + 3 (dy + 1) + 9 (dz + 1)
  __shared__ uint32_t s_scan[8];
  const uint32_t g = blockIdx.x;
  const int tid = (int)threadIdx.x;
  uint32_t first = 0u;
  if (kEmit) {
    if (g == 0u && tid == 0) *d_count = (long long)*total;
    first = pos[g];
    if (cnt[g] == 0u || (long long)first >= capacity) return;
  }
  const int bx = b.bx0 + (int)(g % (uint32_t)b.nbx), by = b.by0 + (int)((g / (uint32_t)b.nbx) % (uint32_t)b.nby);
  const int bz = b.bz0 + (int)(g / ((uint32_t)b.nbx * (uint32_t)b.nby));
  if (tid == 0) s_nb[13] = lookup_block(tab, bx, by, bz);  // (the box lies inside the grid: surface_box)
  lds_barrier();
  if (s_nb[13] < 0) {
    if (!kEmit && tid == 0) cnt[g] = 0u;
    return;
  }
  if (tid < 27 && tid != 13) {  // (a neighbour beyond the grid is absent)
    const int x = bx + tid % 3 - 1, y = by + tid / 3 % 3 - 1, z = bz + tid / 9 - 1;
    s_nb[tid] = block_in_grid(x, y, z) ? lookup_block(tab, x, y, z) : -1;
  }
  lds_barrier();

  constexpr int lo = kEmit ? -1 : 0, n = kEmit ? 11 : 9;
  for (int i = tid; i < n * n * n; i += 512) {
    const int px = i % n + lo, py = i / n % n + lo, pz = i / (n * n) + lo;
    const int32_t blk = s_nb[((px + 8) >> 3) + 3 * ((py + 8) >> 3) + 9 * ((pz + 8) >> 3)];
    float t = 0.f;
    uint32_t ob = 0u;
    if (blk >= 0) {
      const size_t p = ((size_t)blk << 9) + (size_t)((px & 7) + 8 * (py & 7) + 64 * (pz & 7));
      const float tv = pool.tsdf[p];
      const uint32_t w = pool.rgbw[p] >> 24;
      if (w >= min_weight && !(w == 1u && __float_as_uint(tv) == 0xBF800000u)) t = tv, ob = 1u;
    }
    const int s = (pz + 1) * kSurfPlane + (py + 1) * kSurfRow + (px + 1);
    s_t[s] = t;
    s_obs[s] = (uint8_t)ob;
  }
  lds_barrier();

  const int x = tid & 7, y = (tid >> 3) & 7, z = tid >> 6;
  const int vx = bx * 8 + x, vy = by * 8 + y, vz = bz * 8 + z;
  const int c = (z + 1) * kSurfPlane + (y + 1) * kSurfRow + (x + 1);
  const bool own = (unsigned)(vx - b.ox) < (unsigned)b.X && (unsigned)(vy - b.oy) < (unsigned)b.Y &&
                   (unsigned)(vz - b.oz) < (unsigned)b.Z && s_obs[c] != 0;
  const float t0 = s_t[c];
  bool cr[3];
  float f[3], prob[3];
  size_t pv[3];  // pool index of the chosen endpoint
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int st = a == 0 ? 1 : a == 1 ? kSurfRow : kSurfPlane, st8 = a == 0 ? 1 : a == 1 ? 8 : 64;
    const int la = a == 0 ? x : a == 1 ? y : z;
    const float t1 = s_t[c + st];
    cr[a] = own && s_obs[c + st] != 0 && ((t0 < 0.f) != (t1 < 0.f));
    f[a] = t0 / (t0 - t1);
    prob[a] = 0.f;
    pv[a] = 0;
    if (cr[a]) {
      const bool up = f[a] >= 0.5f, next = up && la == 7;  // (next: the upper endpoint lies in the next block)
      const int32_t blk = next ? s_nb[13 + (a == 0 ? 1 : a == 1 ? 3 : 9)] : s_nb[13];
      pv[a] = ((size_t)blk << 9) + (size_t)(tid + (next ? -7 * st8 : up ? st8 : 0));
      prob[a] = pool.segm[pv[a]];
      cr[a] = !(prob[a] < min_prob);
    }
  }
  const uint32_t mine = (uint32_t)cr[0] + (uint32_t)cr[1] + (uint32_t)cr[2];
  uint32_t cell = 0u;
  const uint32_t at = block_exclusive_scan(mine, s_scan, &cell);
  if (!kEmit) {
    if (tid == 0) cnt[g] = cell;
    return;
  }
  if (mine == 0u) return;
  const float d0[3] = {surface_diff(s_t, s_obs, c, 1), surface_diff(s_t, s_obs, c, kSurfRow),
                       surface_diff(s_t, s_obs, c, kSurfPlane)};
  const float vf[3] = {(float)vx, (float)vy, (float)vz};
  long long o = (long long)first + (long long)at;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (!cr[a]) continue;
    float r[6];
    surface_pos_normal(s_t, s_obs, c, a, f[a], d0, vf, vs, r);
    if (o < capacity) {
      const uint32_t colour = pool.rgbw[pv[a]];
      out[2 * (size_t)o] = make_uint4(__float_as_uint(r[0]), __float_as_uint(r[1]), __float_as_uint(r[2]),
                                      __float_as_uint(r[3]));
      out[2 * (size_t)o + 1] = make_uint4(__float_as_uint(r[4]), __float_as_uint(r[5]), __float_as_uint(prob[a]), colour);
    }
    ++o;
  }
}

}  // namespace ratsdf
