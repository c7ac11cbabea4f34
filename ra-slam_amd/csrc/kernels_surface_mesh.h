// kernels_surface_mesh.h -- welded triangle mesh of a box of the map (include/ratsdf_surface_mesh.h): the surface
// points of kernels_surface.h as vertices and the marching-cubes triangles over them as indices.  No reference
// counterpart (k_marching_cubes stays the reference's mesh).
//
// The shape of kernels_surface.h: one 512-thread workgroup per cell of the block grid of the voxel range
// [origin, origin + dims] (the vertex owners; up to one block more per axis than the box meets), x fastest, one lane per
// voxel of the block, run twice:
//   k_surface_mesh<false>  count: vertices and triangles of the cell -> cnt_v[cell], cnt_t[cell], and per voxel a
//                          16-bit code (the lane's exclusive vertex offset within the block << 3 | its axis mask) --
//                          only where the cell has a vertex at all: readers test cnt_v first
//   (the exclusive scan of kernels_mesh.h, once over cnt_v and once over cnt_t)
//   k_surface_mesh<true>   emit: the same again; vertex records as k_surface writes them (surface_pos_normal, shared
//                          with it), triangle indices from the codes of this cell and its seven upper neighbours:
//                          index of edge (w, a) = pos_v[cell of w] + offset(w) + popcount(mask(w) & ((1 << a) - 1))
// tsdf and "observed" are staged exactly as k_surface<true> stages them (local -1 .. 9 for the emit pass: the gradients;
// -1 .. 8 for the count pass: the cells below own edges of this block's voxels), same kSurfRow padding.  A byte per
// local cell -1 .. 7, "complete and in the box", follows from eight observed bytes; a lane's edge is a vertex iff it
// crosses and one of the four cells around it carries the flag, and the lane's own cell emits ntri[case] triangles.
// A cell leaves after one directory probe when its block is absent (every vertex and every triangle of a cell needs
// the cell's own voxel observed); the emit pass leaves before any probe when the cell counted nothing or everything
// it would write lies beyond both capacities.  The map is only read.
#pragma once
#include "kernels_surface.h"

namespace ratsdf {

struct SurfaceMeshTables {
  McTables mc;
  uint8_t ntri[256];  // triangles per sign pattern
};
inline SurfaceMeshTables make_surface_mesh_tables() {
  SurfaceMeshTables t;
  t.mc = make_mc_tables();
  for (int c = 0; c < 256; ++c) {
    int n = 0;
    while (n < 5 && t.mc.tri[c][3 * n] >= 0) ++n;
    t.ntri[c] = (uint8_t)n;
  }
  return t;
}

constexpr int kMeshCodes = 729;  // 9^3: the voxels of a block and the first layer of its upper neighbours

// b: the box, its block grid that of the vertex owners, voxels [o, min(o + dims, 32767)] per axis (surface_mesh_box);
// cnt_v / cnt_t: vertices / triangles per cell, code: 512 halfwords per cell (written by the count pass, read by the
// emit pass); pos_v / pos_t / total[2]: the scans' results; out_v: 2 uint4 per vertex, out_t: 3 words per triangle;
// d_counts: the two totals as int64
template <bool kEmit>
__global__ __launch_bounds__(512) void k_surface_mesh(Table tab, Pool pool, MapBox b, uint32_t min_weight, float vs,
                                                      const SurfaceMeshTables* __restrict__ mt,
                                                      uint32_t* __restrict__ cnt_v, uint32_t* __restrict__ cnt_t,
                                                      uint16_t* __restrict__ code, const uint32_t* __restrict__ pos_v,
                                                      const uint32_t* __restrict__ pos_t,
                                                      const uint32_t* __restrict__ total, uint4* __restrict__ out_v,
                                                      long long vcap, int32_t* __restrict__ out_t, long long tcap,
                                                      long long* __restrict__ d_counts) {
  __shared__ float s_t[kSurfVolume];
  __shared__ uint8_t s_obs[kSurfVolume];
  __shared__ uint8_t s_cell[kSurfVolume];  // cell (x, y, z) in -1 .. 7 under the index of its voxel: complete and in the box
  __shared__ int32_t s_nb[27];  // pool index of block (dx, dy, dz) in {-1, 0, 1}^3 at dx + 1 + 3 (dy + 1) + 9 (dz + 1)
  __shared__ uint32_t s_scan[8];
  __shared__ uint16_t s_code[kEmit ? kMeshCodes + 1 : 2];  // codes of local voxels 0 .. 8 per axis at x + 9 y + 81 z
  __shared__ uint32_t s_base[8];  // first vertex of grid cell (dx, dy, dz) in {0, 1}^3 at dx + 2 dy + 4 dz, ~0u: none
  const uint32_t g = blockIdx.x;
  const int tid = (int)threadIdx.x;
  uint32_t first_v = 0u, first_t = 0u;
  bool want_v = false, want_t = false;  // (emit) something of this cell's lies below the capacity
  if (kEmit) {
    if (g == 0u && tid == 0) d_counts[0] = (long long)total[0], d_counts[1] = (long long)total[1];
    first_v = pos_v[g], first_t = pos_t[g];
    want_v = cnt_v[g] != 0u && (long long)first_v < vcap;
    want_t = cnt_t[g] != 0u && (long long)first_t < tcap;
    if (!want_v && !want_t) return;
  }
  const int gx = (int)(g % (uint32_t)b.nbx), gy = (int)((g / (uint32_t)b.nbx) % (uint32_t)b.nby);
  const int gz = (int)(g / ((uint32_t)b.nbx * (uint32_t)b.nby));
  const int bx = b.bx0 + gx, by = b.by0 + gy, bz = b.bz0 + gz;
  if (tid == 0) s_nb[13] = lookup_block(tab, bx, by, bz);  // (the grid lies inside the int16 range: surface_mesh_box)
  lds_barrier();
  if (s_nb[13] < 0) {
    if (!kEmit && tid == 0) cnt_v[g] = 0u, cnt_t[g] = 0u;
    return;
  }
  if (tid < 27 && tid != 13) {  // (a neighbour beyond the grid of int16 voxels is absent)
    const int x = bx + tid % 3 - 1, y = by + tid / 3 % 3 - 1, z = bz + tid / 9 - 1;
    s_nb[tid] = block_in_grid(x, y, z) ? lookup_block(tab, x, y, z) : -1;
  }
  if (kEmit && tid >= 64 && tid < 72) {  // where the vertices of the upper neighbour cells start
    const int dx = tid & 1, dy = (tid >> 1) & 1, dz = (tid >> 2) & 1;
    uint32_t base = ~0u;
    if (gx + dx < b.nbx && gy + dy < b.nby && gz + dz < b.nbz) {
      const uint32_t gn = g + (uint32_t)dx + (uint32_t)b.nbx * ((uint32_t)dy + (uint32_t)b.nby * (uint32_t)dz);
      if (cnt_v[gn] != 0u) base = pos_v[gn];
    }
    s_base[tid - 64] = base;
  }
  lds_barrier();

  constexpr int lo = -1, n = kEmit ? 11 : 10;
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
  if (kEmit && want_t) {  // (uniform) the codes the triangles' indices are made of
    for (int i = tid; i < kMeshCodes; i += 512) {
      const int wx = i % 9, wy = i / 9 % 9, wz = i / 81;
      const int dx = wx >> 3, dy = wy >> 3, dz = wz >> 3;
      uint16_t cd = 0;
      if (s_base[dx + 2 * dy + 4 * dz] != ~0u) {
        const size_t gn = (size_t)g + (size_t)dx + (size_t)b.nbx * ((size_t)dy + (size_t)b.nby * (size_t)dz);
        cd = code[(gn << 9) + (size_t)((wx & 7) + 8 * (wy & 7) + 64 * (wz & 7))];
      }
      s_code[i] = cd;
    }
  }
  lds_barrier();

  for (int i = tid; i < 729; i += 512) {  // the cells -1 .. 7
    const int cx = i % 9 - 1, cy = i / 9 % 9 - 1, cz = i / 81 - 1;
    const int s = (cz + 1) * kSurfPlane + (cy + 1) * kSurfRow + (cx + 1);
    const bool in = (unsigned)(bx * 8 + cx - b.ox) < (unsigned)b.X && (unsigned)(by * 8 + cy - b.oy) < (unsigned)b.Y &&
                    (unsigned)(bz * 8 + cz - b.oz) < (unsigned)b.Z;
    const uint32_t all = s_obs[s] & s_obs[s + 1] & s_obs[s + kSurfRow] & s_obs[s + kSurfRow + 1] &
                         s_obs[s + kSurfPlane] & s_obs[s + kSurfPlane + 1] & s_obs[s + kSurfPlane + kSurfRow] &
                         s_obs[s + kSurfPlane + kSurfRow + 1];
    s_cell[s] = (uint8_t)(in ? all : 0u);
  }
  lds_barrier();

  const int x = tid & 7, y = (tid >> 3) & 7, z = tid >> 6;
  const int c = (z + 1) * kSurfPlane + (y + 1) * kSurfRow + (x + 1);
  const bool seen = s_obs[c] != 0;
  const float t0 = s_t[c];
  uint32_t mask = 0u;  // bit a: edge (this voxel, a) is a vertex
  float f[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int st = a == 0 ? 1 : a == 1 ? kSurfRow : kSurfPlane;
    const int sb = a == 0 ? kSurfRow : 1, sc = a == 2 ? kSurfRow : kSurfPlane;  // the two other axes
    const float t1 = s_t[c + st];
    const bool cross = seen && s_obs[c + st] != 0 && ((t0 < 0.f) != (t1 < 0.f));
    const uint32_t around = s_cell[c] | s_cell[c - sb] | s_cell[c - sc] | s_cell[c - sb - sc];
    f[a] = t0 / (t0 - t1);
    if (cross && around != 0u) mask |= 1u << a;
  }
  uint32_t pattern = 0u, ntri = 0u;
  if (s_cell[c] != 0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int ci = c + (i == 1 || i == 2 || i == 5 || i == 6 ? 1 : 0) + (i >= 4 ? kSurfRow : 0) +
                     (i == 2 || i == 3 || i == 6 || i == 7 ? kSurfPlane : 0);  // kCorner[i]
      pattern |= (uint32_t)(s_t[ci] < 0.f) << i;
    }
    ntri = mt->ntri[pattern];
  }
  const uint32_t mine = (uint32_t)__popc(mask) | ntri << 16;  // (a cell has at most 1536 vertices and 2560 triangles)
  uint32_t cell = 0u;
  const uint32_t at = block_exclusive_scan(mine, s_scan, &cell);
  const uint32_t at_v = at & 0xFFFFu, at_t = at >> 16;
  if (!kEmit) {
    if (tid == 0) cnt_v[g] = cell & 0xFFFFu, cnt_t[g] = cell >> 16;
    if ((cell & 0xFFFFu) != 0u) code[((size_t)g << 9) + (size_t)tid] = (uint16_t)(at_v << 3 | mask);
    return;
  }

  if (want_v && mask != 0u) {
    const float d0[3] = {surface_diff(s_t, s_obs, c, 1), surface_diff(s_t, s_obs, c, kSurfRow),
                         surface_diff(s_t, s_obs, c, kSurfPlane)};
    const float vf[3] = {(float)(bx * 8 + x), (float)(by * 8 + y), (float)(bz * 8 + z)};
    long long o = (long long)first_v + (long long)at_v;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (!(mask >> a & 1u)) continue;
      if (o < vcap) {  // the record of k_surface (surface_pos_normal), probability and colour of the chosen endpoint
        const int st8 = a == 0 ? 1 : a == 1 ? 8 : 64, la = a == 0 ? x : a == 1 ? y : z;
        const bool up = f[a] >= 0.5f, next = up && la == 7;  // (next: the upper endpoint lies in the next block)
        const int32_t blk = next ? s_nb[13 + (a == 0 ? 1 : a == 1 ? 3 : 9)] : s_nb[13];
        const size_t pv = ((size_t)blk << 9) + (size_t)(tid + (next ? -7 * st8 : up ? st8 : 0));
        float r[6];
        surface_pos_normal(s_t, s_obs, c, a, f[a], d0, vf, vs, r);
        const float prob = pool.segm[pv];
        const uint32_t colour = pool.rgbw[pv];
        out_v[2 * (size_t)o] = make_uint4(__float_as_uint(r[0]), __float_as_uint(r[1]), __float_as_uint(r[2]),
                                          __float_as_uint(r[3]));
        out_v[2 * (size_t)o + 1] = make_uint4(__float_as_uint(r[4]), __float_as_uint(r[5]), __float_as_uint(prob), colour);
      }
      ++o;
    }
  }
  if (want_t && ntri != 0u) {
    const int8_t* cs = mt->mc.tri[pattern];
    long long o = (long long)first_t + (long long)at_t;
    for (uint32_t i = 0; i < ntri; ++i, ++o) {
      if (o >= tcap) break;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int e = cs[3 * i + j];  // (the table's own order winds towards free space)
        const int lc = mt->mc.edge_lower[e], dim = mt->mc.edge_dim[e];
        const int wx = x + kCorner[lc][0], wy = y + kCorner[lc][1], wz = z + kCorner[lc][2];
        const uint32_t cd = s_code[wx + 9 * wy + 81 * wz];
        const uint32_t base = s_base[(wx >> 3) + 2 * (wy >> 3) + 4 * (wz >> 3)];
        out_t[3 * (size_t)o + j] = (int32_t)(base + (cd >> 3) + (uint32_t)__popc(cd & ((1u << dim) - 1u)));
      }
    }
  }
}

}  // namespace ratsdf
