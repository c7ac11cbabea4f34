// kernels_cluster_mesh.h -- clustered mesh of a box of the map (include/ratsdf_cluster_mesh.h): the welded mesh of
// kernels_surface_mesh.h with its vertices merged per lattice-aligned cluster of k x k x k voxels (k = 1 << s, s in
// 1 .. 3) and its triangles re-indexed, the degenerate ones dropped and the duplicates removed.  No reference
// counterpart (the reference simplifies on the host, with Open3D).
//
// The shape of kernels_surface_mesh.h: one 512-thread workgroup per cell of the owners' block grid, x fastest, one lane
// per voxel of the block (lane = x + 8 y + 64 z), run twice with the scan of kernels_mesh.h in between:
//   k_cluster_mesh<false>  count: the 64-bit mask of the block's non-empty clusters -> mask[cell], its popcount ->
//                          cnt_v[cell]; the popcount of the triangle bitmap -> cnt_t[cell]
//   k_cluster_mesh<true>   emit: the cluster records, and the triangles from the rebuilt bitmap
// A cluster lies inside one block (k divides 8), so a block's vertices are its clusters in the order of their local
// index lx + m ly + m^2 lz (m = 8 / k), and a cluster's vertex index is pos_v[cell] + popcount(mask[cell] below it).
//
// Staging: tsdf and "observed" as k_surface_mesh stages them, rows kClusRow = 24 words apart, but 12 rows and planes:
// local -2 .. 9 for the emit pass, -1 .. 8 for the count pass.  A member edge owned at local -1 (its upper endpoint, the
// chosen one, is voxel 0 of this block) takes its gradient from local -2, one voxel further down than k_surface_mesh
// reaches; kSurfPlane holds 11 rows, which is why surface_pos_normal cannot be called on this staging:
// cluster_member_normal restates its normal over surface_diff, which takes its stride as an argument.  A byte per
// cell -1 .. 7, "complete and in the box", as in k_surface_mesh.
//
// The vertex half (a lane is the voxel u): the up to six member edges whose chosen endpoint is u are added to 0.0f in
// the header's order; then the header's tree.  Its x and y levels are lane bits 0 .. s - 1 and 3 .. 3 + s - 1, inside a
// wave (a wave is one z plane): xor exchanges, the value of the lower lane on the left.  The z levels cross waves: the
// first lane of every cluster's plane leaves its twelve sums in LDS and the cluster's first lane adds the k planes as the
// tree's last s levels do.  Probability and colour are the lane's own voxel's (every member's chosen endpoint is u).
//
// The triangle half: every complete cell of local -1 .. 7 in the box (each has a corner in this block) maps the table
// triangles of its case to three clusters, by f of the three edges from the staged tsdf.  A cluster is (block offset
// in {-1, 0, 1}^3, local index); offset z, y, x and the local index, packed in that order, compare as the vertex indices
// do.  A triangle with two equal clusters is dropped, the others are rotated so that the smallest comes first, and those
// whose first cluster lies in this block set bit (first local * 27 + code2) * 27 + code3 of an LDS bitmap (64 * 729
// bits) with an LDS atomic OR: the bitmap removes the duplicates and its bit order is the header's triangle order.  The
// emit pass rebuilds it, ranks its bits with a workgroup scan and turns (block offset, local index) into an index with
// the masks and vertex starts of the 27 neighbouring cells.
// A cell leaves after one directory probe when its block is absent (every member's chosen endpoint and every kept
// triangle's first cluster is an observed voxel of the block); the emit pass leaves before any probe when the cell
// counted nothing or everything it would write lies beyond both capacities.  The map is only read.
#pragma once
#include "kernels_surface_mesh.h"

namespace ratsdf {

constexpr int kClusRow = kSurfRow, kClusPlane = 12 * kClusRow, kClusVolume = 12 * kClusPlane;  // local -2 .. 9
constexpr int kClusBits = 64 * 729, kClusBitWords = (kClusBits + 31) / 32;                     // 1458 words
constexpr int kClusSums = 12;  // rel[3], normal[3], prob | members, r, g, b, weight

__device__ inline int clus_at(int x, int y, int z) { return (z + 2) * kClusPlane + (y + 2) * kClusRow + (x + 2); }

// unit normal of the crossing on edge (the voxel at LDS index w, axis stride st) with factor f: the lines of
// surface_pos_normal (kernels_surface.h) on this kernel's strides; the same bytes as the welded mesh's vertex
__device__ inline void cluster_member_normal(const float* s_t, const uint8_t* s_obs, int w, int st, float f,
                                             float (&r)[3]) {
  const float u = 1.f - f;
  const float g0 = surface_diff(s_t, s_obs, w, 1) * u + surface_diff(s_t, s_obs, w + st, 1) * f;
  const float g1 = surface_diff(s_t, s_obs, w, kClusRow) * u + surface_diff(s_t, s_obs, w + st, kClusRow) * f;
  const float g2 = surface_diff(s_t, s_obs, w, kClusPlane) * u + surface_diff(s_t, s_obs, w + st, kClusPlane) * f;
  const float len = sqrtf(g0 * g0 + g1 * g1 + g2 * g2);
  const bool flat = len == 0.f || !(fabsf(len) < INFINITY);  // 0, infinite or NaN
  r[0] = flat ? 0.f : g0 / len, r[1] = flat ? 0.f : g1 / len, r[2] = flat ? 0.f : g2 / len;
}

// The cluster of the local voxel (ux, uy, uz) in -1 .. 8, packed so that two of them compare as their vertex indices
// do: (block offset z, y, x in 0 .. 2 as one number 0 .. 26) << 18 | local index << 12 | the cluster's coordinates
// relative to the block's first cluster, each + 1 (0 .. m + 1), x | y << 4 | z << 8
__device__ inline uint32_t cluster_pack(int ux, int uy, int uz, int s, int m) {
  const int qx = ((ux + 8) >> s) - m, qy = ((uy + 8) >> s) - m, qz = ((uz + 8) >> s) - m;  // -1 .. m
  const int ox = qx < 0 ? -1 : qx >= m ? 1 : 0, oy = qy < 0 ? -1 : qy >= m ? 1 : 0, oz = qz < 0 ? -1 : qz >= m ? 1 : 0;
  const int local = (qx - ox * m) + m * ((qy - oy * m) + m * (qz - oz * m));
  return (uint32_t)((oz + 1) * 9 + (oy + 1) * 3 + (ox + 1)) << 18 | (uint32_t)local << 12 |
         (uint32_t)((qx + 1) | (qy + 1) << 4 | (qz + 1) << 8);
}
__device__ inline int cluster_code(uint32_t p, uint32_t first) {  // code(q_p - q_first) of the header
  const int d0 = (int)(p & 15u) - (int)(first & 15u), d1 = (int)(p >> 4 & 15u) - (int)(first >> 4 & 15u);
  const int d2 = (int)(p >> 8 & 15u) - (int)(first >> 8 & 15u);
  return (d0 + 1) + 3 * (d1 + 1) + 9 * (d2 + 1);
}

// b: the box, its block grid that of surface_mesh_box; s: log2 of the factor; cnt_v / cnt_t: vertices / triangles per
// cell, mask: the non-empty clusters per cell (written by the count pass, read by the emit pass); pos_v / pos_t /
// total[2]: the scans' results; out_v: 2 uint4 per vertex, out_t: 3 words per triangle; d_counts: the totals as int64
template <bool kEmit>
__global__ __launch_bounds__(512) void k_cluster_mesh(Table tab, Pool pool, MapBox b, uint32_t min_weight, float vs,
                                                      int s, const SurfaceMeshTables* __restrict__ mt,
                                                      uint32_t* __restrict__ cnt_v, uint32_t* __restrict__ cnt_t,
                                                      unsigned long long* __restrict__ mask,
                                                      const uint32_t* __restrict__ pos_v,
                                                      const uint32_t* __restrict__ pos_t,
                                                      const uint32_t* __restrict__ total, uint4* __restrict__ out_v,
                                                      long long vcap, int32_t* __restrict__ out_t, long long tcap,
                                                      long long* __restrict__ d_counts) {
  __shared__ float s_t[kClusVolume];
  __shared__ uint8_t s_obs[kClusVolume];
  __shared__ uint8_t s_cell[kClusVolume];  // cell (x, y, z) in -1 .. 7 under the index of its voxel: complete and in the box
  __shared__ uint32_t s_bits[kClusBitWords];
  __shared__ uint32_t s_red[kEmit ? kClusSums * 128 : 1];  // the sums of a cluster's plane: [quantity][z][plane's cluster]
  __shared__ unsigned long long s_mask[27];  // (count) [13]: this block's; (emit) the 27 neighbouring cells'
  __shared__ uint32_t s_start[27];           // (emit) where their vertices start
  __shared__ int32_t s_nb[27];  // pool index of block (dx, dy, dz) in {-1, 0, 1}^3 at dx + 1 + 3 (dy + 1) + 9 (dz + 1)
  __shared__ uint32_t s_scan[8];
  const uint32_t g = blockIdx.x;
  const int tid = (int)threadIdx.x;
  const int k = 1 << s, m = 8 >> s;
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
    if (!kEmit && tid == 0) cnt_v[g] = 0u, cnt_t[g] = 0u, mask[g] = 0ull;
    return;
  }
  if (tid < 27) {
    const int dx = tid % 3 - 1, dy = tid / 3 % 3 - 1, dz = tid / 9 - 1;
    if (tid != 13)  // (a neighbour beyond the grid of int16 voxels is absent)
      s_nb[tid] = block_in_grid(bx + dx, by + dy, bz + dz) ? lookup_block(tab, bx + dx, by + dy, bz + dz) : -1;
    unsigned long long nm = 0ull;
    uint32_t ns = 0u;
    if (kEmit && (unsigned)(gx + dx) < (unsigned)b.nbx && (unsigned)(gy + dy) < (unsigned)b.nby &&
        (unsigned)(gz + dz) < (unsigned)b.nbz) {  // (no cluster of a triangle lies beyond the grid)
      const size_t gn = (size_t)((long long)g + dx + (long long)b.nbx * (dy + (long long)b.nby * dz));
      nm = mask[gn], ns = pos_v[gn];
    }
    s_mask[tid] = nm, s_start[tid] = ns;
  }
  for (int i = tid; i < kClusBitWords; i += 512) s_bits[i] = 0u;
  lds_barrier();

  constexpr int lo = kEmit ? -2 : -1, n = kEmit ? 12 : 10;
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
    const int si = clus_at(px, py, pz);
    s_t[si] = t;
    s_obs[si] = (uint8_t)ob;
  }
  lds_barrier();

  for (int i = tid; i < 729; i += 512) {  // the cells -1 .. 7
    const int cx = i % 9 - 1, cy = i / 9 % 9 - 1, cz = i / 81 - 1;
    const int c = clus_at(cx, cy, cz);
    const bool in = (unsigned)(bx * 8 + cx - b.ox) < (unsigned)b.X && (unsigned)(by * 8 + cy - b.oy) < (unsigned)b.Y &&
                    (unsigned)(bz * 8 + cz - b.oz) < (unsigned)b.Z;
    const uint32_t all = s_obs[c] & s_obs[c + 1] & s_obs[c + kClusRow] & s_obs[c + kClusRow + 1] &
                         s_obs[c + kClusPlane] & s_obs[c + kClusPlane + 1] & s_obs[c + kClusPlane + kClusRow] &
                         s_obs[c + kClusPlane + kClusRow + 1];
    s_cell[c] = (uint8_t)(in ? all : 0u);
  }
  lds_barrier();

  // ---- the vertex half: the members of this lane's voxel ---------------------------------------------------------
  const int x = tid & 7, y = (tid >> 3) & 7, z = tid >> 6;
  const int c = clus_at(x, y, z);
  const int cl = (x >> s) + m * ((y >> s) + m * (z >> s));  // the cluster's local index
  if (!kEmit || want_v) {                                     // (uniform)
    float sum[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};      // rel[3], normal[3], prob
    uint32_t members = 0u;
    const bool seen = s_obs[c] != 0;
    const float tu = s_t[c];
    float prob = 0.f;
    if (kEmit && seen) prob = pool.segm[((size_t)s_nb[13] << 9) + (size_t)tid];
    const float rel[3] = {(float)(x & (k - 1)), (float)(y & (k - 1)), (float)(z & (k - 1))};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const int st = a == 0 ? 1 : a == 1 ? kClusRow : kClusPlane;
      const int sb = a == 0 ? kClusRow : 1, sc = a == 2 ? kClusRow : kClusPlane;  // the two other axes
#pragma unroll
      for (int own = 0; own < 2; ++own) {  // edge (u - e_a, a), then edge (u, a)
        const int w = own ? c : c - st;
        const float t0 = own ? tu : s_t[w], t1 = own ? s_t[c + st] : tu;
        const bool cross = seen && s_obs[own ? c + st : w] != 0 && ((t0 < 0.f) != (t1 < 0.f));
        const uint32_t around = s_cell[w] | s_cell[w - sb] | s_cell[w - sc] | s_cell[w - sb - sc];
        const float f = t0 / (t0 - t1);
        const bool up = f >= 0.5f;  // the chosen endpoint is the upper one
        if (!(cross && around != 0u && up == (own == 0))) continue;
        ++members;
        if (kEmit) {
          float nrm[3];
          cluster_member_normal(s_t, s_obs, w, st, f, nrm);
          const float lower = own ? rel[a] : rel[a] - 1.f;  // the owner relative to the cluster's base (may be -1)
          sum[0] = sum[0] + (a == 0 ? lower + f : rel[0]);
          sum[1] = sum[1] + (a == 1 ? lower + f : rel[1]);
          sum[2] = sum[2] + (a == 2 ? lower + f : rel[2]);
          sum[3] = sum[3] + nrm[0], sum[4] = sum[4] + nrm[1], sum[5] = sum[5] + nrm[2];
          sum[6] = sum[6] + prob;
        }
      }
    }
    if (!kEmit) {
      if (members != 0u) atomicOr(&s_mask[13], 1ull << cl);  // (zero since the probes; stored after the next barrier)
    } else {
      uint32_t isum[5] = {members, 0u, 0u, 0u, 0u};
      if (members != 0u) {
        const uint32_t colour = pool.rgbw[((size_t)s_nb[13] << 9) + (size_t)tid];
        isum[1] = members * (colour & 255u), isum[2] = members * (colour >> 8 & 255u);
        isum[3] = members * (colour >> 16 & 255u), isum[4] = members * (colour >> 24);
      }
      // the tree's x and y levels: lane bits 0 .. s - 1 and 3 .. 3 + s - 1, the lower lane's value on the left
      for (int ax = 0; ax < 2; ++ax)
        for (int l = 0; l < s; ++l) {
          const int bit = 1 << (3 * ax + l);
          const bool upper = (tid & bit) != 0;
#pragma unroll
          for (int q = 0; q < 7; ++q) {
            const float o = __shfl_xor(sum[q], bit);
            sum[q] = upper ? o + sum[q] : sum[q] + o;
          }
#pragma unroll
          for (int q = 0; q < 5; ++q) isum[q] += __shfl_xor(isum[q], bit);
        }
      // the z levels: the planes of a cluster through LDS
      const bool plane_head = ((x | y) & (k - 1)) == 0;
      const int slot = z * 16 + (x >> s) + m * (y >> s);
      if (plane_head) {
#pragma unroll
        for (int q = 0; q < 7; ++q) s_red[q * 128 + slot] = __float_as_uint(sum[q]);
#pragma unroll
        for (int q = 0; q < 5; ++q) s_red[(7 + q) * 128 + slot] = isum[q];
      }
      lds_barrier();
      if (plane_head && (z & (k - 1)) == 0) {
#pragma unroll
        for (int q = 0; q < 7; ++q) {
          float part[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) part[j] = j < k ? __uint_as_float(s_red[q * 128 + slot + 16 * j]) : 0.f;
#pragma unroll
          for (int step = 1; step < 8; step <<= 1)
            if (step < k) {
#pragma unroll
              for (int j = 0; j < 8; j += 2 * step)
                if (j < k) part[j] = part[j] + part[j + step];
            }
          sum[q] = part[0];
        }
#pragma unroll
        for (int q = 0; q < 5; ++q) {
          uint32_t v = 0u;
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (j < k) v += s_red[(7 + q) * 128 + slot + 16 * j];
          isum[q] = v;
        }
        const uint32_t nmem = isum[0];
        const long long o = (long long)first_v + (long long)__popcll(s_mask[13] & ((1ull << cl) - 1ull));
        if (nmem != 0u && o < vcap) {
          const float fn = (float)nmem;
          const float p0 = ((float)(bx * 8 + x) + sum[0] / fn) * vs, p1 = ((float)(by * 8 + y) + sum[1] / fn) * vs;
          const float p2 = ((float)(bz * 8 + z) + sum[2] / fn) * vs;
          const float len = sqrtf(sum[3] * sum[3] + sum[4] * sum[4] + sum[5] * sum[5]);
          const bool flat = len == 0.f || !(fabsf(len) < INFINITY);  // 0, infinite or NaN
          const float n0 = flat ? 0.f : sum[3] / len, n1 = flat ? 0.f : sum[4] / len, n2 = flat ? 0.f : sum[5] / len;
          const uint32_t colour = (2u * isum[1] + nmem) / (2u * nmem) | (2u * isum[2] + nmem) / (2u * nmem) << 8 |
                                  (2u * isum[3] + nmem) / (2u * nmem) << 16 | (2u * isum[4] + nmem) / (2u * nmem) << 24;
          out_v[2 * (size_t)o] = make_uint4(__float_as_uint(p0), __float_as_uint(p1), __float_as_uint(p2),
                                            __float_as_uint(n0));
          out_v[2 * (size_t)o + 1] = make_uint4(__float_as_uint(n1), __float_as_uint(n2),
                                                __float_as_uint(sum[6] / fn), colour);
        }
      }
    }
  }
  if (kEmit && !want_t) return;  // (uniform)

  // ---- the triangle half: the cells -1 .. 7 into the bitmap ------------------------------------------------------
  for (int i = tid; i < 729; i += 512) {
    const int cx = i % 9 - 1, cy = i / 9 % 9 - 1, cz = i / 81 - 1;
    const int cc = clus_at(cx, cy, cz);
    if (s_cell[cc] == 0) continue;
    uint32_t pattern = 0u;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int ci = cc + (j == 1 || j == 2 || j == 5 || j == 6 ? 1 : 0) + (j >= 4 ? kClusRow : 0) +
                     (j == 2 || j == 3 || j == 6 || j == 7 ? kClusPlane : 0);  // kCorner[j]
      pattern |= (uint32_t)(s_t[ci] < 0.f) << j;
    }
    const int8_t* cs = mt->mc.tri[pattern];
    const uint32_t ntri = mt->ntri[pattern];
    for (uint32_t ti = 0; ti < ntri; ++ti) {
      uint32_t p[3];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int e = cs[3 * ti + j];
        const int lc = mt->mc.edge_lower[e], dim = mt->mc.edge_dim[e];
        const int wx = cx + kCorner[lc][0], wy = cy + kCorner[lc][1], wz = cz + kCorner[lc][2];
        const int w = clus_at(wx, wy, wz);
        const float t0 = s_t[w], t1 = s_t[w + (dim == 0 ? 1 : dim == 1 ? kClusRow : kClusPlane)];
        const int up = t0 / (t0 - t1) >= 0.5f ? 1 : 0;
        p[j] = cluster_pack(wx + (dim == 0 ? up : 0), wy + (dim == 1 ? up : 0), wz + (dim == 2 ? up : 0), s, m);
      }
      if (p[0] == p[1] || p[1] == p[2] || p[0] == p[2]) continue;  // two vertices in one cluster: dropped
      uint32_t a0 = p[0], a1 = p[1], a2 = p[2];                    // rotated, the winding kept
      if (p[1] < p[0] && p[1] < p[2]) a0 = p[1], a1 = p[2], a2 = p[0];
      if (p[2] < p[0] && p[2] < p[1]) a0 = p[2], a1 = p[0], a2 = p[1];
      if (a0 >> 18 != 13u) continue;  // its first cluster lies in another block: that block's triangle
      const uint32_t bit = ((a0 >> 12 & 63u) * 27u + (uint32_t)cluster_code(a1, a0)) * 27u +
                           (uint32_t)cluster_code(a2, a0);
      atomicOr(&s_bits[bit >> 5], 1u << (bit & 31u));
    }
  }
  lds_barrier();

  // three words of the bitmap per lane, in order
  uint32_t word[3], mine = 0u;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int wi = 3 * tid + j;
    word[j] = wi < kClusBitWords ? s_bits[wi] : 0u;
    mine += (uint32_t)__popc(word[j]);
  }
  uint32_t cell = 0u;
  const uint32_t at = block_exclusive_scan(mine, s_scan, &cell);
  if (!kEmit) {
    if (tid == 0) {
      const unsigned long long mk = s_mask[13];
      mask[g] = mk, cnt_v[g] = (uint32_t)__popcll(mk), cnt_t[g] = cell;
    }
    return;
  }
  long long o = (long long)first_t + (long long)at;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    uint32_t left = word[j];
    while (left != 0u && o < tcap) {
      const uint32_t bit = (uint32_t)(3 * tid + j) * 32u + (uint32_t)(__ffs((int)left) - 1);
      left &= left - 1u;
      const uint32_t fl = bit / 729u, code2 = bit / 27u % 27u, code3 = bit % 27u;
      const int lx = (int)fl % m, ly = (int)fl / m % m, lz = (int)fl / (m * m);
      int32_t idx[3];
      idx[0] = (int32_t)(first_v + (uint32_t)__popcll(s_mask[13] & ((1ull << fl) - 1ull)));
#pragma unroll
      for (int v = 1; v < 3; ++v) {
        const int code = (int)(v == 1 ? code2 : code3);
        const int qx = lx + code % 3 - 1, qy = ly + code / 3 % 3 - 1, qz = lz + code / 9 - 1;  // -1 .. m
        const int ox = qx < 0 ? -1 : qx >= m ? 1 : 0, oy = qy < 0 ? -1 : qy >= m ? 1 : 0,
                  oz = qz < 0 ? -1 : qz >= m ? 1 : 0;
        const int nb = (ox + 1) + 3 * (oy + 1) + 9 * (oz + 1);
        const int local = (qx - ox * m) + m * ((qy - oy * m) + m * (qz - oz * m));
        idx[v] = (int32_t)(s_start[nb] + (uint32_t)__popcll(s_mask[nb] & ((1ull << local) - 1ull)));
      }
      out_t[3 * (size_t)o] = idx[0], out_t[3 * (size_t)o + 1] = idx[1], out_t[3 * (size_t)o + 2] = idx[2];
      ++o;
    }
  }
}

}  // namespace ratsdf
