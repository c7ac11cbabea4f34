// kernels_regions.h -- connected regions of a box of the map (include/ratsdf_regions.h): a label per voxel (the
// smallest box index of its region) and a table of the regions.  No reference counterpart.
//
// Union-find with parents that only point DOWN (a parent's box index is never above its child's), so the root of a
// region is its smallest index -- the contract's label -- and every chase is bounded by the index it starts at.
// Every phase is a launch of its own on the engine's stream; no workgroup waits for another inside a kernel:
//   k_regions_seed      one workgroup per map block the box meets (as k_esdf_seed): state | member bit per voxel
//   k_regions_local     one workgroup per 32 x 8 x 4 tile of the box (x contiguous): the tile's components resolved in
//                       LDS, each member's label written as the box index of its tile-local root
//   k_regions_merge     each member on the upper x / y / z face of its tile with a member neighbour in the next tile
//                       unites the two trees in global memory (atomicMin hooks, see region_unite)
//   k_regions_flatten   every member's label chased to its root; the root flags for the scan
//   (the exclusive scan of kernels_mesh.h over the root flags: each root's rank = its row of the table, ascending)
//   k_regions_init / k_regions_accumulate / k_regions_finish
//                       the table: integer atomics into record rank[label], in the caller's buffer (below)
// All arithmetic that reaches the result is integer min / max / add: nothing depends on arrival order.
// The map is only read: no directory entry, pool word, free-list slot or delta bit is written.
#pragma once
#include "kernels_esdf.h"
#include "map_read.h"

namespace ratsdf {

constexpr uint32_t kRegionMember = 4u;  // the member bit of a seed byte, above the two bits of the state
constexpr int kRegTX = 32, kRegTY = 8, kRegTZ = 4, kRegTile = kRegTX * kRegTY * kRegTZ;  // voxels of a tile

// seed bytes of the box's voxels that lie in one map block (blockIdx.x: the block, x fastest): k_esdf_seed's state,
// and the member bit of the header (the probability is read for observed voxels only: an UNKNOWN voxel's is 0)
__global__ __launch_bounds__(256) void k_regions_seed(Table tab, Pool pool, MapBox b, float occupied_below,
                                                      float min_prob, uint32_t states, uint8_t* __restrict__ st) {
  __shared__ int32_t s_blk;
  const uint32_t g = blockIdx.x;
  const int bx = b.bx0 + (int)(g % (uint32_t)b.nbx), by = b.by0 + (int)((g / (uint32_t)b.nbx) % (uint32_t)b.nby);
  const int bz = b.bz0 + (int)(g / ((uint32_t)b.nbx * (uint32_t)b.nby));
  if (threadIdx.x == 0) s_blk = lookup_block(tab, bx, by, bz);  // (the box lies inside the grid: esdf_box)
  __syncthreads();
  const int32_t blk = s_blk;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int v = (int)threadIdx.x + 256 * h;  // voxel x + 8y + 64z of the block
    const int x = bx * 8 + (v & 7) - b.ox, y = by * 8 + ((v >> 3) & 7) - b.oy, z = bz * 8 + (v >> 6) - b.oz;
    uint32_t s = kEsdfUnknown;
    float p = 0.f;
    if (blk >= 0) {
      const size_t at = ((size_t)blk << 9) + (size_t)v;
      const float t = pool.tsdf[at];
      const uint32_t w = pool.rgbw[at] >> 24;
      s = w == 0u ? kEsdfUnknown : (t <= occupied_below ? kEsdfOccupied : kEsdfFree);
      if (s != kEsdfUnknown) p = pool.segm[at];
    }
    const bool member = ((states >> s) & 1u) && !(p < min_prob);
    if ((unsigned)x < (unsigned)b.X && (unsigned)y < (unsigned)b.Y && (unsigned)z < (unsigned)b.Z)
      st[(size_t)x + (size_t)b.X * ((size_t)y + (size_t)b.Y * (size_t)z)] = (uint8_t)(s | (member ? kRegionMember : 0u));
  }
}

// The root of x's tree.  Parents only point down, so x falls every step: at most x steps, whatever is read.
template <int kScope>
__device__ inline int32_t region_find(int32_t* L, int32_t x) {
  for (;;) {
    const int32_t p = __hip_atomic_load(L + x, __ATOMIC_RELAXED, kScope);
    if (p == x) return x;
    x = p;
  }
}
// Unite the trees of a and b: the larger root is hooked under the smaller with an atomic min, and when the min finds
// that the "root" had a parent already, the work goes on from that parent (the value the atomic returned).
//
// Why a stale read is harmless (kScope agent: parents are read with relaxed loads that another XCD's hook may not
// have reached yet).  A word L[x] only ever falls, and every value it ever held was put there by a union of two
// voxels of x's region: a stale parent is an older, larger ancestor-to-be of the same region, never a voxel of
// another.  So a chase from a stale value ends at some voxel r of the right region that may no longer be a root; the
// atomic min on L[r] is what decides, at the memory itself: it returns r only if r still was a root (and then the
// hook is made), otherwise the parent r really has, and the loop takes that instead.  When the min replaces a parent
// `old` by the smaller b, the link r - old it overwrote is re-made by the same loop, which goes on to unite old and
// b.  A stale read therefore costs a retry and never a wrong or a lost union.
// The loop ends: a step either returns or replaces a by a smaller value with b unchanged or smaller (roots of
// values that only fall), so a + b falls every step.
template <int kScope>
__device__ inline void region_unite(int32_t* L, int32_t a, int32_t b) {
  for (;;) {
    a = region_find<kScope>(L, a);
    b = region_find<kScope>(L, b);
    if (a == b) return;
    if (a < b) {
      const int32_t t = a;
      a = b, b = t;
    }
    const int32_t old = __hip_atomic_fetch_min(L + a, b, __ATOMIC_RELAXED, kScope);
    if (old == a) return;  // a was a root: hooked
    a = old;
  }
}

// The components of one tile, in LDS.  Tile t: x fastest; local index l = lx + 32 (ly + 8 lz), which orders the tile's
// voxels as the box index does, so the tile-local root is the component's smallest box index.  Thread: the column
// (lx, ly), its four voxels lz = 0 .. 3.  L[i]: the box index of voxel i's tile-local root, -1 for a non-member.
__global__ __launch_bounds__(256) void k_regions_local(const uint8_t* __restrict__ st, int X, int Y, int Z, int ntx,
                                                       int nty, int32_t* __restrict__ L) {
  __shared__ int32_t s_par[kRegTile];
  __shared__ uint8_t s_mem[kRegTile];
  const int tid = (int)threadIdx.x, lx = tid & (kRegTX - 1), ly = tid >> 5;
  const uint32_t t = blockIdx.x;
  const int x0 = (int)(t % (uint32_t)ntx) * kRegTX, y0 = (int)((t / (uint32_t)ntx) % (uint32_t)nty) * kRegTY;
  const int z0 = (int)(t / ((uint32_t)ntx * (uint32_t)nty)) * kRegTZ;
  const int x = x0 + lx, y = y0 + ly;
  const bool in_xy = x < X && y < Y;
#pragma unroll
  for (int k = 0; k < kRegTZ; ++k) {
    const int l = tid + 256 * k, z = z0 + k;
    const bool in = in_xy && z < Z;
    s_mem[l] = in && (st[(size_t)x + (size_t)X * ((size_t)y + (size_t)Y * (size_t)z)] & kRegionMember);
    s_par[l] = l;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kRegTZ; ++k) {
    const int l = tid + 256 * k;
    if (!s_mem[l]) continue;
    if (lx + 1 < kRegTX && s_mem[l + 1]) region_unite<__HIP_MEMORY_SCOPE_WORKGROUP>(s_par, l, l + 1);
    if (ly + 1 < kRegTY && s_mem[l + kRegTX]) region_unite<__HIP_MEMORY_SCOPE_WORKGROUP>(s_par, l, l + kRegTX);
    if (k + 1 < kRegTZ && s_mem[l + 256]) region_unite<__HIP_MEMORY_SCOPE_WORKGROUP>(s_par, l, l + 256);
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kRegTZ; ++k) {
    const int l = tid + 256 * k, z = z0 + k;
    if (!(in_xy && z < Z)) continue;
    int32_t v = -1;
    if (s_mem[l]) {
      const int r = region_find<__HIP_MEMORY_SCOPE_WORKGROUP>(s_par, l);
      v = (x0 + (r & (kRegTX - 1))) + X * ((y0 + ((r >> 5) & (kRegTY - 1))) + Y * (z0 + (r >> 8)));
    }
    L[(size_t)x + (size_t)X * ((size_t)y + (size_t)Y * (size_t)z)] = v;
  }
}

// The unions across tile faces: one thread per voxel of the box; a member on the upper x / y / z face of its tile
// whose neighbour in the next tile is a member unites the two (region_unite, agent scope).
// One union per run: if the pair one step back along the face (s voxels back, in the same two tiles) are members
// that carry the labels of i and of j, that pair's thread unites the same two trees -- or leaves it to the pair
// before it, down to the first of the run, which has nobody to leave it to.  Equal labels mean one tree when they are
// read, and trees only grow together, so the test may be made at any time.  (A box that is one region has 416 such
// pairs per tile and 16 runs: measured on 512 x 384 x 256, the launch fell from 1.77 to 0.52 ms.)
__device__ inline void region_face(const uint8_t* __restrict__ st, int32_t* L, uint32_t i, uint32_t j, bool has_prev,
                                   uint32_t s) {
  if (!(st[j] & kRegionMember)) return;
  if (has_prev && (st[i - s] & kRegionMember) && (st[j - s] & kRegionMember) &&
      __hip_atomic_load(L + (i - s), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ==
          __hip_atomic_load(L + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) &&
      __hip_atomic_load(L + (j - s), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ==
          __hip_atomic_load(L + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
    return;
  region_unite<__HIP_MEMORY_SCOPE_AGENT>(L, (int32_t)i, (int32_t)j);
}
__global__ __launch_bounds__(256) void k_regions_merge(const uint8_t* __restrict__ st, int X, int Y, int Z, uint32_t n,
                                                       int32_t* L) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n || !(st[i] & kRegionMember)) return;
  const uint32_t XY = (uint32_t)X * (uint32_t)Y;
  const int x = (int)(i % (uint32_t)X), y = (int)(i / (uint32_t)X % (uint32_t)Y), z = (int)(i / XY);
  const bool prev_x = (x & (kRegTX - 1)) != 0, prev_y = (y & (kRegTY - 1)) != 0;
  if ((x & (kRegTX - 1)) == kRegTX - 1 && x + 1 < X) region_face(st, L, i, i + 1u, prev_y, (uint32_t)X);
  if ((y & (kRegTY - 1)) == kRegTY - 1 && y + 1 < Y) region_face(st, L, i, i + (uint32_t)X, prev_x, 1u);
  if ((z & (kRegTZ - 1)) == kRegTZ - 1 && z + 1 < Z) region_face(st, L, i, i + XY, prev_x, 1u);
}

// Every member's label becomes its root, in place (a word is overwritten by its own voxel's thread only, with its
// root: whoever reads it meanwhile finds the old parent or the root, both on the way to the same root; a root's word
// is never written).  labels (may be null): a copy for the caller, -1 for non-members.  is_root: the flags the scan
// turns into ranks.
__global__ __launch_bounds__(256) void k_regions_flatten(int32_t* L, uint32_t n, int32_t* __restrict__ labels,
                                                         uint32_t* __restrict__ is_root) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const int32_t p = __hip_atomic_load(L + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  int32_t r = p;
  if (p >= 0) {
    r = region_find<__HIP_MEMORY_SCOPE_AGENT>(L, p);
    if (r != p) __hip_atomic_store(L + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (labels) labels[i] = r;
  is_root[i] = r == (int32_t)i ? 1u : 0u;
}

// ---- the table ----
// The first min(total, capacity) records are accumulated where they are delivered, as eight int32 words
//   root | voxels | frontier | lo x | lo y | hi x | hi y | hi z        (bounds relative to the box's origin)
// which k_regions_finish turns into ratsdf_region in place.  lo z needs no word: the root is the region's smallest
// index, so it lies in its lowest plane.  faces follow from the bounds.
constexpr int kRegRoot = 0, kRegVoxels = 1, kRegFrontier = 2, kRegLoX = 3, kRegLoY = 4, kRegHiX = 5, kRegHiY = 6,
              kRegHiZ = 7;

// the total for the caller, and the neutral element of every record that will be written
__global__ __launch_bounds__(256) void k_regions_init(uint4* __restrict__ rec, const uint32_t* __restrict__ total,
                                                      long long capacity, long long* __restrict__ d_count) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x, tot = *total;
  if (r == 0u) *d_count = (long long)tot;
  if (r >= tot || (long long)r >= capacity) return;
  rec[2 * (size_t)r] = make_uint4(0u, 0u, 0u, 0x7FFFFFFFu);
  rec[2 * (size_t)r + 1] = make_uint4(0x7FFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
}

__device__ inline int wave_all_min(int v) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) v = min(v, __shfl_xor(v, d, 64));
  return v;
}
__device__ inline int wave_all_max(int v) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) v = max(v, __shfl_xor(v, d, 64));
  return v;
}
__device__ inline int wave_all_sum(int v) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// what some voxels of one region add to record r; voxels == 0: nothing
struct RegionPart {
  uint32_t r;
  int voxels, frontier, x0, y0, x1, y1, z1;
};
__device__ inline RegionPart region_part_none() { return {0u, 0, 0, 0x7FFFFFFF, 0x7FFFFFFF, -1, -1, -1}; }
__device__ inline void region_part_add(RegionPart& a, const RegionPart& b) {  // (of the same record)
  a.voxels += b.voxels, a.frontier += b.frontier;
  a.x0 = min(a.x0, b.x0), a.y0 = min(a.y0, b.y0);
  a.x1 = max(a.x1, b.x1), a.y1 = max(a.y1, b.y1), a.z1 = max(a.z1, b.z1);
}
// A bound only moves one way: a value that does not improve on what is there already (or on an older, weaker value a
// stale read shows) needs no atomic.
__device__ inline void region_part_send(int32_t* rec, const RegionPart& p) {
  int32_t* q = rec + 8 * (size_t)p.r;
  atomicAdd(q + kRegVoxels, p.voxels);
  if (p.frontier) atomicAdd(q + kRegFrontier, p.frontier);
  if (__hip_atomic_load(q + kRegLoX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > p.x0) atomicMin(q + kRegLoX, p.x0);
  if (__hip_atomic_load(q + kRegLoY, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > p.y0) atomicMin(q + kRegLoY, p.y0);
  if (__hip_atomic_load(q + kRegHiX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < p.x1) atomicMax(q + kRegHiX, p.x1);
  if (__hip_atomic_load(q + kRegHiY, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < p.y1) atomicMax(q + kRegHiY, p.y1);
  if (__hip_atomic_load(q + kRegHiZ, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < p.z1) atomicMax(q + kRegHiZ, p.z1);
}

// The members whose region's record is delivered add themselves to it.  A box that is one region sends every voxel
// to ONE record, and atomics on one line take their turn at the memory (measured: 45 ns each, 72 ms for a box of 50 M
// voxels when every wave sent its own), so what shares a record is summed on the way: a workgroup takes kRegChunk
// consecutive voxels, a lane sums its 16 while they name one record (it sends what it holds when the record changes),
// a wave whose lanes ended on one record reduces across them, and the four waves' results are joined where they
// agree.  A chunk inside one region sends once.  Integer sums and bounds: the grouping does not reach the result.
constexpr int kRegPerLane = 16, kRegChunk = 256 * kRegPerLane;
__global__ __launch_bounds__(256) void k_regions_accumulate(const uint8_t* __restrict__ st,
                                                            const int32_t* __restrict__ L,
                                                            const uint32_t* __restrict__ rank, int X, int Y, int Z,
                                                            uint32_t n, int32_t* rec, long long capacity) {
  __shared__ RegionPart s_part[4];
  const uint32_t XY = (uint32_t)X * (uint32_t)Y;
  RegionPart acc = region_part_none();
  for (int k = 0; k < kRegPerLane; ++k) {
    const uint32_t i = blockIdx.x * (uint32_t)kRegChunk + (uint32_t)k * 256u + threadIdx.x;
    if (i >= n || !(st[i] & kRegionMember)) continue;
    const int32_t lab = L[i];
    const uint32_t r = rank[lab];
    if ((long long)r >= capacity) continue;
    const int x = (int)(i % (uint32_t)X), y = (int)(i / (uint32_t)X % (uint32_t)Y), z = (int)(i / XY);
    const bool frontier =
        (x > 0 && (st[i - 1u] & 3u) == kEsdfUnknown) || (x + 1 < X && (st[i + 1u] & 3u) == kEsdfUnknown) ||
        (y > 0 && (st[i - (uint32_t)X] & 3u) == kEsdfUnknown) || (y + 1 < Y && (st[i + (uint32_t)X] & 3u) == kEsdfUnknown) ||
        (z > 0 && (st[i - XY] & 3u) == kEsdfUnknown) || (z + 1 < Z && (st[i + XY] & 3u) == kEsdfUnknown);
    if (lab == (int32_t)i) rec[8 * (size_t)r + kRegRoot] = lab;  // (the root: the one writer of this word)
    const RegionPart v = {r, 1, frontier ? 1 : 0, x, y, x, y, z};
    if (acc.voxels && acc.r != r) {
      region_part_send(rec, acc);
      acc = v;
    } else if (acc.voxels) {
      region_part_add(acc, v);
    } else {
      acc = v;
    }
  }
  // across the wave, if the lanes that hold something agree on the record
  const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
  const uint64_t act = __ballot(acc.voxels != 0);
  RegionPart w = region_part_none();
  if (act != 0ull) {  // (the whole wave)
    const uint32_t r0 = (uint32_t)__shfl((int)acc.r, __ffsll((unsigned long long)act) - 1, 64);
    if (__ballot(acc.voxels != 0 && acc.r != r0) == 0ull) {
      w.r = r0;
      w.voxels = wave_all_sum(acc.voxels), w.frontier = wave_all_sum(acc.frontier);
      w.x0 = wave_all_min(acc.x0), w.y0 = wave_all_min(acc.y0);
      w.x1 = wave_all_max(acc.x1), w.y1 = wave_all_max(acc.y1), w.z1 = wave_all_max(acc.z1);
    } else if (acc.voxels) {
      region_part_send(rec, acc);
    }
  }
  if (lane == 0) s_part[wave] = w;
  __syncthreads();
  if (threadIdx.x != 0) return;
  RegionPart run = region_part_none();
  for (int k = 0; k < 4; ++k) {
    const RegionPart p = s_part[k];
    if (!p.voxels) continue;
    if (run.voxels && run.r == p.r) {
      region_part_add(run, p);
    } else {
      if (run.voxels) region_part_send(rec, run);
      run = p;
    }
  }
  if (run.voxels) region_part_send(rec, run);
}

// the accumulated words of record r -> ratsdf_region, in place
__global__ __launch_bounds__(256) void k_regions_finish(uint4* __restrict__ rec, const uint32_t* __restrict__ total,
                                                        long long capacity, MapBox b) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r >= *total || (long long)r >= capacity) return;
  const uint4 a = rec[2 * (size_t)r], c = rec[2 * (size_t)r + 1];
  const int lox = (int)a.w, loy = (int)c.x, hix = (int)c.y, hiy = (int)c.z, hiz = (int)c.w;
  const int loz = (int)(a.x / ((uint32_t)b.X * (uint32_t)b.Y));
  const uint32_t faces = (lox == 0 ? 1u : 0u) | (hix == b.X - 1 ? 2u : 0u) | (loy == 0 ? 4u : 0u) |
                         (hiy == b.Y - 1 ? 8u : 0u) | (loz == 0 ? 16u : 0u) | (hiz == b.Z - 1 ? 32u : 0u);
  auto two = [](int first, int second) { return ((uint32_t)first & 0xFFFFu) | ((uint32_t)second << 16); };  // int16 pair
  rec[2 * (size_t)r] = make_uint4(a.x, a.y, a.z, faces);
  rec[2 * (size_t)r + 1] =
      make_uint4(two(lox + b.ox, loy + b.oy), two(loz + b.oz, hix + b.ox), two(hiy + b.oy, hiz + b.oz), 0u);
}

}  // namespace ratsdf
