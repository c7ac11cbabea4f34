// kernels_cost.h -- the cost-to-go field of a box of the map (include/ratsdf_cost.h): for every traversable voxel the
// least chamfer length (10 / 14 / 17 per face / edge / corner move) of a path through traversable voxels to a goal
// voxel, and the move to take.  No reference counterpart.
//
// A label-correcting shortest-path relaxation, tile by tile.  Every phase is a launch of its own on the engine's
// stream; no workgroup waits for another inside a kernel, and every loop has a bound that follows from its code:
//   (the ESDF of the box, esdf_launch, into the workspace: state bytes and the fp32 field)
//   k_cost_seed      one thread per voxel: the traversable byte; the cost word NONE (or, continuing, what the caller's
//                    buffer holds, made harmless); the dirty flags and their counts
//   k_cost_goals     one thread per goal: a goal inside the box on a traversable voxel gets cost 0; its tile and the
//                    tiles that have it in their halo are dirty
//   k_cost_relax     one launch per round, one workgroup per 32 x 8 x 4 tile (k_regions_local's tiling): a tile that is
//                    not dirty returns at once; a dirty one loads its words and a one-voxel halo (34 x 10 x 6) into
//                    LDS, relaxes there until nothing changes (at most kRegTile sweeps), writes back the words that
//                    fell and marks the neighbouring tiles whose halo they are in dirty for the NEXT round
//   k_cost_summary   the counts and the largest finite cost, summed per wave and workgroup before they are sent
//   k_cost_next      the move of every voxel, from the delivered field
// Why a word read while its owner rewrites it is harmless is argued at k_cost_relax.
// All arithmetic that reaches the result is integer min / add: nothing depends on arrival order.
// The map is only read: no directory entry, pool word, free-list slot or delta bit is written.
#pragma once
#include "kernels_regions.h"

namespace ratsdf {

constexpr uint32_t kCostNone = 0xFFFFFFFFu;               // RATSDF_COST_NONE
constexpr uint32_t kCostMax = ((uint32_t)1 << 27) * 17u;  // no path of a box is longer: 2^27 voxels, 17 a move
constexpr uint32_t kCostAtGoal = 255u, kCostNoStep = 254u;  // RATSDF_COST_AT_GOAL / RATSDF_COST_NO_STEP
constexpr int kCostHX = kRegTX + 2, kCostHY = kRegTY + 2, kCostHZ = kRegTZ + 2;  // a tile with its halo
constexpr int kCostHalo = kCostHX * kCostHY * kCostHZ;

// cost of the voxel a move of weight w leads away from, given the cost c of where it leads (NONE stays NONE: the sum of
// a finite cost never wraps, kCostMax + 17 < 2^32, and NONE + w does)
__device__ inline uint32_t cost_step(uint32_t c, uint32_t w) {
  const uint32_t s = c + w;
  return s < w ? kCostNone : s;
}
__device__ inline uint32_t cost_weight(int dx, int dy, int dz) {
  const int k = (dx != 0) + (dy != 0) + (dz != 0);
  return k == 1 ? 10u : (k == 2 ? 14u : 17u);
}

// a dirty mark for tile t in `flags` (one word per tile, 0 or 1) and its count: the count is the number of set flags
// whenever no kernel is running
__device__ inline void cost_mark(uint32_t* flags, uint32_t* count, uint32_t t) {
  if (atomicExch(flags + t, 1u) == 0u) atomicAdd(count, 1u);
}

// One thread per voxel i < n and per flag word i < 2 * ntiles.  trav[i]: the header's traversable(v), from the ESDF
// pass's state and field.  cost[i]: NONE; continuing (`resume`), a traversable voxel keeps what the buffer holds
// unless that is no possible cost (then NONE), so that whatever the caller left there, every word in play is a finite
// cost <= kCostMax or NONE and no sum wraps.  Flags: none set (the goals mark their tiles), or all of parity 0 set.
__global__ __launch_bounds__(256) void k_cost_seed(const uint8_t* __restrict__ st, const float* __restrict__ field,
                                                   float clearance, uint32_t through_unknown, uint32_t resume,
                                                   uint32_t n, uint32_t ntiles, uint8_t* __restrict__ trav,
                                                   uint32_t* cost, uint32_t* __restrict__ flags,
                                                   uint32_t* __restrict__ counts) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < n) {
    const uint32_t s = st[i];
    const bool t = (s == kEsdfFree || (s == kEsdfUnknown && through_unknown != 0u)) && !(field[i] < clearance);
    trav[i] = t ? 1 : 0;
    uint32_t c = kCostNone;
    if (resume && t) {
      c = cost[i];
      if (c > kCostMax) c = kCostNone;
    }
    cost[i] = c;
  }
  if (i < 2u * ntiles) flags[i] = (resume && i < ntiles) ? 1u : 0u;
  if (i == 0u) counts[0] = resume ? ntiles : 0u, counts[1] = 0u;
}

// The neighbouring tiles that have voxel (lx, ly, lz) of a tile in their halo, up to 7 of the 26 (face moves only: 3),
// as a mask: bit (sx + 1) + 3 (sy + 1) + 9 (sz + 1) for the neighbour at tile offset (sx, sy, sz).  Whoever lowers a
// word owes these tiles a mark: k_cost_goals for a goal, k_cost_relax for the words of a round.
template <bool kFacesOnly>
__device__ inline uint32_t cost_halo_mask(int lx, int ly, int lz) {
  const int fx = lx == 0 ? -1 : (lx == kRegTX - 1 ? 1 : 0), fy = ly == 0 ? -1 : (ly == kRegTY - 1 ? 1 : 0);
  const int fz = lz == 0 ? -1 : (lz == kRegTZ - 1 ? 1 : 0);
  uint32_t mask = 0u;
#pragma unroll
  for (int c = 1; c < 8; ++c) {
    const int sx = (c & 1) ? fx : 0, sy = (c & 2) ? fy : 0, sz = (c & 4) ? fz : 0;
    const int moved = (sx != 0) + (sy != 0) + (sz != 0);
    if (moved == 0 || (kFacesOnly && moved != 1)) continue;
    mask |= 1u << ((sx + 1) + 3 * (sy + 1) + 9 * (sz + 1));
  }
  return mask;
}
// the neighbour of tile (tx, ty, tz) that bit d of such a mask names, marked if it exists
__device__ inline void cost_mark_neighbour(uint32_t* flags, uint32_t* count, int d, int tx, int ty, int tz, int ntx,
                                           int nty, int ntz) {
  const int ux = tx + d % 3 - 1, uy = ty + (d / 3) % 3 - 1, uz = tz + d / 9 - 1;
  if ((unsigned)ux < (unsigned)ntx && (unsigned)uy < (unsigned)nty && (unsigned)uz < (unsigned)ntz)
    cost_mark(flags, count, (uint32_t)ux + (uint32_t)ntx * ((uint32_t)uy + (uint32_t)nty * (uint32_t)uz));
}

// One thread per goal (absolute voxel triples).  Outside the box or on a voxel that is not traversable: ignored.
// Duplicates store the same word and mark the same tiles.  A goal's word is lowered HERE, not in a round, so this
// kernel owes the marks a round would make for it: the goal's own tile and every tile whose halo holds the goal (a
// goal on a tile face may be the only way across that face).
template <bool kFacesOnly>
__global__ __launch_bounds__(256) void k_cost_goals(const int32_t* __restrict__ goals, uint32_t n_goals, MapBox b,
                                                    int ntx, int nty, int ntz, const uint8_t* __restrict__ trav,
                                                    uint32_t* cost, uint32_t* flags, uint32_t* counts) {
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  if (g >= n_goals) return;
  const long long x = (long long)goals[3 * (size_t)g] - b.ox, y = (long long)goals[3 * (size_t)g + 1] - b.oy,
                  z = (long long)goals[3 * (size_t)g + 2] - b.oz;
  if (x < 0 || x >= b.X || y < 0 || y >= b.Y || z < 0 || z >= b.Z) return;
  const uint32_t i = (uint32_t)x + (uint32_t)b.X * ((uint32_t)y + (uint32_t)b.Y * (uint32_t)z);
  if (!trav[i]) return;
  __hip_atomic_store(cost + i, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const int tx = (int)x / kRegTX, ty = (int)y / kRegTY, tz = (int)z / kRegTZ;
  cost_mark(flags, counts, (uint32_t)tx + (uint32_t)ntx * ((uint32_t)ty + (uint32_t)nty * (uint32_t)tz));
  const uint32_t mask = cost_halo_mask<kFacesOnly>((int)x % kRegTX, (int)y % kRegTY, (int)z % kRegTZ);
  for (int d = 0; d < 27; ++d)
    if ((mask >> d) & 1u) cost_mark_neighbour(flags, counts, d, tx, ty, tz, ntx, nty, ntz);
}

// One round.  Tile t = blockIdx.x (x fastest, as k_regions_local); thread: the column (lx, ly), its four voxels.
// `now` / `next`: the dirty flags and counts of this round's parity and of the next round's.
//
// Who writes what.  A cost word is written by the workgroup of its own tile only (the halo is read, never written),
// so no two workgroups of a round write one word.  A tile clears its own flag of `now` and nobody else touches `now`
// in this round; marks go to `next`, which no tile reads in this round.
//
// Why an old word is harmless (the halo and the flags are read with relaxed agent-scope loads, which another XCD's
// store of the same round may or may not have reached).  Every value a word ever holds is the length of a real path
// from its voxel to a goal through traversable voxels of the box (0 at a goal; otherwise a neighbour's value of some
// earlier moment plus the move's weight), and a word only falls.  So whatever mixture of old and new halo words a tile
// reads, what it computes are lengths of real paths again: never below the exact cost.  And nothing is lost: WHOEVER
// lowers a word marks every tile that reads it -- k_cost_goals the goal's own tile and the tiles that have the goal in
// their halo, a tile of a round the neighbours that have a fallen word in theirs -- for the NEXT launch, and the
// kernel boundary makes the word visible to them; the neighbour then reads the new value whatever it saw this round.
// (k_cost_seed lowers nothing: from NONE everywhere no tile can lower a word, and continuing it marks every tile.)
// When a round ends with no flag set, every tile has run after the last change of every word it reads and found
// nothing to lower: the shortest-path equations hold everywhere, and their solution is unique.
//
// The sweep loop: after sweep j every voxel whose best path inside the tile (halo fixed) has at most j moves is final,
// and such a path has fewer than kRegTile voxels.  A tile that is still changing at the cap marks ITSELF and goes on
// next round.
template <bool kFacesOnly>
__global__ __launch_bounds__(256) void k_cost_relax(const uint8_t* __restrict__ trav, int X, int Y, int Z, int ntx,
                                                    int nty, int ntz, uint32_t* cost, uint32_t* now_flags,
                                                    uint32_t* now_count, uint32_t* next_flags, uint32_t* next_count) {
  __shared__ uint32_t s_c[kCostHalo];
  __shared__ uint32_t s_dirty, s_mark;
  const int tid = (int)threadIdx.x, lx = tid & (kRegTX - 1), ly = tid >> 5;
  const uint32_t t = blockIdx.x;
  if (tid == 0) {
    s_dirty = __hip_atomic_load(now_flags + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_mark = 0u;
  }
  __syncthreads();
  if (s_dirty == 0u) return;  // (the whole workgroup)
  if (tid == 0) {
    __hip_atomic_store(now_flags + t, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    atomicSub(now_count, 1u);
  }
  const int tx = (int)(t % (uint32_t)ntx), ty = (int)((t / (uint32_t)ntx) % (uint32_t)nty);
  const int tz = (int)(t / ((uint32_t)ntx * (uint32_t)nty));
  const int x0 = tx * kRegTX, y0 = ty * kRegTY, z0 = tz * kRegTZ;
  for (int i = tid; i < kCostHalo; i += 256) {
    const int x = x0 + i % kCostHX - 1, y = y0 + (i / kCostHX) % kCostHY - 1, z = z0 + i / (kCostHX * kCostHY) - 1;
    uint32_t v = kCostNone;  // outside the box: nothing to step to
    if ((unsigned)x < (unsigned)X && (unsigned)y < (unsigned)Y && (unsigned)z < (unsigned)Z)
      v = __hip_atomic_load(cost + ((size_t)x + (size_t)X * ((size_t)y + (size_t)Y * (size_t)z)), __ATOMIC_RELAXED,
                            __HIP_MEMORY_SCOPE_AGENT);
    s_c[i] = v;
  }
  const int x = x0 + lx, y = y0 + ly;
  const bool in_xy = x < X && y < Y;
  uint32_t open = 0u;  // bit k: voxel k of the column is in the box and traversable
#pragma unroll
  for (int k = 0; k < kRegTZ; ++k)
    if (in_xy && z0 + k < Z && trav[(size_t)x + (size_t)X * ((size_t)y + (size_t)Y * (size_t)(z0 + k))]) open |= 1u << k;
  __syncthreads();
  const int centre = (lx + 1) + kCostHX * (ly + 1);  // the column in a plane of the halo block
  uint32_t first[kRegTZ], cur[kRegTZ];
#pragma unroll
  for (int k = 0; k < kRegTZ; ++k) first[k] = cur[k] = s_c[centre + kCostHX * kCostHY * (k + 1)];

  int again = open != 0u;  // (a column with nothing open never changes anything)
  again = __syncthreads_or(again);
  int sweep = 0;
  for (; again && sweep < kRegTile; ++sweep) {
    int changed = 0;
    if (open) {
      // the 3 x 3 columns around this one, all six planes: what the other columns held at some moment since the last
      // barrier (old or new: see above); this column's own words come from registers
      uint32_t nb[kCostHZ][9];
#pragma unroll
      for (int p = 0; p < kCostHZ; ++p)
#pragma unroll
        for (int j = 0; j < 9; ++j)
          nb[p][j] = __hip_atomic_load(s_c + centre + kCostHX * kCostHY * p + (j % 3 - 1) + kCostHX * (j / 3 - 1),
                                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#pragma unroll
      for (int k = 0; k < kRegTZ; ++k) {
        if (!((open >> k) & 1u)) continue;
        uint32_t best = cur[k];
#pragma unroll
        for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
          for (int j = 0; j < 9; ++j) {
            const int dx = j % 3 - 1, dy = j / 3 - 1;
            if (dx == 0 && dy == 0 && dz == 0) continue;
            if (kFacesOnly && (dx != 0) + (dy != 0) + (dz != 0) != 1) continue;
            best = min(best, cost_step(nb[k + 1 + dz][j], cost_weight(dx, dy, dz)));
          }
        if (best < cur[k]) {
          cur[k] = best;
          nb[k + 1][4] = best;  // the voxel above it in this column sees it in this sweep
          __hip_atomic_store(s_c + centre + kCostHX * kCostHY * (k + 1), best, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_WORKGROUP);
          changed = 1;
        }
      }
    }
    again = __syncthreads_or(changed);
  }

  // the words that fell, and the tiles whose halo they are in: bit (sx + 1) + 3 (sy + 1) + 9 (sz + 1) of the mark
  uint32_t mark = 0u;
#pragma unroll
  for (int k = 0; k < kRegTZ; ++k) {
    if (!(cur[k] < first[k])) continue;
    const int z = z0 + k;
    __hip_atomic_store(cost + ((size_t)x + (size_t)X * ((size_t)y + (size_t)Y * (size_t)z)), cur[k], __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
    mark |= cost_halo_mask<kFacesOnly>(lx, ly, k);
  }
  if (mark) atomicOr(&s_mark, mark);
  __syncthreads();
  if (tid < 27 && ((s_mark >> tid) & 1u)) cost_mark_neighbour(next_flags, next_count, tid, tx, ty, tz, ntx, nty, ntz);
  if (tid == 13 && again) cost_mark(next_flags, next_count, t);  // stopped at the cap: goes on next round
}

__device__ inline uint32_t wave_all_umax(uint32_t v) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) v = max(v, (uint32_t)__shfl_xor((int)v, d, 64));
  return v;
}

// ratsdf_cost_summary as eight words, accumulated where it is delivered (zeroed in front of this launch):
//   goals | traversable | reached | max_cost | pending | rounds | 0 | 0
// A workgroup takes kCostChunk consecutive voxels; a lane sums its 16, a wave its lanes, the workgroup its four waves,
// and one lane sends: integer adds and a max, so the grouping does not reach the result.
constexpr int kCostPerLane = 16, kCostChunk = 256 * kCostPerLane;
__global__ __launch_bounds__(256) void k_cost_summary(const uint8_t* __restrict__ trav, const uint32_t* __restrict__ cost,
                                                      uint32_t n, const uint32_t* __restrict__ pending, uint32_t rounds,
                                                      uint32_t* sum) {
  __shared__ uint32_t s_part[4][4];
  int goals = 0, open = 0, reached = 0;
  uint32_t most = 0u;
  for (int k = 0; k < kCostPerLane; ++k) {
    const uint32_t i = blockIdx.x * (uint32_t)kCostChunk + (uint32_t)k * 256u + threadIdx.x;
    if (i >= n) continue;
    const uint32_t c = cost[i];
    open += trav[i] != 0;
    if (c == kCostNone) continue;
    ++reached;
    goals += c == 0u;
    most = max(most, c);
  }
  goals = wave_all_sum(goals), open = wave_all_sum(open), reached = wave_all_sum(reached);
  most = wave_all_umax(most);
  const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
  if (lane == 0) s_part[wave][0] = (uint32_t)goals, s_part[wave][1] = (uint32_t)open, s_part[wave][2] = (uint32_t)reached, s_part[wave][3] = most;
  __syncthreads();
  if (threadIdx.x != 0) return;
  uint32_t g = 0u, o = 0u, r = 0u, m = 0u;
  for (int w = 0; w < 4; ++w) g += s_part[w][0], o += s_part[w][1], r += s_part[w][2], m = max(m, s_part[w][3]);
  if (g) atomicAdd(sum + 0, g);
  if (o) atomicAdd(sum + 1, o);
  if (r) atomicAdd(sum + 2, r);
  if (m) atomicMax(sum + 3, m);
  if (blockIdx.x == 0u) sum[4] = *pending, sum[5] = rounds;  // (6 and 7 stay 0)
}

// The move of every voxel, from the delivered field: 255 at cost 0, 254 at NONE, otherwise the code
// (dx + 1) + 3 (dy + 1) + 9 (dz + 1) of the move to a neighbour u inside the box with a finite cost that minimises
// cost[u] + w, the smallest code among equals (254 where a finite voxel has no such neighbour: not a field of this
// engine).
template <bool kFacesOnly>
__global__ __launch_bounds__(256) void k_cost_next(const uint32_t* __restrict__ cost, int X, int Y, int Z, uint32_t n,
                                                   uint8_t* __restrict__ next) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint32_t c = cost[i];
  uint32_t code = c == 0u ? kCostAtGoal : kCostNoStep;
  if (c != 0u && c != kCostNone) {
    const uint32_t XY = (uint32_t)X * (uint32_t)Y;
    const int x = (int)(i % (uint32_t)X), y = (int)(i / (uint32_t)X % (uint32_t)Y), z = (int)(i / XY);
    uint32_t best = kCostNone;
#pragma unroll
    for (int d = 0; d < 27; ++d) {
      const int dx = d % 3 - 1, dy = (d / 3) % 3 - 1, dz = d / 9 - 1;
      const int moved = (dx != 0) + (dy != 0) + (dz != 0);
      if (moved == 0 || (kFacesOnly && moved != 1)) continue;
      const int ux = x + dx, uy = y + dy, uz = z + dz;
      if ((unsigned)ux >= (unsigned)X || (unsigned)uy >= (unsigned)Y || (unsigned)uz >= (unsigned)Z) continue;
      const uint32_t s = cost_step(cost[(uint32_t)ux + (uint32_t)X * ((uint32_t)uy + (uint32_t)Y * (uint32_t)uz)],
                                   cost_weight(dx, dy, dz));
      if (s < best) best = s, code = (uint32_t)d;
    }
  }
  next[i] = (uint8_t)code;
}

}  // namespace ratsdf
