// kernels_exposure.h -- the exposure of surface points to lamps through a box of the map (include/ratsdf_surface.h,
// ratsdf_exposure*).  No reference counterpart.
//
// The box's states come from k_esdf_seed (kernels_esdf.h), launched unchanged; then
//   k_exposure_pack   one lane per 4 x 4 x 4 brick of the box (box-relative, x fastest): the 64 state bytes into one
//                     64-bit word, bit (x & 3) + 4 (y & 3) + 16 (z & 3) set <=> the voxel is BLOCKING; voxels of an
//                     edge brick beyond the box are set.  Lanes adjacent in x read adjacent bytes of a row.
//   k_exposure_lamps  one wave: lane k resolves lamp k -- its voxel, box-relative, and whether it is accepted -- and
//                     starts the lamp table and the summary.
//   k_exposure_walk   one lane per (point, lamp) pair.  A wave holds 64 / M points, M = n_lamps rounded up to a power
//                     of two, the M lanes of a point side by side: they start in the same voxel, so their first
//                     steps read the same words.  The walk itself is integer only and keeps the current brick's word
//                     in a register: a new word about every fourth step.  It never leaves the bounding box of its two
//                     ends, both of which lie in the box, so every brick index is in range.  A wave's visible pairs
//                     are one ballot; a point's mask is its M bits of it; its dose is summed by walking the ballot's
//                     set bits in ascending order with one readlane each -- the order is the contract, so no tree.
//                     Counts go through integer atomics in LDS and once per workgroup to memory: deterministic.  No
//                     float atomics.
// The map is only read: no directory entry, pool word, free-list slot or delta bit is written.
#pragma once
#include "kernels_esdf.h"

namespace ratsdf {

constexpr int kExposureMaxLamps = 64;
constexpr uint32_t kExposureMaxWG = 4096;  // workgroups of k_exposure_walk: each strides over the waves' batches

// the bricks of a box
struct ExposureGrid {
  int nbx, nby, nbz;  // bricks per axis
  uint32_t nbricks;
};

__global__ __launch_bounds__(256) void k_exposure_pack(const uint8_t* __restrict__ st, int X, int Y, int Z,
                                                       ExposureGrid g, uint32_t unknown_blocks,
                                                       unsigned long long* __restrict__ bits) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= g.nbricks) return;
  const int x0 = (int)(i % (uint32_t)g.nbx) * 4, y0 = (int)((i / (uint32_t)g.nbx) % (uint32_t)g.nby) * 4;
  const int z0 = (int)(i / ((uint32_t)g.nbx * (uint32_t)g.nby)) * 4;
  unsigned long long w = 0ull;
  for (int r = 0; r < 16; ++r) {
    const int y = y0 + (r & 3), z = z0 + (r >> 2);
    uint32_t row = 0xFu;  // beyond the box: blocking
    if (y < Y && z < Z) {
      const uint8_t* p = st + (size_t)X * ((size_t)y + (size_t)Y * (size_t)z);
      row = 0u;
#pragma unroll
      for (int dx = 0; dx < 4; ++dx) {
        const int x = x0 + dx;
        bool blocking = true;
        if (x < X) {
          const uint32_t s = p[x];
          blocking = s == kEsdfOccupied || (s == kEsdfUnknown && unknown_blocks != 0u);
        }
        row |= (blocking ? 1u : 0u) << dx;
      }
    }
    w |= (unsigned long long)row << (4 * r);
  }
  bits[i] = w;
}

__device__ inline bool exposure_blocking(const unsigned long long* __restrict__ bits, const ExposureGrid& g, int x,
                                         int y, int z) {
  const uint32_t brick = (uint32_t)(x >> 2) + (uint32_t)g.nbx * ((uint32_t)(y >> 2) + (uint32_t)g.nby * (uint32_t)(z >> 2));
  return (bits[brick] >> ((x & 3) | ((y & 3) << 2) | ((z & 3) << 4))) & 1ull;
}

// (float)lo <= f < (float)(lo + n), false for a NaN; lo and lo + n are exact in fp32 (|.| <= 32768)
__device__ inline bool exposure_in_box(float f, int lo, int n) { return f >= (float)lo && f < (float)(lo + n); }

// lamp_vox[k] = (L - origin, accepted); table[k] = (accepted, 0, 0, 0) when there is a table; the summary's start
__global__ __launch_bounds__(64) void k_exposure_lamps(const float4* __restrict__ lamps, int n_lamps, MapBox b, float vs,
                                                       const unsigned long long* __restrict__ bits, ExposureGrid g,
                                                       int4* __restrict__ lamp_vox, int4* __restrict__ table,
                                                       uint32_t* __restrict__ summary) {
  const int k = (int)threadIdx.x;
  bool accepted = false;
  if (k < n_lamps) {
    const float4 l = lamps[k];
    const float fx = l.x / vs + 0.5f, fy = l.y / vs + 0.5f, fz = l.z / vs + 0.5f;
    int4 v = make_int4(0, 0, 0, 0);
    if (exposure_in_box(fx, b.ox, b.X) && exposure_in_box(fy, b.oy, b.Y) && exposure_in_box(fz, b.oz, b.Z)) {
      v.x = (int)floorf(fx) - b.ox, v.y = (int)floorf(fy) - b.oy, v.z = (int)floorf(fz) - b.oz;
      accepted = !exposure_blocking(bits, g, v.x, v.y, v.z);
    }
    v.w = accepted ? 1 : 0;
    lamp_vox[k] = v;
    if (table) table[k] = make_int4(v.w, 0, 0, 0);
  }
  const unsigned long long acc = __builtin_amdgcn_ballot_w64(accepted);
  if (k < 8) summary[k] = k == 4 ? (uint32_t)__popcll(acc) : 0u;  // lit_pairs | points_lit | points_outside | lamps_accepted | reserved
}

struct ExposureArgs {
  const float4* points;  // ratsdf_surface_point: two float4 each (pos, normal.x | normal.yz, prob, rgbw)
  const float4* lamps;
  const int4* lamp_vox;
  const unsigned long long* bits;
  float* dose;
  unsigned long long* mask;  // may be null
  int4* table;               // may be null
  uint32_t* summary;
  uint32_t n_points;
  int n_lamps;
  int log_m;  // M = 1 << log_m lanes per point
  float vs, max_range, min_irradiance, p_cutoff;
  uint32_t accumulate;
};

__global__ __launch_bounds__(256) void k_exposure_walk(ExposureArgs a, MapBox b, ExposureGrid g, uint32_t n_batches) {
  __shared__ uint32_t s_lit[kExposureMaxLamps], s_high[kExposureMaxLamps];
  __shared__ uint32_t s_sum[3];  // visible pairs | points lit | points outside
  if (threadIdx.x < (unsigned)kExposureMaxLamps) s_lit[threadIdx.x] = 0u, s_high[threadIdx.x] = 0u;
  if (threadIdx.x < 3u) s_sum[threadIdx.x] = 0u;
  __syncthreads();
  const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
  const int m = 1 << a.log_m, k = lane & (m - 1), first = lane & ~(m - 1);
  const uint32_t per_wave = 64u >> a.log_m;
  const float mr2 = a.max_range * a.max_range;
  // this lane's lamp, the same for every batch
  const bool has_lamp = k < a.n_lamps;
  float4 lamp = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  int4 lv = make_int4(0, 0, 0, 0);
  if (has_lamp) lamp = a.lamps[k], lv = a.lamp_vox[k];
  for (uint32_t batch = blockIdx.x * 4u + (uint32_t)wave; batch < n_batches; batch += gridDim.x * 4u) {
    const uint32_t i = batch * per_wave + (uint32_t)(lane >> a.log_m);
    const bool has_point = i < a.n_points;
    bool outside = false, visible = false, lit = false, high = false;
    float e = 0.0f;
    if (has_point) {
      const float4 p0 = a.points[2 * (size_t)i], p1 = a.points[2 * (size_t)i + 1];
      const float px = p0.x, py = p0.y, pz = p0.z, nx = p0.w, ny = p1.x, nz = p1.y, prob = p1.z;
      const float fx = (px / a.vs + nx) + 0.5f, fy = (py / a.vs + ny) + 0.5f, fz = (pz / a.vs + nz) + 0.5f;
      outside = !(exposure_in_box(fx, b.ox, b.X) && exposure_in_box(fy, b.oy, b.Y) && exposure_in_box(fz, b.oz, b.Z));
      if (!outside && has_lamp && lv.w != 0) {
        const float dx = lamp.x - px, dy = lamp.y - py, dz = lamp.z - pz;
        const float r2 = dx * dx + dy * dy + dz * dz;
        const float c = nx * dx + ny * dy + nz * dz;
        if (c > 0.0f && !(r2 > mr2)) {
          // the walk: position (x, y, z), box-relative, from s to L
          int x = (int)floorf(fx) - b.ox, y = (int)floorf(fy) - b.oy, z = (int)floorf(fz) - b.oz;
          const int sx = lv.x > x ? 1 : -1, sy = lv.y > y ? 1 : -1, sz = lv.z > z ? 1 : -1;
          const int n0 = abs(lv.x - x), n1 = abs(lv.y - y), n2 = abs(lv.z - z);
          int t0 = 1, t1 = 1, t2 = 1;     // 2 k[a] + 1
          int left = n0 + n1 + n2;        // steps to go
          uint32_t brick = (uint32_t)(x >> 2) + (uint32_t)g.nbx * ((uint32_t)(y >> 2) + (uint32_t)g.nby * (uint32_t)(z >> 2));
          unsigned long long word = a.bits[brick];
          bool clear = true;
          for (;;) {
            if ((word >> ((x & 3) | ((y & 3) << 2) | ((z & 3) << 4))) & 1ull) {
              clear = false;
              break;
            }
            if (left == 0) break;
            --left;
            // the axis with the smallest (2 k + 1) / n among those with steps left (2 k + 1 < 2 n); ties: the lowest
            int axis = t0 < 2 * n0 ? 0 : (t1 < 2 * n1 ? 1 : 2);
            int tb = axis == 0 ? t0 : (axis == 1 ? t1 : t2), nb = axis == 0 ? n0 : (axis == 1 ? n1 : n2);
            if (axis < 1 && t1 < 2 * n1 && t1 * nb < tb * n1) axis = 1, tb = t1, nb = n1;
            if (axis < 2 && t2 < 2 * n2 && t2 * nb < tb * n2) axis = 2;
            if (axis == 0) x += sx, t0 += 2;
            else if (axis == 1) y += sy, t1 += 2;
            else z += sz, t2 += 2;
            const uint32_t nbrick =
                (uint32_t)(x >> 2) + (uint32_t)g.nbx * ((uint32_t)(y >> 2) + (uint32_t)g.nby * (uint32_t)(z >> 2));
            if (nbrick != brick) brick = nbrick, word = a.bits[brick];
          }
          if (clear) {
            visible = true;
            e = lamp.w * (c / (r2 * sqrtf(r2))) * 0.07957747f;
            lit = e >= a.min_irradiance;
            high = lit && prob >= a.p_cutoff;
          }
        }
      }
    }
    // the wave's visible pairs; this point's are bits first .. first + m - 1
    const unsigned long long bal = __builtin_amdgcn_ballot_w64(visible);
    const unsigned long long mine = (bal >> first) & (m == 64 ? ~0ull : (1ull << m) - 1ull);
    const bool leader = has_point && k == 0;
    float acc = 0.0f;
    if (leader && a.accumulate && !outside) acc = a.dose[i];
    // ascending over the set bits, so ascending in k within every point: lane j's e to the lanes of j's point
    for (unsigned long long rest = bal; rest != 0ull; rest &= rest - 1ull) {
      const int j = __builtin_ctzll(rest);
      const float ej = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(e), j));
      if ((j & ~(m - 1)) == first) acc = acc + ej;
    }
    if (leader && !outside) a.dose[i] = acc;
    if (leader && a.mask) a.mask[i] = mine;
    if (a.table) {
      if (lit) atomicAdd(&s_lit[k], 1u);
      if (high) atomicAdd(&s_high[k], 1u);
    }
    const unsigned long long lit_points = __builtin_amdgcn_ballot_w64(leader && mine != 0ull);
    const unsigned long long out_points = __builtin_amdgcn_ballot_w64(leader && outside);
    if (lane == 0) {
      if (bal) atomicAdd(&s_sum[0], (uint32_t)__popcll(bal));
      if (lit_points) atomicAdd(&s_sum[1], (uint32_t)__popcll(lit_points));
      if (out_points) atomicAdd(&s_sum[2], (uint32_t)__popcll(out_points));
    }
  }
  __syncthreads();
  if (a.table && threadIdx.x < (unsigned)a.n_lamps) {
    if (s_lit[threadIdx.x]) atomicAdd(&a.table[threadIdx.x].y, (int)s_lit[threadIdx.x]);
    if (s_high[threadIdx.x]) atomicAdd(&a.table[threadIdx.x].z, (int)s_high[threadIdx.x]);
  }
  if (threadIdx.x == 64u && s_sum[0]) atomicAdd((unsigned long long*)a.summary, (unsigned long long)s_sum[0]);
  if (threadIdx.x == 65u && s_sum[1]) atomicAdd(&a.summary[2], s_sum[1]);
  if (threadIdx.x == 66u && s_sum[2]) atomicAdd(&a.summary[3], s_sum[2]);
}

}  // namespace ratsdf
