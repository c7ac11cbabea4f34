// kernels_esdf.h -- the Euclidean signed distance field over a box of the map (include/ratsdf_esdf.h).  No reference
// counterpart.
//
// An exact separable transform (Meijster, Roerdink & Hesselink 2000) run for both sets at once -- the squared
// distance to the obstacle set O and to its complement in the box -- so each pass reads and writes the box once:
//   k_esdf_seed    one workgroup per map block the box meets: one lane resolves the block through the directory, the
//                  lanes read its tsdf / rgbw as 2 KB lines and write the state byte of each voxel inside the box
//   k_esdf_x       one wave per row (x, the contiguous axis): the nearest member of O and of box \ O on the left
//                  and on the right of each voxel come from wave-wide max / min scans of positions; out: the two 1D
//                  distances as a uint16 pair (0xFFFF: none on the row)
//   k_esdf_col     one lane per column, lanes adjacent in x (every step's loads and stores are contiguous across the
//                  wave): Meijster's phase 2 with the integer separator, y then z.  The per-column stacks live in a
//                  global workspace laid out [k][column]; the top of each stack stays in registers.  The z pass
//                  writes the signed float.
// Squared distances are int32 with kEsdfInf (2^30) for "nothing on this line" and clamped to it after every pass:
// every term of Sep and of the envelope comparison stays below 2^30 + 3 * 1023^2 < 2^31.
// The map is only read: no directory entry, pool word, free-list slot or delta bit is written.
#pragma once
#include "map_read.h"

namespace ratsdf {

constexpr int32_t kEsdfInf = 1 << 30;
constexpr uint32_t kEsdfUnknown = 0u, kEsdfFree = 1u, kEsdfOccupied = 2u;  // RATSDF_ESDF_STATE_*
constexpr int kEsdfColWG = 64;  // lanes (columns) per workgroup of k_esdf_col: small boxes have few columns

// state bytes of the box's voxels that lie in one map block (blockIdx.x: the block, x fastest)
__global__ __launch_bounds__(256) void k_esdf_seed(Table tab, Pool pool, MapBox b, float occupied_below,
                                                   uint8_t* __restrict__ st) {
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
    if (blk >= 0) {
      const size_t p = ((size_t)blk << 9) + (size_t)v;
      const float t = pool.tsdf[p];
      const uint32_t w = pool.rgbw[p] >> 24;
      s = w == 0u ? kEsdfUnknown : (t <= occupied_below ? kEsdfOccupied : kEsdfFree);
    }
    if ((unsigned)x < (unsigned)b.X && (unsigned)y < (unsigned)b.Y && (unsigned)z < (unsigned)b.Z)
      st[(size_t)x + (size_t)b.X * ((size_t)y + (size_t)b.Y * (size_t)z)] = (uint8_t)s;
  }
}

__device__ inline int wave_scan_max(int v, int lane) {  // inclusive, lanes 0 .. lane
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl_up(v, d, 64);
    if (lane >= d) v = max(v, t);
  }
  return v;
}
__device__ inline int wave_scan_min_rev(int v, int lane) {  // inclusive, lanes lane .. 63
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl_down(v, d, 64);
    if (lane + d < 64) v = min(v, t);
  }
  return v;
}

// 1D distances along x.  omask: bit s set <=> state s is in O.  gx[v] = d(O) | d(box \ O) << 16, 0xFFFF for none.
constexpr int kEsdfNone = 4096;  // a position "beyond the row" on either side: any distance to it exceeds 1023
__global__ __launch_bounds__(256) void k_esdf_x(const uint8_t* __restrict__ st, uint32_t omask, int X, uint32_t rows,
                                                uint32_t* __restrict__ gx) {
  __shared__ uint32_t s_left[4][1024];  // per wave: nearest O | box \ O position at or left of x, each + kEsdfNone
  const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
  const uint32_t row = blockIdx.x * 4u + (uint32_t)wave;
  if (row >= rows) return;  // (no barrier below: each wave keeps to its own LDS row)
  const uint8_t* r = st + (size_t)row * (size_t)X;
  uint32_t* o = gx + (size_t)row * (size_t)X;
  uint32_t* left = s_left[wave];
  int c0 = -kEsdfNone, c1 = -kEsdfNone;
  for (int base = 0; base < X; base += 64) {
    const int x = base + lane;
    const bool in = x < X;
    const bool ob = in && ((omask >> r[in ? x : 0]) & 1u);
    const int a0 = max(wave_scan_max(in && ob ? x : -kEsdfNone, lane), c0);
    const int a1 = max(wave_scan_max(in && !ob ? x : -kEsdfNone, lane), c1);
    c0 = __shfl(a0, 63, 64);
    c1 = __shfl(a1, 63, 64);
    if (in) left[x] = (uint32_t)(a0 + kEsdfNone) | ((uint32_t)(a1 + kEsdfNone) << 16);
  }
  c0 = c1 = 2 * kEsdfNone;
  for (int base = (X - 1) & ~63; base >= 0; base -= 64) {
    const int x = base + lane;
    const bool in = x < X;
    const bool ob = in && ((omask >> r[in ? x : 0]) & 1u);
    const int b0 = min(wave_scan_min_rev(in && ob ? x : 2 * kEsdfNone, lane), c0);
    const int b1 = min(wave_scan_min_rev(in && !ob ? x : 2 * kEsdfNone, lane), c1);
    c0 = __shfl(b0, 0, 64);
    c1 = __shfl(b1, 0, 64);
    if (in) {
      const uint32_t l = left[x];
      const int d0 = min(x - ((int)(l & 0xFFFFu) - kEsdfNone), b0 - x);
      const int d1 = min(x - ((int)(l >> 16) - kEsdfNone), b1 - x);
      o[x] = (uint32_t)(d0 < 1024 ? d0 : 0xFFFF) | ((uint32_t)(d1 < 1024 ? d1 : 0xFFFF) << 16);
    }
  }
}

// one lower envelope of Meijster's phase 2: the top of the stack in registers, the rest at stk[k * ncols]
struct EsdfEnv {
  int s, t, fs;  // top: the parabola's apex position, where it starts to be the minimum, its offset f(s)
  int q;         // entries below the top
};
__device__ inline void env_start(EsdfEnv& E, int f0) { E.s = 0, E.t = 0, E.fs = f0, E.q = 0; }
__device__ inline uint2 env_pack(const EsdfEnv& E) { return make_uint2((uint32_t)E.s | ((uint32_t)E.t << 16), (uint32_t)E.fs); }
__device__ inline void env_unpack(EsdfEnv& E, uint2 w) {
  E.s = (int)(w.x & 0xFFFFu), E.t = (int)(w.x >> 16), E.fs = (int)w.y;
}
// the forward scan's step u with f(u) = fu over a column of n
__device__ inline void env_add(EsdfEnv& E, int u, int fu, int n, uint2* __restrict__ stk, uint32_t ncols) {
  for (;;) {
    const int dt = E.t - E.s, du = E.t - u;
    if (dt * dt + E.fs <= du * du + fu) break;  // the top still wins where it starts
    if (E.q == 0) {                              // u wins everywhere the stack did: it becomes the only entry
      E.s = u, E.t = 0, E.fs = fu;
      return;
    }
    --E.q;
    env_unpack(E, stk[(size_t)E.q * ncols]);
  }
  // Sep(s, u) = (u^2 - s^2 + f(u) - f(s)) div (2 (u - s)); the numerator is >= 0 here (the top wins at t >= 0)
  const int w = 1 + (u * u - E.s * E.s + fu - E.fs) / (2 * (u - E.s));
  if (w < n) {
    stk[(size_t)E.q * ncols] = env_pack(E);
    ++E.q;
    E.s = u, E.t = w, E.fs = fu;
  }
}

// kPass 1: y (in: the x pass's uint16 pairs, out: squared-distance pairs); kPass 2: z (in: pairs, out: the field).
// Column c: x = c % X, base = x + (c / X) * plane, voxels base + u * stride for u < n.
template <int kPass>
__global__ __launch_bounds__(kEsdfColWG) void k_esdf_col(const void* __restrict__ in, int n, int X, uint32_t plane,
                                                         uint32_t stride, uint32_t ncols, uint2* __restrict__ stk0,
                                                         uint2* __restrict__ stk1, void* __restrict__ out, float vs) {
  const uint32_t c = blockIdx.x * (uint32_t)kEsdfColWG + threadIdx.x;
  if (c >= ncols) return;
  const size_t base = (size_t)(c % (uint32_t)X) + (size_t)(c / (uint32_t)X) * plane;
  uint2* s0 = stk0 + c;
  uint2* s1 = stk1 + c;
  auto load = [&](int u) -> uint2 {  // (f to O, f to box \ O) of voxel u of the column
    const size_t v = base + (size_t)u * stride;
    if (kPass == 1) {
      const uint32_t w = ((const uint32_t*)in)[v];
      const int a = (int)(w & 0xFFFFu), b = (int)(w >> 16);
      return make_uint2(a == 0xFFFF ? (uint32_t)kEsdfInf : (uint32_t)(a * a),
                        b == 0xFFFF ? (uint32_t)kEsdfInf : (uint32_t)(b * b));
    }
    return ((const uint2*)in)[v];
  };
  EsdfEnv e0, e1;
  uint2 f = load(0);
  env_start(e0, (int)f.x);
  env_start(e1, (int)f.y);
  uint2 nx = load(n > 1 ? 1 : 0);
  for (int u = 1; u < n; ++u) {
    f = nx;
    nx = load(u + 1 < n ? u + 1 : u);  // one step ahead
    env_add(e0, u, (int)f.x, n, s0, ncols);
    env_add(e1, u, (int)f.y, n, s1, ncols);
  }
  for (int u = n - 1; u >= 0; --u) {
    const int d0 = u - e0.s, d1 = u - e1.s;
    const int v0 = min(d0 * d0 + e0.fs, kEsdfInf), v1 = min(d1 * d1 + e1.fs, kEsdfInf);
    const size_t v = base + (size_t)u * stride;
    if (kPass == 1) {
      ((uint2*)out)[v] = make_uint2((uint32_t)v0, (uint32_t)v1);
    } else {
      // v in O <=> its distance to O is 0; the contract's fp32 formula.  sqrtf is the correctly rounded square root
      // (llvm.sqrt.f32: v_sqrt_f32 and its correction steps, read in the listing).  NOT __fsqrt_rn: unless the
      // headers are built with OCML_BASIC_ROUNDED_OPERATIONS that is __ocml_native_sqrt_f32, the bare v_sqrt_f32,
      // which is not correctly rounded (it broke byte equality with the restatement on the MI355X).
      float r;
      if (v0 == 0) r = v1 >= kEsdfInf ? -INFINITY : -(sqrtf((float)v1) * vs);
      else r = v0 >= kEsdfInf ? INFINITY : sqrtf((float)v0) * vs;
      ((float*)out)[v] = r;
    }
    if (u == e0.t && e0.q > 0) env_unpack(e0, s0[(size_t)--e0.q * ncols]);
    if (u == e1.t && e1.q > 0) env_unpack(e1, s1[(size_t)--e1.q * ncols]);
  }
}

}  // namespace ratsdf
