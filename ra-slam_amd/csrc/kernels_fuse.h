// kernels_fuse.h -- map fusion (include/ratsdf_fuse.h): the voxels of listed source blocks merged into the destination
// map's blocks with the weighted-average update of tsdf_integrate_kernel (voxel_tsdf.cu:224-248, wo = the destination's
// weight, wn = the source's).  No reference counterpart.
//
// The pass is bandwidth: 6 KB read per source block, 6 KB read and (where a voxel changes) 6 KB written in the
// destination.  One wave per block (a wave strides over the list); lane l owns voxels 8l .. 8l+7, i.e. two 16-byte accesses per array and side, so
// every wave access covers whole lines.  All twelve loads of a lane are issued before the first is used.
//
// A call makes several allocation passes over one list (an insertion can lose its bucket to another one of the same
// pass), and fusing twice is not harmless the way copying twice is: `done` holds one bit per listed block, set by the
// pass that fused it (or found that the shard filter refuses it); later passes skip the block.  What is still missing
// is counted per pass.
#pragma once
#include "map_read.h"

namespace ratsdf {

// counters of one chunk of a fusion (device scratch; the host sums the chunks)
struct FuseCounters {
  unsigned long long voxels;  // copied | averaged << 32: one atomic per wave of k_fuse_blocks
  uint32_t missing;           // blocks the directory does not hold yet (reset before every pass)
  uint32_t skipped;           // blocks the shard filter refused
  uint32_t listed;            // fuse_map: live blocks of the chunk (k_fuse_unpack)
  uint32_t pad;
};

__device__ inline bool fuse_done(const uint32_t* done, uint32_t b) { return (done[b >> 5] >> (b & 31u)) & 1u; }

// fuse_map: items [first, first + n) of the source's selection (VisItem, the machinery of ratsdf_dump_directory) as a
// position list and the pool indices beside it.  An entry left pending by a failed frame (kPlaceholderIdx) is no block:
// it is marked done from the start and never looked at again.
__global__ __launch_bounds__(256) void k_fuse_unpack(const VisItem* sel, uint32_t n, int32_t src_num_block,
                                                     int16_t* pos, int32_t* idx, uint32_t* done, FuseCounters* cnt) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const VisItem it = sel[i];
  pos[3 * i] = it.x;
  pos[3 * i + 1] = it.y;
  pos[3 * i + 2] = it.z;
  const bool live = it.idx >= 0 && it.idx < src_num_block;
  idx[i] = live ? it.idx : 0;
  if (live) atomicAdd(&cnt->listed, 1u);  // (one add per wave: the compiler sums the active lanes)
  else atomicOr(&done[i >> 5], 1u << (i & 31u));
}

// k_alloc_list for a fusion: request i has rank i; blocks that are done ask for nothing
__global__ __launch_bounds__(256) void k_fuse_alloc(Table tab, FrameParams P, const int16_t* pos, int n,
                                                    const uint32_t* done, Request* req, uint32_t req_cap,
                                                    SlowRequest* slow, uint32_t slow_cap, Ctl* ctl, uint32_t par) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n || fuse_done(done, (uint32_t)i)) return;
  const int x = pos[3 * i], y = pos[3 * i + 1], z = pos[3 * i + 2];
  if (!shard_owned(x, P)) return;
  alloc_request(tab, x, y, z, (uint32_t)i, req, req_cap, slow, slow_cap, ctl, &ctl->fr[par]);
}

__device__ inline bool fuse_contributes(uint32_t rgbw, uint32_t tsdf_bits) {
  const uint32_t w = rgbw >> 24;
  return w != 0u && !(w == 1u && tsdf_bits == 0xBF800000u);
}

// log2 of the odds p / (1 - p).  The hardware's log2 reads a subnormal input as zero (-inf where the header's logf
// gives -88 .. -103), and a probability below 2^-126 has subnormal odds: those are scaled into the normal range first,
// as the compiler's own log2 lowering does.  Every other input -- normal, zero, negative, infinite, NaN -- takes the one
// instruction it always took.  (A branch that no wave of a scanned map takes; the select form of the same costs the
// kernel two registers and with them a wave per SIMD.)
__device__ inline float fuse_log2_odds(float o) {
  float l = __builtin_amdgcn_logf(o);
  if (__builtin_expect(o < 0x1p-126f && o > 0.f, 0)) l = __builtin_amdgcn_logf(o * 0x1p32f) - 32.f;
  return l;
}

// One voxel.  Returns 0: unchanged, 1: copied, 2: averaged.
__device__ inline uint32_t fuse_voxel(uint32_t& at, uint32_t& ac, uint32_t& ap, uint32_t bt, uint32_t bc, uint32_t bp) {
  if (!fuse_contributes(bc, bt)) return 0u;
  if (!fuse_contributes(ac, at)) {
    at = bt;
    ac = bc;
    ap = bp;
    return 1u;
  }
  const float wa = (float)(ac >> 24), wb = (float)(bc >> 24);
  const float wc = wa + wb;  // 2 .. 510
  const float t = (__uint_as_float(at) * wa + __uint_as_float(bt) * wb) / wc;  // (any float may sit in an imported map)
  // colours: numerators are integers in [0, 255 * 510], the divisor in [2, 510]: div_shared's proven range
  const Recip rwc = make_recip(wc);
  const uint32_t r = rpi_abs(div_shared((float)(ac & 255u) * wa + (float)(bc & 255u) * wb, rwc));
  const uint32_t g = rpi_abs(div_shared((float)((ac >> 8) & 255u) * wa + (float)((bc >> 8) & 255u) * wb, rwc));
  const uint32_t bl = rpi_abs(div_shared((float)((ac >> 16) & 255u) * wa + (float)((bc >> 16) & 255u) * wb, rwc));
  const uint32_t w = (uint32_t)fminf(wc, 40.f);
  // probability: the log-odds form of the frame update (kernels_integrate.h), hardware log2 / exp2 / rcp
  const float pa = __uint_as_float(ap), pb = __uint_as_float(bp);
  const float la = fuse_log2_odds(pa * __builtin_amdgcn_rcpf(1.f - pa)) * 0.69314718f;
  const float lb = fuse_log2_odds(pb * __builtin_amdgcn_rcpf(1.f - pb)) * 0.69314718f;
  const float x = (wa * la + wb * lb) * rwc.r1;
  const float ex = __builtin_amdgcn_exp2f(x * -1.44269504f);
  at = __float_as_uint(t);
  ac = r | (g << 8) | (bl << 16) | (w << 24);
  ap = __float_as_uint(__builtin_amdgcn_rcpf(1.f + ex));
  return 2u;
}

// Source block b of the list: voxels at s_tsdf / s_rgbw / s_prob + (src_idx ? src_idx[b] : b) * stride words (stride
// 512 with src_idx: a pool; 512 without: three arrays of n x 512; 1536: one record {tsdf | rgbw | prob} per block, the
// pointers 0 / 512 / 1024 words into the first).  All of them 16-byte aligned.
__global__ __launch_bounds__(256) void k_fuse_blocks(Table tab, Pool pool, FrameParams P, const int16_t* pos, int n,
                                                     const int32_t* src_idx, const uint32_t* s_tsdf,
                                                     const uint32_t* s_rgbw, const uint32_t* s_prob, uint32_t stride,
                                                     uint32_t* done, FuseCounters* cnt) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave0 = __builtin_amdgcn_readfirstlane((blockIdx.x * 256u + threadIdx.x) >> 6);
  const uint32_t nwaves = gridDim.x * 4u;
  // what this wave counts over its blocks, added once at the end: a single address takes ~90 atomics per microsecond
  // ("Lessons already paid for"), and an add per block would cost a chunk more than its voxels do
  uint32_t n_missing = 0, n_skipped = 0;
  unsigned long long n_voxels = 0;  // copied | averaged << 32
  for (uint32_t b = wave0; b < (uint32_t)n; b += nwaves) {  // (uniform)
    if (fuse_done(done, b)) continue;
    const int x = pos[3 * b], y = pos[3 * b + 1], z = pos[3 * b + 2];
    if (!shard_owned(x, P)) {
      if (lane == 0) atomicOr(&done[b >> 5], 1u << (b & 31u));
      ++n_skipped;
      continue;
    }
    const int32_t idx = lookup_block(tab, x, y, z);
    if (idx < 0) {
      ++n_missing;
      continue;
    }
    const size_t so = (size_t)(src_idx ? (uint32_t)src_idx[b] : b) * stride + lane * 8u;
    const size_t d = ((size_t)idx << 9) + lane * 8u;
    const uint4* ps[3] = {reinterpret_cast<const uint4*>(s_tsdf + so), reinterpret_cast<const uint4*>(s_rgbw + so),
                          reinterpret_cast<const uint4*>(s_prob + so)};
    uint4* pd[3] = {reinterpret_cast<uint4*>(pool.tsdf + d), reinterpret_cast<uint4*>(pool.rgbw + d),
                    reinterpret_cast<uint4*>(pool.segm + d)};
    uint4 A[3][2], B[3][2];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      B[k][0] = ps[k][0];
      B[k][1] = ps[k][1];
      A[k][0] = pd[k][0];
      A[k][1] = pd[k][1];
    }
    uint32_t at[8] = {A[0][0].x, A[0][0].y, A[0][0].z, A[0][0].w, A[0][1].x, A[0][1].y, A[0][1].z, A[0][1].w};
    uint32_t ac[8] = {A[1][0].x, A[1][0].y, A[1][0].z, A[1][0].w, A[1][1].x, A[1][1].y, A[1][1].z, A[1][1].w};
    uint32_t ap[8] = {A[2][0].x, A[2][0].y, A[2][0].z, A[2][0].w, A[2][1].x, A[2][1].y, A[2][1].z, A[2][1].w};
    const uint32_t bt[8] = {B[0][0].x, B[0][0].y, B[0][0].z, B[0][0].w, B[0][1].x, B[0][1].y, B[0][1].z, B[0][1].w};
    const uint32_t bc[8] = {B[1][0].x, B[1][0].y, B[1][0].z, B[1][0].w, B[1][1].x, B[1][1].y, B[1][1].z, B[1][1].w};
    const uint32_t bp[8] = {B[2][0].x, B[2][0].y, B[2][0].z, B[2][0].w, B[2][1].x, B[2][1].y, B[2][1].z, B[2][1].w};
    uint32_t tally = 0;  // copied | averaged << 16 of this lane
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const uint32_t r = fuse_voxel(at[i], ac[i], ap[i], bt[i], bc[i], bp[i]);
      tally += r == 1u ? 1u : (r == 2u ? 0x10000u : 0u);
    }
    if (tally) {  // (a lane none of whose voxels changed writes nothing)
      pd[0][0] = make_uint4(at[0], at[1], at[2], at[3]);
      pd[0][1] = make_uint4(at[4], at[5], at[6], at[7]);
      pd[1][0] = make_uint4(ac[0], ac[1], ac[2], ac[3]);
      pd[1][1] = make_uint4(ac[4], ac[5], ac[6], ac[7]);
      pd[2][0] = make_uint4(ap[0], ap[1], ap[2], ap[3]);
      pd[2][1] = make_uint4(ap[4], ap[5], ap[6], ap[7]);
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) tally += __shfl_xor(tally, s);  // (at most 512 per half: no carry between them)
    if (lane == 0) atomicOr(&done[b >> 5], 1u << (b & 31u));  // (32 blocks share a word: spread over n / 32 addresses)
    n_voxels += (unsigned long long)(tally & 0xFFFFu) | ((unsigned long long)(tally >> 16) << 32);
  }
  if (lane == 0) {
    if (n_voxels) atomicAdd(&cnt->voxels, n_voxels);
    if (n_missing) atomicAdd(&cnt->missing, n_missing);
    if (n_skipped) atomicAdd(&cnt->skipped, n_skipped);
  }
}

}  // namespace ratsdf
