// kernels_sample.h -- batched point sampling of the map (include/ratsdf_sample.h): trilinear TSDF, its gradient, the
// nearest voxel's probability and colour, for n world points.  No reference counterpart (the nearest relative is
// VoxelHashTable::RetrieveTSDF, voxel_hash.cu:161-188, whose corner / weight pairing is mirrored: see the header).
//
// One lane per point.  The sampler is a chain of dependent round trips -- the directory probe, then the voxels -- so
// the kernel is shaped to make that chain as short as it can be, not to save instructions:
//   * the 8 corners of a point span 1, 2, 4 or 8 blocks (more than one only where a local coordinate is 7).  The
//     distinct blocks are worked out first and the home entries of ALL of them are loaded back to back (one round
//     trip), then matched; only a block whose home bucket overflowed walks its chain (rare; kernels_raycast.h
//     explains why probes one after the other cost a round trip each);
//   * every voxel load -- 8 tsdf, 8 rgbw (the weights; the nearest voxel's colour comes with them) and the nearest
//     voxel's probability -- is issued before any is used: the common point costs one probe round trip and one voxel
//     round trip;
//   * the record leaves as two 16-byte stores.
// The map is only read: no directory entry, pool word, free-list slot or delta bit is written.
#pragma once
#include "map_read.h"

namespace ratsdf {

constexpr uint32_t kSampleAllocated = 1u, kSampleObserved = 2u, kSampleNearest = 4u;  // RATSDF_SAMPLE_*

// out: 2 uint4 per point (the 32-byte ratsdf_sample).  xyz: 3 floats per point (metres).
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(6))) void k_sample(Table tab, Pool pool, const float* __restrict__ xyz, int n, float vs,
                                                uint4* __restrict__ out) {
  const int i = blockIdx.x * block_threads() + threadIdx.x;
  if (i >= n) return;
  const size_t i3 = (size_t)i * 3;
  const float gx = xyz[i3] / vs, gy = xyz[i3 + 1] / vs, gz = xyz[i3 + 2] / vs;
  const float lxf = floorf(gx), lyf = floorf(gy), lzf = floorf(gz);
  // defaults: tsdf / grad the quiet NaN 0x7FC00000 (outputs compare byte for byte), everything else 0
  uint4 r0 = make_uint4(0x7FC00000u, 0x7FC00000u, 0x7FC00000u, 0x7FC00000u), r1 = make_uint4(0u, 0u, 0u, 0u);
  if (cell_in_grid(lxf, lyf, lzf)) {
    const int lx = (int)lxf, ly = (int)lyf, lz = (int)lzf;
    const float fx = gx - lxf, fy = gy - lyf, fz = gz - lzf;
    const float ux = 1.f - fx, uy = 1.f - fy, uz = 1.f - fz;
    // the nearest voxel: roundf (half away from zero) is floor or floor + 1, i.e. corner (nx, ny, nz)
    const int nx = roundf(gx) != lxf, ny = roundf(gy) != lyf, nz = roundf(gz) != lzf;
    // which axes the corners' blocks span (local coordinate 7)
    const int bx = lx >> 3, by = ly >> 3, bz = lz >> 3;
    const int span = ((lx & 7) == 7 ? 1 : 0) | ((ly & 7) == 7 ? 2 : 0) | ((lz & 7) == 7 ? 4 : 0);
    // the distinct blocks: combination m (bit 0: x + 1, bit 1: y + 1, bit 2: z + 1) is needed iff m is inside span,
    // and corner combination m lies in block (m & span).  The home pairs of all eight are loaded back to back, then
    // matched (and the rare chain walked).  The loads are not predicated -- a lane that does not need combination m
    // loads the pair of (m & span), a line it loads anyway -- because any branch around them, per lane or per wave,
    // makes the compiler wait for each pair inside it: eight round trips instead of one.
    uint32_t e0[8];
    EntryWords ha[8], hb[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      const int mm = m & span;
      e0[m] = block_hash(bx + (mm & 1), by + ((mm >> 1) & 1), bz + ((mm >> 2) & 1), tab.bucket_mask) << 1;
      ha[m] = load_entry(tab.entries, e0[m]);
      hb[m] = load_entry(tab.entries, e0[m] + 1);
    }
    int32_t blk[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      const int mm = m & span;
      blk[m] = resolve_block(tab, bx + (mm & 1), by + ((mm >> 1) & 1), bz + ((mm >> 2) & 1), e0[m], ha[m], hb[m]);
    }
    // every voxel load before any use (not predicated either: a corner whose block is absent reads voxel 0 of pool
    // block 0, which exists, and drops the value)
    const int ax[2] = {lx & 7, (lx + 1) & 7}, ay[2] = {ly & 7, (ly + 1) & 7}, az[2] = {lz & 7, (lz + 1) & 7};
    float t[8];
    uint32_t c[8];
    bool all = true;
#pragma unroll
    for (int k = 0; k < 8; ++k) {  // corner k: x + (k >> 2), y + ((k >> 1) & 1), z + (k & 1) -- t000 .. t111
      const int32_t b = blk[(k >> 2) | (((k >> 1) & 1) << 1) | ((k & 1) << 2)];
      all = all && b >= 0;
      const size_t v = b >= 0 ? ((size_t)b << 9) + (size_t)(ax[k >> 2] + ay[(k >> 1) & 1] * 8 + az[k & 1] * 64) : 0;
      t[k] = pool.tsdf[v];
      c[k] = pool.rgbw[v];
    }
    const int kn = (nx << 2) | (ny << 1) | nz;
    const int32_t bn = blk[nx | (ny << 1) | (nz << 2)];
    float prob = pool.segm[bn >= 0 ? ((size_t)bn << 9) + (size_t)(ax[nx] + ay[ny] * 8 + az[nz] * 64) : 0];
    uint32_t cn = 0u;
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (k == kn) cn = c[k];
    if (bn < 0) prob = 0.f, cn = 0u;
    uint32_t flags = bn >= 0 ? kSampleNearest : 0u;
    uint32_t wmin = 0u;
    if (all) {
      wmin = 255u;
#pragma unroll
      for (int k = 0; k < 8; ++k) wmin = min(wmin, c[k] >> 24);
      flags |= kSampleAllocated | (wmin >= 1u ? kSampleObserved : 0u);
      // the contract of include/ratsdf_sample.h, evaluated as written (-ffp-contract=off)
      const Trilinear s = trilinear(t, fx, fy, fz, ux, uy, uz);
      const float dx = (s.c1 - s.c0) / vs;
      const float dy = ((s.c01 - s.c00) * ux + (s.c11 - s.c10) * fx) / vs;
      const float dz = (((t[1] - t[0]) * uy + (t[3] - t[2]) * fy) * ux + ((t[5] - t[4]) * uy + (t[7] - t[6]) * fy) * fx) / vs;
      r0 = make_uint4(__float_as_uint(s.value), __float_as_uint(dx), __float_as_uint(dy), __float_as_uint(dz));
    }
    r1 = make_uint4(__float_as_uint(prob), cn, wmin | (flags << 8), 0u);
  }
  out[2 * (size_t)i] = r0;
  out[2 * (size_t)i + 1] = r1;
}

}  // namespace ratsdf
