// cand_shares.h -- how the NEXT frame's candidate pass (kernels_cand.h) is cut over the launches of the current frame:
// share A rides in k_front, share B in k_alloc_rank (a launch only where the serial role is one of its own: the
// diagnostic build's RATSDF_FUSED_SERIAL=0, and one voxel per lane), share C at the head of k_integrate's grid.
// Plain C++, no HIP types: tests/cpp/test_cand_shares.cc compiles it alone and sweeps it.
// ratsdf_engine::geometry (ratsdf_engine.hip) copies the result into the launches' AheadGeom.
//
// What the kernels rely on:
//   - the shares are disjoint and together cover [0, tiles): every tile's texels are written and its blocks
//     requested exactly once;
//   - a share without a launch has no tiles;
//   - shares begin at multiples of 16 super-tiles (64 tiles): cand_pixel_work pairs neighbouring super-tiles per XCD
//     by the workgroup's number within its share, and only whole groups of 16 workgroups are paired, so a ragged end
//     may close the LAST non-empty share -- nothing begins behind it;
//   - tiles_per_wg is 4 for A and C (256-thread workgroups) and 1 .. 16 for B (1024-thread workgroups).
#pragma once
#include <cstdint>

namespace ratsdf {

struct CandShare {
  uint32_t first_tile, n_tiles, tiles_per_wg;
};

struct CandShares {
  uint32_t tiles_x;  // super-tiles per image row = ceil(W / 16)
  uint32_t tiles;    // 16x4-pixel tiles of the image, four per 16x16 super-tile
  CandShare a, b, c;
};

// split_a / split_b: percent of the super-tiles for A and B, the rest is C's; cand_wgs: look-ahead workgroups B may
// use (about one per CU); b_launched: whether the frame has a k_alloc_rank launch at all
inline CandShares cand_shares(int H, int W, int split_a, int split_b, uint32_t cand_wgs, bool b_launched) {
  CandShares s;
  s.tiles_x = (uint32_t)((W + 15) / 16);
  s.tiles = s.tiles_x * (uint32_t)((H + 15) / 16) * 4u;
  const uint32_t tiles = s.tiles, supers = tiles / 4;
  if (split_a < 0) split_a = 0;
  if (split_b < 0 || !b_launched) split_b = 0;
  if (cand_wgs < 1) cand_wgs = 1;
  // whole groups of 16 super-tiles for the shares that something follows
  uint32_t tiles_a = (uint32_t)((uint64_t)supers * (unsigned)split_a / 100) / 16 * 64;
  if (tiles_a > tiles) tiles_a = tiles;
  uint32_t tiles_b = (uint32_t)((uint64_t)supers * (unsigned)split_b / 100) / 16 * 64;
  if (tiles_b > tiles - tiles_a) tiles_b = tiles - tiles_a;
  if (split_a + split_b >= 100) {  // nothing for k_integrate: the ragged end closes the last share that runs
    if (b_launched) tiles_b = tiles - tiles_a;
    else tiles_a = tiles;
  }
  s.a = CandShare{0, tiles_a, 4};
  // a 1024-thread workgroup uses as many of its 16 waves as it needs to cover its tiles
  uint32_t tpw = (tiles_b + cand_wgs - 1) / cand_wgs;
  tpw = tpw < 1 ? 1 : tpw > 16 ? 16 : tpw;
  // (an empty share begins at 0: no workgroup reads it, and "begins at a multiple of 64" then holds for every share)
  const uint32_t tiles_c = tiles - tiles_a - tiles_b;
  s.b = CandShare{tiles_b ? tiles_a : 0u, tiles_b, tpw};
  s.c = CandShare{tiles_c ? tiles_a + tiles_b : 0u, tiles_c, 4};
  return s;
}

}  // namespace ratsdf
