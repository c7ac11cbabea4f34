// The look-ahead shares of the candidate pass (ra-slam_amd/csrc/cand_shares.h), on the host alone.
//
// Sweep: every super-tile count from 1 to 9216 as up to three images (one row of super-tiles, one column, the most
// square factorisation), each with ragged W and H (not multiples of 16), and the named sizes below; split_a in
// {0, 10, 50, 100}, split_b in {0, 30}, share B launched and not, 1 / 248 / 4096 look-ahead workgroups for B.
// For every combination:
//   * the shares are disjoint and together cover [0, tiles) exactly (A, B, C in this order, each possibly empty)
//   * B and C begin at multiples of 64 tiles (cand_pixel_work's XCD pairing goes by the workgroup's number in its share)
//   * tiles_per_wg is in 1 .. 16, and 4 for A and C (256-thread workgroups)
//   * a share that has no launch has no tiles: B when it is not launched; C when A and B were asked to take all of it
//     (one voxel per lane: k_integrate<1> hosts no look-ahead)
//   * at most the last non-empty share is ragged (implied by the above; stated on its own for the message)
//
// usage: test_cand_shares        (prints "cand shares OK: ..." and returns 0, or names what failed)
#include <cstdint>
#include <cstdio>
#include <vector>

#include "cand_shares.h"

using namespace ratsdf;

static long g_failures = 0;
static long g_first_supers = -1;
#define CHECK(cond, ...)                    \
  do {                                      \
    if (!(cond)) {                          \
      if (g_failures++ < 40) {              \
        printf("FAILED %s: ", #cond);       \
        printf(__VA_ARGS__);                \
        printf("\n");                       \
      }                                     \
    }                                       \
  } while (0)

struct Size {
  int W, H;
};

static long check(int W, int H, int sa, int sb, uint32_t wgs, bool b_launched) {
  const CandShares s = cand_shares(H, W, sa, sb, wgs, b_launched);
  const uint32_t tx = (uint32_t)((W + 15) / 16), ty = (uint32_t)((H + 15) / 16), tiles = tx * ty * 4;
  const long before = g_failures;
#define AT "%dx%d (%u super-tiles) split %d,%d B %s, %u wgs: A [%u +%u) B [%u +%u) x%u C [%u +%u)"
#define ARGS W, H, tx * ty, sa, sb, b_launched ? "launched" : "not launched", wgs, s.a.first_tile, s.a.n_tiles, \
             s.b.first_tile, s.b.n_tiles, s.b.tiles_per_wg, s.c.first_tile, s.c.n_tiles
  CHECK(s.tiles_x == tx && s.tiles == tiles, AT, ARGS);
  // disjoint, in order, covering [0, tiles): walk them
  uint64_t at = 0;
  const CandShare* sh[3] = {&s.a, &s.b, &s.c};
  int last_nonempty = -1;
  for (int i = 0; i < 3; ++i) {
    if (!sh[i]->n_tiles) continue;
    CHECK(sh[i]->first_tile == at, "share %c does not begin where the one before ends; " AT, "ABC"[i], ARGS);
    at = (uint64_t)sh[i]->first_tile + sh[i]->n_tiles;
    last_nonempty = i;
  }
  CHECK(at == tiles, "the shares cover %llu of %u tiles; " AT, (unsigned long long)at, tiles, ARGS);
  CHECK((uint64_t)s.a.n_tiles + s.b.n_tiles + s.c.n_tiles == tiles, AT, ARGS);
  CHECK(s.a.first_tile == 0, AT, ARGS);
  CHECK(s.b.first_tile % 64 == 0 && s.c.first_tile % 64 == 0, "B or C begins inside a group of 16 super-tiles; " AT, ARGS);
  for (int i = 0; i < 3; ++i)
    if (i != last_nonempty && sh[i]->n_tiles)
      CHECK(sh[i]->n_tiles % 64 == 0, "share %c is ragged and another follows; " AT, "ABC"[i], ARGS);
  CHECK(s.a.tiles_per_wg == 4 && s.c.tiles_per_wg == 4, AT, ARGS);
  CHECK(s.b.tiles_per_wg >= 1 && s.b.tiles_per_wg <= 16, AT, ARGS);
  // B's workgroups cover its tiles with what they may use (16 waves at most: then more workgroups than `wgs`)
  if (s.b.n_tiles && s.b.tiles_per_wg < 16)
    CHECK((uint64_t)s.b.tiles_per_wg * wgs >= s.b.n_tiles, AT, ARGS);
  CHECK(b_launched || s.b.n_tiles == 0, "share B has tiles and no launch; " AT, ARGS);
  if (sa + (b_launched ? sb : 0) >= 100) CHECK(s.c.n_tiles == 0, "share C has tiles though A and B take all; " AT, ARGS);
  if (sa == 0) CHECK(s.a.n_tiles == 0, AT, ARGS);
  // the percentages are kept to within a group of 16 super-tiles (the ragged end aside)
  if (sa < 100) CHECK((uint64_t)s.a.n_tiles <= (uint64_t)tiles * (unsigned)sa / 100, AT, ARGS);
  if (sa < 100 && tiles >= 64) CHECK((uint64_t)s.a.n_tiles + 64 > (uint64_t)tiles * (unsigned)sa / 100, AT, ARGS);
#undef AT
#undef ARGS
  if (g_failures != before && g_first_supers < 0) g_first_supers = (long)tx * ty;
  return g_failures - before;
}

int main() {
  std::vector<Size> sizes;
  const int kMaxSupers = 9216;
  for (int n = 1; n <= kMaxSupers; ++n) {
    // ragged edges: 1 .. 15 pixels short of the full super-tile, different in W and H, and full now and then
    const int cut_w = n % 16, cut_h = (n * 7 + 3) % 16;
    sizes.push_back(Size{16 * n - cut_w, 16 - cut_h});  // one row of super-tiles
    sizes.push_back(Size{16 - cut_h, 16 * n - cut_w});  // one column
    int f = 1;
    for (int d = 1; (long)d * d <= n; ++d)
      if (n % d == 0) f = d;
    if (f > 1) sizes.push_back(Size{16 * (n / f) - cut_w, 16 * f - cut_h});
  }
  const Size named[] = {{1, 1},      {15, 3},     {16, 4},     {17, 5},     {1, 300},     {300, 1},    {250, 157},
                        {353, 97},   {999, 600},  {1000, 600}, {1001, 601}, {1296, 968},  {1600, 1200}, {160, 120},
                        {640, 480},  {1280, 720}, {1920, 1080}, {64, 48},   {61, 83},     {3840, 2160}};
  for (const Size& z : named) sizes.push_back(z);
  const int split_a[] = {0, 10, 50, 100}, split_b[] = {0, 30};
  const uint32_t wgs[] = {1, 248, 4096};
  long combos = 0, failing_sizes = 0;
  for (const Size& z : sizes) {
    long bad = 0;
    for (int sa : split_a)
      for (int sb : split_b)
        for (int launched = 0; launched < 2; ++launched)
          for (uint32_t w : wgs) {
            bad += check(z.W, z.H, sa, sb, w, launched != 0);
            ++combos;
          }
    if (bad) ++failing_sizes;
  }
  if (g_failures) {
    printf("%ld checks failed at %ld of %zu sizes, first at %ld super-tiles\n", g_failures, failing_sizes, sizes.size(),
           g_first_supers);
    return 1;
  }
  printf("cand shares OK: %zu sizes up to %d super-tiles, %ld combinations\n", sizes.size(), kMaxSupers, combos);
  return 0;
}
