// The workspace layout of the cost-to-go field (cost_layout, ra-slam_amd/csrc/workspace.h), on the host alone: an ESDF
// workspace of its own, the traversable bytes, the two dirty arrays, and the summary with the two dirty counts.
//   * the size from a null-based cursor == the hand-written sum == where the cursor ends on a real base
//   * the ESDF parts are esdf_layout's, at the buffer's start; esdf_layout itself measures what it did
//   * every part starts 256-aligned except the counts, which follow the summary after 32 bytes
//   * the parts do not overlap and the summary block ends the buffer
//   * cost_tiles_max(n) is no less than the 32 x 8 x 4 tiles of any box of n voxels (axes up to 1024)
// usage: test_workspace_cost_layout   (prints "workspace cost layout OK" and returns 0, or names what failed)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "workspace.h"

using namespace ratsdf;

static size_t up(size_t b) { return (b + 255) & ~(size_t)255; }

int main() {
  int failures = 0;
  for (size_t n : {(size_t)1, (size_t)255, (size_t)256, (size_t)2160, (size_t)12600, (size_t)294912}) {
    const size_t tiles = n / 16 + 420;
    const size_t esdf = up(n) + up(4 * n) + 3 * up(8 * n);
    const size_t want = esdf + up(n) + up(8 * tiles) + 256;
    const size_t size = ws_bytes(cost_layout, n);
    if (size != want) ++failures, printf("FAILED n=%zu: %zu bytes, not %zu\n", n, size, want);
    if (ws_bytes(esdf_layout, n) != esdf) ++failures, printf("FAILED n=%zu: esdf_layout moved\n", n);
    if (cost_tiles_max(n) != tiles) ++failures, printf("FAILED n=%zu: cost_tiles_max\n", n);
    {
      WsCursor c{nullptr};
      CostWork w;
      cost_layout(c, n, &w);
      if (w.esdf.st || w.trav || w.dirty || w.summary || w.counts) ++failures, printf("FAILED n=%zu: pointers on a null base\n", n);
    }
    uint8_t* base = (uint8_t*)aligned_alloc(256, up(size));
    if (!base) return 2;
    WsCursor c{base};
    CostWork w;
    cost_layout(c, n, &w);
    if (c.off != size) ++failures, printf("FAILED n=%zu: the cursor ends at %zu\n", n, c.off);
    WsCursor ce{base};
    EsdfWork we;
    esdf_layout(ce, n, &we);
    if (we.st != w.esdf.st || we.gx != w.esdf.gx || we.gy != w.esdf.gy || we.stk0 != w.esdf.stk0 ||
        we.stk1 != w.esdf.stk1 || (uint8_t*)w.trav != base + ce.off)
      ++failures, printf("FAILED n=%zu: the ESDF parts are not esdf_layout's\n", n);
    const uint8_t* part[9] = {(uint8_t*)w.esdf.st,   (uint8_t*)w.esdf.gx, (uint8_t*)w.esdf.gy,
                              (uint8_t*)w.esdf.stk0, (uint8_t*)w.esdf.stk1, (uint8_t*)w.trav,
                              (uint8_t*)w.dirty,     (uint8_t*)w.summary,  (uint8_t*)w.counts};
    const size_t bytes[9] = {n, 4 * n, 8 * n, 8 * n, 8 * n, n, 8 * tiles, 32, 8};
    if (part[0] != base) ++failures, printf("FAILED n=%zu: the states do not start the buffer\n", n);
    for (int i = 0; i < 9; ++i) {
      if (i != 8 && ((uintptr_t)part[i] & 255u)) ++failures, printf("FAILED n=%zu: part %d is not 256-aligned\n", n, i);
      if (i + 1 < 9 && part[i] + bytes[i] > part[i + 1]) ++failures, printf("FAILED n=%zu: part %d overlaps\n", n, i);
    }
    if (part[8] != part[7] + 32) ++failures, printf("FAILED n=%zu: the dirty counts\n", n);
    if (part[7] + 256 != base + size) ++failures, printf("FAILED n=%zu: the summary block does not end the buffer\n", n);
    for (int i = 0; i < 9; ++i) memset((void*)part[i], i + 1, bytes[i]);  // (a sanitizer build sees each extent)
    for (int i = 0; i < 9; ++i)
      if (part[i][0] != i + 1 || part[i][bytes[i] - 1] != i + 1) ++failures, printf("FAILED n=%zu: part %d\n", n, i);
    free(base);
  }
  // the tile bound, on the axes where ceil() loses most and at the limits
  const int axes[] = {1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 63, 65, 100, 257, 511, 993, 1023, 1024};
  size_t boxes = 0;
  for (int X : axes)
    for (int Y : axes)
      for (int Z : axes) {
        const size_t n = (size_t)X * Y * Z;
        if (n > ((size_t)1 << 27)) continue;
        const size_t tiles = (size_t)((X + 31) / 32) * ((Y + 7) / 8) * ((Z + 3) / 4);
        if (tiles > cost_tiles_max(n)) ++failures, printf("FAILED %d x %d x %d: %zu tiles\n", X, Y, Z, tiles);
        ++boxes;
      }
  if (failures) return 1;
  printf("workspace cost layout OK: 6 sizes, %zu boxes\n", boxes);
  return 0;
}
