// The workspace layout of the exposure read-out (exposure_layout, ra-slam_amd/csrc/workspace.h), on the host alone: the
// state bytes, the blocking bitmap, the lamps' voxels, the host form's lamp table and its summary.
//   * the size from a null-based cursor == the hand-written sum == where the cursor ends on a real base
//   * the states, the bitmap, the lamp voxels and the summary start 256-aligned; the table follows the lamp voxels after
//     1024 bytes (16-byte records: 16-aligned)
//   * the parts do not overlap and the summary block ends the buffer
//   * exposure_bricks_max(n) is no less than the 4 x 4 x 4 bricks of any box of n voxels (axes up to 1024), and it
//     never falls as n grows: a buffer laid out for its capacity holds every smaller box
// usage: test_workspace_exposure_layout   (prints "workspace exposure layout OK" and returns 0, or names what failed)
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
    const size_t pairs = 2 * n + 1 < ((size_t)3 << 20) ? 2 * n + 1 : (size_t)3 << 20;
    const size_t bricks = (n + 3 * pairs + 27675) / 64 + 1;
    const size_t want = up(n) + up(8 * bricks) + 1024 + 1024 + 256;
    const size_t size = ws_bytes(exposure_layout, n);
    if (size != want) ++failures, printf("FAILED n=%zu: %zu bytes, not %zu\n", n, size, want);
    if (exposure_bricks_max(n) != bricks) ++failures, printf("FAILED n=%zu: exposure_bricks_max\n", n);
    {
      WsCursor c{nullptr};
      ExposureWork w;
      exposure_layout(c, n, &w);
      if (w.st || w.bits || w.lamp_vox || w.table || w.summary) ++failures, printf("FAILED n=%zu: pointers on a null base\n", n);
    }
    uint8_t* base = (uint8_t*)aligned_alloc(256, up(size));
    if (!base) return 2;
    WsCursor c{base};
    ExposureWork w;
    exposure_layout(c, n, &w);
    if (c.off != size) ++failures, printf("FAILED n=%zu: the cursor ends at %zu\n", n, c.off);
    const uint8_t* part[5] = {(uint8_t*)w.st, (uint8_t*)w.bits, (uint8_t*)w.lamp_vox, (uint8_t*)w.table,
                              (uint8_t*)w.summary};
    const size_t bytes[5] = {n, 8 * bricks, 1024, 1024, 32};
    if (part[0] != base) ++failures, printf("FAILED n=%zu: the states do not start the buffer\n", n);
    for (int i = 0; i < 5; ++i) {
      if (i != 3 && ((uintptr_t)part[i] & 255u)) ++failures, printf("FAILED n=%zu: part %d is not 256-aligned\n", n, i);
      if (i + 1 < 5 && part[i] + bytes[i] > part[i + 1]) ++failures, printf("FAILED n=%zu: part %d overlaps\n", n, i);
    }
    if (part[3] != part[2] + 1024) ++failures, printf("FAILED n=%zu: the lamp table\n", n);
    if (part[4] + 256 != base + size) ++failures, printf("FAILED n=%zu: the summary block does not end the buffer\n", n);
    for (int i = 0; i < 5; ++i) memset((void*)part[i], i + 1, bytes[i]);  // (a sanitizer build sees each extent)
    for (int i = 0; i < 5; ++i)
      if (part[i][0] != i + 1 || part[i][bytes[i] - 1] != i + 1) ++failures, printf("FAILED n=%zu: part %d\n", n, i);
    free(base);
  }
  // the brick bound, on the axes where ceil() loses most and at the limits
  const int axes[] = {1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 63, 65, 100, 257, 511, 993, 1021, 1023, 1024};
  size_t boxes = 0;
  for (int X : axes)
    for (int Y : axes)
      for (int Z : axes) {
        const size_t n = (size_t)X * Y * Z;
        if (n > ((size_t)1 << 27)) continue;
        const size_t bricks = (size_t)((X + 3) / 4) * ((Y + 3) / 4) * ((Z + 3) / 4);
        if (bricks > exposure_bricks_max(n)) ++failures, printf("FAILED %d x %d x %d: %zu bricks\n", X, Y, Z, bricks);
        ++boxes;
      }
  size_t last = 0;
  for (size_t n = 1; n <= ((size_t)1 << 27); n += (n < 70000 ? 1 : 4099)) {
    const size_t b = exposure_bricks_max(n);
    if (b < last) ++failures, printf("FAILED n=%zu: the bound falls\n", n);
    last = b;
  }
  if (exposure_bricks_max((size_t)1 << 27) > ((size_t)1 << 22)) ++failures, printf("FAILED: the largest bitmap exceeds 32 MB\n");
  if (failures) return 1;
  printf("workspace exposure layout OK: 6 sizes, %zu boxes\n", boxes);
  return 0;
}
