// The workspace layout of the label scores, against points and against a mesh (score_layout, ra-slam_amd/csrc/
// workspace.h: one layout and one buffer for both host entry points), on the host alone: the score table of the host
// entry point (520 int64, a ratsdf_label_score) and its int64 count behind it.
//   * the size from a null-based cursor == where the cursor ends on a real base
//   * the table starts the buffer, holds 4160 bytes per item and is followed by the count on an 8-byte boundary
//   * the count's 16 bytes end the buffer
// usage: test_workspace_score_layout   (prints "workspace score layout OK" and returns 0, or names what failed)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "workspace.h"

using namespace ratsdf;

int main() {
  int failures = 0;
  for (size_t n : {(size_t)1, (size_t)2, (size_t)16}) {
    const size_t size = ws_bytes(score_layout, n);
    const size_t table = (4160 * n + 255) & ~(size_t)255;
    if (size != table + 16) ++failures, printf("FAILED n=%zu: %zu bytes, not %zu\n", n, size, table + 16);
    {
      WsCursor c{nullptr};
      ScoreWork w;
      score_layout(c, n, &w);
      if (w.score || w.count) ++failures, printf("FAILED n=%zu: pointers on a null base\n", n);
    }
    uint8_t* base = (uint8_t*)aligned_alloc(256, (size + 255) & ~(size_t)255);
    if (!base) return 2;
    WsCursor c{base};
    ScoreWork w;
    score_layout(c, n, &w);
    if (c.off != size) ++failures, printf("FAILED n=%zu: the cursor ends at %zu\n", n, c.off);
    if ((uint8_t*)w.score != base) ++failures, printf("FAILED n=%zu: the table does not start the buffer\n", n);
    if ((uint8_t*)w.count != base + table) ++failures, printf("FAILED n=%zu: the count is not behind the table\n", n);
    if (((uintptr_t)w.count & 7u) || ((uintptr_t)w.score & 255u)) ++failures, printf("FAILED n=%zu: alignment\n", n);
    memset(w.score, 1, 4160 * n);  // (a sanitizer build sees each part's extent inside the buffer)
    memset(w.count, 2, 16);
    if (((uint8_t*)w.score)[4160 * n - 1] != 1 || ((uint8_t*)w.count)[15] != 2) ++failures, printf("FAILED overlap\n");
    free(base);
  }
  if (failures) return 1;
  printf("workspace score layout OK: 3 sizes\n");
  return 0;
}
