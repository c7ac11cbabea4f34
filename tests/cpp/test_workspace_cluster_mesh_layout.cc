// The workspace layout of the clustered mesh (cluster_mesh_layout, ra-slam_amd/csrc/workspace.h), on the host alone:
// four words per cell of the block grid, the scan's tile sums, the two totals with the host entry point's two int64
// counts, and the 64-bit cluster mask per cell.
//   * the size from a null-based cursor == where the cursor ends on a real base
//   * every part starts 256-aligned except the counts, which follow the totals after 8 bytes on an 8-byte boundary
//   * the parts do not overlap and the masks end the buffer
//   * surface_mesh_layout beside it measures what the hand-written sum gives
// usage: test_workspace_cluster_mesh_layout   (prints "workspace cluster mesh layout OK" and returns 0, or names what
// failed)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "workspace.h"

using namespace ratsdf;

static size_t up(size_t b) { return (b + 255) & ~(size_t)255; }

int main() {
  int failures = 0;
  for (size_t n : {(size_t)1, (size_t)63, (size_t)64, (size_t)4096, (size_t)4097, (size_t)5832}) {
    const size_t tiles = (n + 4095) / 4096;
    const size_t want = 4 * up(4 * n) + up(4 * tiles) + 256 + up(8 * n);
    const size_t size = ws_bytes(cluster_mesh_layout, n);
    if (size != want) ++failures, printf("FAILED n=%zu: %zu bytes, not %zu\n", n, size, want);
    if (ws_bytes(surface_mesh_layout, n) != 4 * up(4 * n) + up(4 * tiles) + 256 + 1024 * n)
      ++failures, printf("FAILED n=%zu: surface_mesh_layout moved\n", n);
    {
      WsCursor c{nullptr};
      ClusterMeshWork w;
      cluster_mesh_layout(c, n, &w);
      if (w.cnt_v || w.mask || w.counts) ++failures, printf("FAILED n=%zu: pointers on a null base\n", n);
    }
    uint8_t* base = (uint8_t*)aligned_alloc(256, up(size));
    if (!base) return 2;
    WsCursor c{base};
    ClusterMeshWork w;
    cluster_mesh_layout(c, n, &w);
    if (c.off != size) ++failures, printf("FAILED n=%zu: the cursor ends at %zu\n", n, c.off);
    const uint8_t* part[8] = {(uint8_t*)w.cnt_v, (uint8_t*)w.cnt_t, (uint8_t*)w.pos_v,  (uint8_t*)w.pos_t,
                              (uint8_t*)w.tiles, (uint8_t*)w.total, (uint8_t*)w.counts, (uint8_t*)w.mask};
    const size_t bytes[8] = {4 * n, 4 * n, 4 * n, 4 * n, 4 * tiles, 8, 16, 8 * n};
    if (part[0] != base) ++failures, printf("FAILED n=%zu: the counts do not start the buffer\n", n);
    for (int i = 0; i < 8; ++i) {
      if (i != 6 && ((uintptr_t)part[i] & 255u)) ++failures, printf("FAILED n=%zu: part %d is not 256-aligned\n", n, i);
      if (i + 1 < 8 && part[i] + bytes[i] > part[i + 1]) ++failures, printf("FAILED n=%zu: part %d overlaps\n", n, i);
    }
    if (part[6] != part[5] + 8 || ((uintptr_t)part[6] & 7u)) ++failures, printf("FAILED n=%zu: the int64 counts\n", n);
    if (part[7] + up(8 * n) != base + size) ++failures, printf("FAILED n=%zu: the masks do not end the buffer\n", n);
    for (int i = 0; i < 8; ++i) memset((void*)part[i], i + 1, bytes[i]);  // (a sanitizer build sees each extent)
    for (int i = 0; i < 8; ++i)
      if (part[i][0] != i + 1 || part[i][bytes[i] - 1] != i + 1) ++failures, printf("FAILED n=%zu: part %d\n", n, i);
    free(base);
  }
  if (failures) return 1;
  printf("workspace cluster mesh layout OK: 6 sizes\n");
  return 0;
}
