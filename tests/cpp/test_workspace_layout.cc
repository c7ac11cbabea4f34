// The workspace layouts of the box read-outs (ra-slam_amd/csrc/workspace.h), on the host alone: a layout function
// walked from a null base gives the size of the buffer, walked from a real base it carves the parts, and both must be
// what the four read-outs used to write out by hand, as a sum of bytes and again as a chain of pointer steps.
//
// For each of the four layouts and n = 1, 255, 256 (the rounding edge), 4095, 4096, 4097 (the scan-tile edge), 2^20:
//   * the size from a null-based cursor == where the cursor ends on a real base == the end of the last part
//   * every rounded part starts on a multiple of 256 bytes; no part reaches into the next one
//   * every part starts where the old pointer chain put it (the steps are written out below as they stood)
//   * the size == the closed form of the old *_work_bytes function, written out below as it stood
// Up to 64 MiB every part is also filled with its own byte and read back, so a sanitizer build sees each part's
// extent inside the buffer.
//
// usage: test_workspace_layout        (prints "workspace layout OK" and returns 0, or names what failed)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "workspace.h"

using namespace ratsdf;

static size_t old_round(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
static size_t old_tiles(size_t n) { return (n + 4096 - 1) / 4096; }
// the sums as they stood in esdf.inc, surface.inc, surface_mesh.inc and regions.inc
static size_t old_esdf_bytes(size_t n) { return old_round(n) + old_round(4 * n) + 3 * old_round(8 * n); }
static size_t old_surface_bytes(size_t n) { return 2 * old_round(4 * n) + old_round(4 * old_tiles(n)) + 16; }
static size_t old_surface_mesh_bytes(size_t n) {
  return 4 * old_round(4 * n) + old_round(4 * old_tiles(n)) + old_round(32) + 1024 * n;
}
static size_t old_regions_bytes(size_t n) {
  return old_round(n) + 2 * old_round(4 * n) + old_round(4 * old_tiles(n)) + 16;
}

struct Part {
  const char* name;
  const void* p;
  size_t bytes;  // what its users read and write
  size_t step;   // from its start to the start of the next part (to the end of the buffer for the last one)
  bool rounded;  // starts on a multiple of 256
};

static int g_failures = 0;
#define CHECK(cond, ...)            \
  do {                              \
    if (!(cond)) {                  \
      ++g_failures;                 \
      printf("FAILED %s: ", #cond); \
      printf(__VA_ARGS__);          \
      printf("\n");                 \
    }                               \
  } while (0)

template <class Work, class Parts>
static void check(const char* what, void (*layout)(WsCursor&, size_t, Work*), size_t n, size_t old_bytes,
                  Parts parts_of) {
  const size_t size = ws_bytes(layout, n);
  CHECK(size == old_bytes, "%s n=%zu: %zu bytes, %zu before", what, n, size, old_bytes);
  {  // (a cursor on a null base hands out null pointers, never null + offset)
    WsCursor c{nullptr};
    Work w;
    layout(c, n, &w);
    for (const Part& p : parts_of(w, n)) CHECK(p.p == nullptr, "%s n=%zu: %s on a null base", what, n, p.name);
  }
  uint8_t* base = (uint8_t*)aligned_alloc(256, old_round(size));
  CHECK(base != nullptr, "%s n=%zu: no memory for %zu bytes", what, n, size);
  if (!base) return;
  WsCursor c{base};
  Work w;
  layout(c, n, &w);
  CHECK(c.off == size, "%s n=%zu: the cursor ends at %zu, the size is %zu", what, n, c.off, size);
  const std::vector<Part> parts = parts_of(w, n);
  size_t expect = 0;  // where the old chain put this part
  for (const Part& p : parts) {
    const size_t at = (size_t)((const uint8_t*)p.p - base);
    CHECK(at == expect, "%s n=%zu: %s starts at %zu, %zu before", what, n, p.name, at, expect);
    CHECK(!p.rounded || at % 256 == 0, "%s n=%zu: %s starts at %zu, not a multiple of 256", what, n, p.name, at);
    CHECK(p.bytes <= p.step, "%s n=%zu: %s (%zu bytes) reaches into the next part, %zu on", what, n, p.name, p.bytes,
          p.step);
    expect = at + p.step;
  }
  CHECK(expect == size, "%s n=%zu: the last part ends at %zu, the size is %zu", what, n, expect, size);
  if (g_failures == 0 && size <= ((size_t)64 << 20)) {
    for (size_t i = 0; i < parts.size(); ++i) memset(const_cast<void*>(parts[i].p), (int)(i + 1), parts[i].bytes);
    for (size_t i = 0; i < parts.size(); ++i) {
      const uint8_t* q = (const uint8_t*)parts[i].p;
      CHECK(q[0] == i + 1 && q[parts[i].bytes - 1] == i + 1, "%s n=%zu: %s was overwritten", what, n, parts[i].name);
    }
  }
  free(base);
}

int main() {
  const size_t ns[] = {1, 255, 256, 4095, 4096, 4097, (size_t)1 << 20};
  for (size_t n : ns) {
    // w->gx = p += esdf_round(cap); w->gy = p += esdf_round(4 * cap); w->stk0 = p += esdf_round(8 * cap); ...
    check<EsdfWork>("esdf", esdf_layout, n, old_esdf_bytes(n), [](const EsdfWork& w, size_t n) {
      return std::vector<Part>{{"st", w.st, n, old_round(n), true},
                               {"gx", w.gx, 4 * n, old_round(4 * n), true},
                               {"gy", w.gy, 8 * n, old_round(8 * n), true},
                               {"stk0", w.stk0, 8 * n, old_round(8 * n), true},
                               {"stk1", w.stk1, 8 * n, old_round(8 * n), true}};
    });
    // ... w->total = p += esdf_round(4 * surface_tiles(cap)); w->count = p + 8;   (16 bytes)
    check<SurfaceWork>("surface", surface_layout, n, old_surface_bytes(n), [](const SurfaceWork& w, size_t n) {
      return std::vector<Part>{{"cnt", w.cnt, 4 * n, old_round(4 * n), true},
                               {"pos", w.pos, 4 * n, old_round(4 * n), true},
                               {"tiles", w.tiles, 4 * old_tiles(n), old_round(4 * old_tiles(n)), true},
                               {"total", w.total, 4, 8, true},
                               {"count", w.count, 8, 8, false}};
    });
    // ... w->total = p += esdf_round(4 * surface_tiles(cap)); w->counts = p + 8; w->code = p + esdf_round(32);
    check<SurfaceMeshWork>("surface_mesh", surface_mesh_layout, n, old_surface_mesh_bytes(n),
                           [](const SurfaceMeshWork& w, size_t n) {
                             return std::vector<Part>{
                                 {"cnt_v", w.cnt_v, 4 * n, old_round(4 * n), true},
                                 {"cnt_t", w.cnt_t, 4 * n, old_round(4 * n), true},
                                 {"pos_v", w.pos_v, 4 * n, old_round(4 * n), true},
                                 {"pos_t", w.pos_t, 4 * n, old_round(4 * n), true},
                                 {"tiles", w.tiles, 4 * old_tiles(n), old_round(4 * old_tiles(n)), true},
                                 {"total", w.total, 8, 8, true},
                                 {"counts", w.counts, 16, old_round(32) - 8, false},
                                 {"code", w.code, 1024 * n, 1024 * n, true}};
                           });
    // w->lab = p += esdf_round(cap); w->rank = p += esdf_round(4 * cap); w->tiles = p += esdf_round(4 * cap); ...
    check<RegionsWork>("regions", regions_layout, n, old_regions_bytes(n), [](const RegionsWork& w, size_t n) {
      return std::vector<Part>{{"st", w.st, n, old_round(n), true},
                               {"lab", w.lab, 4 * n, old_round(4 * n), true},
                               {"rank", w.rank, 4 * n, old_round(4 * n), true},
                               {"tiles", w.tiles, 4 * old_tiles(n), old_round(4 * old_tiles(n)), true},
                               {"total", w.total, 4, 8, true},
                               {"count", w.count, 8, 8, false}};
    });
  }
  CHECK(ws_round(0) == 0 && ws_round(1) == 256 && ws_round(256) == 256 && ws_round(257) == 512, "ws_round");
  CHECK(scan_tiles(0) == 0 && scan_tiles(1) == 1 && scan_tiles(4096) == 1 && scan_tiles(4097) == 2, "scan_tiles");
  if (g_failures) return 1;
  printf("workspace layout OK: 4 layouts x %zu sizes\n", sizeof(ns) / sizeof(ns[0]));
  return 0;
}
