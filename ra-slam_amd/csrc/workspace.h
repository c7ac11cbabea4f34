// workspace.h -- how the box read-outs (esdf.inc, surface.inc, surface_mesh.inc, regions.inc, cost.inc, exposure.inc) and the label
// scores (score.inc) carve their device workspaces: a cursor that walks a buffer part by part, and one layout function per read-out that fills its *Work
// struct from a cursor.  Walked from a null base the same function yields the buffer's size (ws_bytes), so a layout is
// written once and cannot disagree with the allocation.  Plain C++, no HIP types: tests/cpp/test_workspace_layout.cc
// compiles it alone.  ratsdf_engine::workspace (ratsdf_engine.hip) owns the buffers and their grow step.
#pragma once
#include <cstddef>
#include <cstdint>

namespace ratsdf {

inline size_t ws_round(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

constexpr size_t kWsScanTile = 4096;  // kScanTile of kernels_mesh.h (ratsdf_engine.hip asserts it)
inline size_t scan_tiles(size_t n) { return (n + kWsScanTile - 1) / kWsScanTile; }  // tile sums of a scan over n items

struct WsCursor {
  uint8_t* base;  // null: nothing is carved, only measured
  size_t off = 0;
  // the current position as a T*, then on by exactly `bytes` ...
  template <class T>
  T* take_raw(size_t bytes) {
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += bytes;
    return p;
  }
  // ... or by ws_round(bytes): the next part starts 256-aligned again
  template <class T>
  T* take(size_t bytes) {
    return take_raw<T>(ws_round(bytes));
  }
};

// the bytes of a layout for n items
template <class Work>
size_t ws_bytes(void (*layout)(WsCursor&, size_t, Work*), size_t n) {
  WsCursor c{nullptr};
  Work w;
  layout(c, n, &w);
  return c.off;
}

// The layouts.  Offsets and sizes are, for every n, those of the hand-written sums and pointer chains they replace
// (the test pins the sums): the alignment the kernels see and the memory footprint are unchanged.

// ESDF, a box of n voxels: state (n B) | x pass (4n B; the host entry point's field after the z pass) | y pass (8n B) |
// stack of the transform to O (8n B) | stack of the transform to box \ O (8n B); the 8-byte records are uint2
struct EsdfWork {
  uint8_t* st;
  uint32_t* gx;
  uint64_t *gy, *stk0, *stk1;
};
inline void esdf_layout(WsCursor& c, size_t n, EsdfWork* w) {  // (offsets and size as before, see above)
  w->st = c.take<uint8_t>(n);
  w->gx = c.take<uint32_t>(4 * n);
  w->gy = c.take<uint64_t>(8 * n);
  w->stk0 = c.take<uint64_t>(8 * n);
  w->stk1 = c.take<uint64_t>(8 * n);
}

// surface points, a box of n cells of the block grid: points per cell (4n B) | where each cell's points start (4n B) |
// the scan's tile sums | the total (a word) and the host entry point's int64 count, 16 bytes together
struct SurfaceWork {
  uint32_t *cnt, *pos, *tiles, *total;
  long long* count;
};
inline void surface_layout(WsCursor& c, size_t n, SurfaceWork* w) {  // (offsets and size as before, see above)
  w->cnt = c.take<uint32_t>(4 * n);
  w->pos = c.take<uint32_t>(4 * n);
  w->tiles = c.take<uint32_t>(4 * scan_tiles(n));
  w->total = c.take_raw<uint32_t>(8);
  w->count = c.take_raw<long long>(8);
}

// welded mesh, a grid of n block cells: vertices per cell | triangles per cell | where each cell's vertices start |
// where its triangles start (4n B each) | the scan's tile sums | the two totals (words) and the host entry point's two
// int64 counts, a rounded 32 bytes together | the vertex codes, 512 halfwords per cell
struct SurfaceMeshWork {
  uint32_t *cnt_v, *cnt_t, *pos_v, *pos_t, *tiles, *total;
  long long* counts;
  uint16_t* code;
};
inline void surface_mesh_layout(WsCursor& c, size_t n, SurfaceMeshWork* w) {  // (offsets and size as before, see above)
  w->cnt_v = c.take<uint32_t>(4 * n);
  w->cnt_t = c.take<uint32_t>(4 * n);
  w->pos_v = c.take<uint32_t>(4 * n);
  w->pos_t = c.take<uint32_t>(4 * n);
  w->tiles = c.take<uint32_t>(4 * scan_tiles(n));
  w->total = c.take_raw<uint32_t>(8);
  w->counts = c.take_raw<long long>(ws_round(32) - 8);
  w->code = c.take_raw<uint16_t>(1024 * n);
}

// clustered mesh (cluster_mesh.inc), a grid of n block cells, a buffer of its own: clusters per cell | triangles per
// cell | where each cell's clusters start | where its triangles start (4n B each) | the scan's tile sums | the two totals
// (words) and the host entry point's two int64 counts, a rounded 32 bytes together | the 64-bit mask of each cell's
// non-empty clusters (8n B)
struct ClusterMeshWork {
  uint32_t *cnt_v, *cnt_t, *pos_v, *pos_t, *tiles, *total;
  long long* counts;
  unsigned long long* mask;
};
inline void cluster_mesh_layout(WsCursor& c, size_t n, ClusterMeshWork* w) {
  w->cnt_v = c.take<uint32_t>(4 * n);
  w->cnt_t = c.take<uint32_t>(4 * n);
  w->pos_v = c.take<uint32_t>(4 * n);
  w->pos_t = c.take<uint32_t>(4 * n);
  w->tiles = c.take<uint32_t>(4 * scan_tiles(n));
  w->total = c.take_raw<uint32_t>(8);
  w->counts = c.take_raw<long long>(ws_round(32) - 8);
  w->mask = c.take<unsigned long long>(8 * n);
}

// regions, a box of n voxels: seed bytes (n B) | labels (4n B) | root flags, then ranks in place (4n B) | the scan's
// tile sums | the number of regions (a word) and the host entry point's int64 count, 16 bytes together
struct RegionsWork {
  uint8_t* st;
  int32_t* lab;
  uint32_t *rank, *tiles, *total;
  long long* count;
};
inline void regions_layout(WsCursor& c, size_t n, RegionsWork* w) {  // (offsets and size as before, see above)
  w->st = c.take<uint8_t>(n);
  w->lab = c.take<int32_t>(4 * n);
  w->rank = c.take<uint32_t>(4 * n);
  w->tiles = c.take<uint32_t>(4 * scan_tiles(n));
  w->total = c.take_raw<uint32_t>(8);
  w->count = c.take_raw<long long>(8);
}

// cost to go (cost.inc), a box of n voxels, a buffer of its own: an ESDF workspace of its own (esdf_layout, from the
// same cursor: state and field of the box) | traversable bytes (n B) | the dirty flags of the tiles, two arrays by round
// parity (4 B a tile each) | the host entry point's summary (32 B), then the two dirty counts: a rounded 256 bytes.
// cost_tiles_max(n): no box of n voxels has more 32 x 8 x 4 tiles -- ceil(X/32) ceil(Y/8) ceil(Z/4) <=
// (X/32 + 1)(Y/8 + 1)(Z/4 + 1) <= n (1 + 4 + 8 + 32) / 1024 + 1024 (1/32 + 1/8 + 1/4) + 1, every axis being <= 1024
// and every product of two axes <= n.
inline size_t cost_tiles_max(size_t n) { return n / 16 + 420; }
struct CostWork {
  EsdfWork esdf;
  uint8_t* trav;
  uint32_t *dirty, *summary, *counts;
};
inline void cost_layout(WsCursor& c, size_t n, CostWork* w) {
  esdf_layout(c, n, &w->esdf);
  w->trav = c.take<uint8_t>(n);
  w->dirty = c.take<uint32_t>(8 * cost_tiles_max(n));
  w->summary = c.take_raw<uint32_t>(32);
  w->counts = c.take_raw<uint32_t>(ws_round(40) - 32);
}

// exposure (exposure.inc), a box of n voxels, a buffer of its own: state bytes (n B) | the blocking bitmap, a 64-bit
// word per 4 x 4 x 4 brick | the lamps' voxels and acceptance (64 x 16 B) | the host entry point's lamp table
// (64 x 16 B) | its summary (32 B), rounded.
// exposure_bricks_max(n): no box of n voxels has more bricks -- ceil(X/4) ceil(Y/4) ceil(Z/4) <= (X+3)(Y+3)(Z+3) / 64 =
// (n + 3 (XY + YZ + XZ) + 9 (X + Y + Z) + 27) / 64, where each pair product is <= n and <= 2^20 (every axis <= 1024),
// their sum <= 2n + 1 (at its largest when two axes are 1) and X + Y + Z <= 3072.  Monotonic in n: a layout for the
// buffer's capacity holds every smaller box.
inline size_t exposure_bricks_max(size_t n) {
  const size_t pairs = 2 * n + 1 < ((size_t)3 << 20) ? 2 * n + 1 : (size_t)3 << 20;
  return (n + 3 * pairs + 9 * 3072 + 27) / 64 + 1;
}
struct ExposureWork {
  uint8_t* st;
  unsigned long long* bits;
  int32_t* lamp_vox;
  uint32_t *table, *summary;
};
inline void exposure_layout(WsCursor& c, size_t n, ExposureWork* w) {
  w->st = c.take<uint8_t>(n);
  w->bits = c.take<unsigned long long>(8 * exposure_bricks_max(n));
  w->lamp_vox = c.take_raw<int32_t>(1024);
  w->table = c.take_raw<uint32_t>(1024);
  w->summary = c.take<uint32_t>(32);
}

// label score against points and against a mesh (score_host in score.inc serves both, from one buffer), n = 1: the
// score table of the host entry point (520 int64) | its int64 count, 16 bytes
struct ScoreWork {
  long long *score, *count;
};
inline void score_layout(WsCursor& c, size_t n, ScoreWork* w) {
  w->score = c.take<long long>(4160 * n);
  w->count = c.take_raw<long long>(16);
}

}  // namespace ratsdf
