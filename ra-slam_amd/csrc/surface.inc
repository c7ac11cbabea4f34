// surface.inc -- oriented surface points of a box of the map (include/ratsdf_surface.h): the host side of
// kernels_surface.h.  Included at the end of ratsdf_engine.hip.

extern "C" {

static_assert(sizeof(ratsdf_surface_point) == 32 && offsetof(ratsdf_surface_point, prob) == 24,
              "ratsdf_surface_point layout");

// the workspace of a box of n cells of the block grid: points per cell (4n B) | where each cell's points start (4n B) |
// the scan's tile sums | the total (a word) and the host entry point's int64 count, 16 bytes together
struct SurfaceWork {
  uint32_t *cnt, *pos, *tiles, *total;
  long long* count;
};
static size_t surface_tiles(size_t n) { return (n + kScanTile - 1) / kScanTile; }
static size_t surface_work_bytes(size_t n) { return 2 * esdf_round(4 * n) + esdf_round(4 * surface_tiles(n)) + 16; }

// argument checks of both entry points (RATSDF_ERR_BAD_ARGUMENT when false); *ncells: cells of the box's block grid
static bool surface_box(const int32_t* origin, const int32_t* dims, const ratsdf_surface_params* p, MapBox* b,
                        size_t* ncells) {
  size_t n = 0;
  if (!p || p->min_weight < 1 || p->min_weight > 255 || std::isnan(p->min_prob) || p->flags || p->reserved ||
      !esdf_box(origin, dims, 0.f, 0u, b, &n))
    return false;
  *ncells = box_cells(*b);
  return true;
}

// a workspace for n cells (laid out for the number it was allocated for)
static int surface_workspace(ratsdf_engine* e, size_t n, SurfaceWork* w) {
  if (e->surface_cap < n) {
    HIPCHK(hipStreamSynchronize(e->stream));  // an earlier call may still be using the old one
    e->surface_cap = 0;
    STCHK(e->d_surface.alloc(surface_work_bytes(n)));
    e->surface_cap = n;
  }
  const size_t cap = e->surface_cap;
  uint8_t* p = e->d_surface.as<uint8_t>();
  w->cnt = (uint32_t*)p;
  w->pos = (uint32_t*)(p += esdf_round(4 * cap));
  w->tiles = (uint32_t*)(p += esdf_round(4 * cap));
  w->total = (uint32_t*)(p += esdf_round(4 * surface_tiles(cap)));
  w->count = (long long*)(p + 8);
  return RATSDF_OK;
}

// the count pass and the scan: points per cell, where each cell's points start, the total (no more than 3 * 2^27)
static int surface_count(ratsdf_engine* e, const MapBox& b, size_t ncells, const ratsdf_surface_params& p,
                         const SurfaceWork& w) {
  hipLaunchKernelGGL(k_surface<false>, dim3((unsigned)ncells), dim3(512), 0, e->stream, e->tab, e->pool, b,
                     (uint32_t)p.min_weight, p.min_prob, e->vs, w.cnt, (const uint32_t*)nullptr,
                     (const uint32_t*)nullptr, (uint4*)nullptr, 0ll, (long long*)nullptr);
  HIPCHK(hipGetLastError());
  const uint32_t ntiles = (uint32_t)surface_tiles(ncells);
  hipLaunchKernelGGL(k_mask_tile_sums, dim3(ntiles), dim3(1024), 0, e->stream, w.cnt, ncells, w.tiles);
  hipLaunchKernelGGL(k_scan_tile_sums, dim3(1), dim3(1024), 0, e->stream, w.tiles, ntiles, w.total);
  hipLaunchKernelGGL(k_mask_positions, dim3(ntiles), dim3(1024), 0, e->stream, w.cnt, ncells, w.tiles, w.pos);
  HIPCHK(hipGetLastError());
  return RATSDF_OK;
}

// the emit pass: the first min(total, capacity) points, and the total as an int64 at d_count
static int surface_emit(ratsdf_engine* e, const MapBox& b, size_t ncells, const ratsdf_surface_params& p,
                        const SurfaceWork& w, void* d_points, int64_t capacity, void* d_count) {
  hipLaunchKernelGGL(k_surface<true>, dim3((unsigned)ncells), dim3(512), 0, e->stream, e->tab, e->pool, b,
                     (uint32_t)p.min_weight, p.min_prob, e->vs, w.cnt, (const uint32_t*)w.pos,
                     (const uint32_t*)w.total, (uint4*)d_points, (long long)capacity, (long long*)d_count);
  HIPCHK(hipGetLastError());
  return RATSDF_OK;
}

int ratsdf_surface_points_device(ratsdf_engine* e, const int32_t origin[3], const int32_t dims[3],
                                 const ratsdf_surface_params* params, void* d_points, int64_t capacity,
                                 void* d_count) {
  MapBox b;
  size_t ncells = 0;
  ENTRY(e, capacity >= 0 && (d_points || capacity == 0) && !((uintptr_t)d_points & 15u) && d_count &&
               !((uintptr_t)d_count & 7u) && surface_box(origin, dims, params, &b, &ncells));
  STCHK(e->settle());
  STCHK(sticky_raised(e));
  SurfaceWork w;
  STCHK(surface_workspace(e, ncells, &w));
  STCHK(surface_count(e, b, ncells, *params, w));
  return surface_emit(e, b, ncells, *params, w, d_points, capacity, d_count);
}

int ratsdf_surface_points(ratsdf_engine* e, const int32_t origin[3], const int32_t dims[3],
                          const ratsdf_surface_params* params, ratsdf_surface_point** out, size_t* n) {
  MapBox b;
  size_t ncells = 0;
  ENTRY(e, out && n && surface_box(origin, dims, params, &b, &ncells));
  STCHK(e->settle());
  STCHK(sticky_raised(e));
  SurfaceWork w;
  STCHK(surface_workspace(e, ncells, &w));
  STCHK(surface_count(e, b, ncells, *params, w));
  uint32_t total = 0;
  STCHK(e->read_small(&total, w.total, 4));
  *out = nullptr;
  *n = 0;
  if (total == 0u) return e->sticky();
  const size_t bytes = (size_t)total * sizeof(ratsdf_surface_point);
  STCHK(e->staging(bytes, kHostChunk));
  void* host = malloc(bytes);
  if (!host) return RATSDF_ERR_DEVICE;  // (nothing is queued: read_small drained the stream)
  int st = surface_emit(e, b, ncells, *params, w, e->d_out.as<void>(), (int64_t)total, w.count);
  if (st == RATSDF_OK) st = e->download(host, e->d_out.as<void>(), bytes);
  if (st == RATSDF_OK) st = e->sticky();
  if (st != RATSDF_OK) {
    free(host);
    return st;
  }
  *out = (ratsdf_surface_point*)host;
  *n = total;
  return RATSDF_OK;
}

}  // extern "C"
