// surface.inc -- oriented surface points of a box of the map (include/ratsdf_surface.h): the host side of
// kernels_surface.h.  Included at the end of ratsdf_engine.hip.  Workspace: EngineMem::ws_surface (SurfaceWork,
// workspace.h), per cell of the box's block grid.

extern "C" {

static_assert(sizeof(ratsdf_surface_point) == 32 && offsetof(ratsdf_surface_point, prob) == 24,
              "ratsdf_surface_point layout");

// argument checks of both entry points (RATSDF_ERR_BAD_ARGUMENT when false); *ncells: cells of the box's block grid
static bool surface_box(const int32_t* origin, const int32_t* dims, const ratsdf_surface_params* p, MapBox* b,
                        size_t* ncells) {
  size_t n = 0;
  if (!p || p->min_weight < 1 || p->min_weight > 255 || std::isnan(p->min_prob) || p->flags || p->reserved ||
      !map_box(origin, dims, b, &n))
    return false;
  *ncells = box_cells(*b);
  return true;
}

// the count pass and the scan: points per cell, where each cell's points start, the total (no more than 3 * 2^27)
static int surface_count(ratsdf_engine* e, const MapBox& b, size_t ncells, const ratsdf_surface_params& p,
                         const SurfaceWork& w) {
  hipLaunchKernelGGL(k_surface<false>, dim3((unsigned)ncells), dim3(512), 0, e->stream, e->tab, e->pool, b,
                     (uint32_t)p.min_weight, p.min_prob, e->vs, w.cnt, (const uint32_t*)nullptr,
                     (const uint32_t*)nullptr, (uint4*)nullptr, 0ll, (long long*)nullptr);
  HIPCHK(hipGetLastError());
  return scan_counts(e, w.cnt, ncells, w.tiles, w.total, w.pos);
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
  STCHK(box_entry(e));
  SurfaceWork w;
  STCHK(e->workspace(e->ws_surface, ncells, surface_layout, &w));
  STCHK(surface_count(e, b, ncells, *params, w));
  return surface_emit(e, b, ncells, *params, w, d_points, capacity, d_count);
}

int ratsdf_surface_points(ratsdf_engine* e, const int32_t origin[3], const int32_t dims[3],
                          const ratsdf_surface_params* params, ratsdf_surface_point** out, size_t* n) {
  MapBox b;
  size_t ncells = 0;
  ENTRY(e, out && n && surface_box(origin, dims, params, &b, &ncells));
  STCHK(box_entry(e));
  SurfaceWork w;
  STCHK(e->workspace(e->ws_surface, ncells, surface_layout, &w));
  STCHK(surface_count(e, b, ncells, *params, w));
  uint32_t total = 0;
  STCHK(e->read_small(&total, w.total, 4));
  const HostPart part = {total, sizeof(ratsdf_surface_point), (void**)out, n};
  return hand_over(e, &part, 1, [&](uint8_t* const* d) {
    return surface_emit(e, b, ncells, *params, w, d[0], (int64_t)total, w.count);
  });
}

}  // extern "C"
