// surface_mesh.inc -- welded triangle mesh of a box of the map (include/ratsdf_surface_mesh.h): the host side of
// kernels_surface_mesh.h.  Included at the end of ratsdf_engine.hip.  Workspace: EngineMem::ws_surface_mesh
// (SurfaceMeshWork, workspace.h), per cell of the block grid.

extern "C" {

// argument checks of both entry points (RATSDF_ERR_BAD_ARGUMENT when false).  The block grid is that of the vertex
// owners, the voxels [origin, origin + dims] clipped to the int16 range: up to one block more per axis than the box
// meets; *ncells: its cells
static bool surface_mesh_box(const int32_t* origin, const int32_t* dims, const ratsdf_surface_mesh_params* p,
                             MapBox* b, size_t* ncells) {
  size_t n = 0;
  if (!p || p->min_weight < 1 || p->min_weight > 255 || p->flags || p->reserved0 || p->reserved1 ||
      !map_box(origin, dims, b, &n))
    return false;
  b->nbx = (std::min(b->ox + b->X, 32767) >> 3) - b->bx0 + 1;
  b->nby = (std::min(b->oy + b->Y, 32767) >> 3) - b->by0 + 1;
  b->nbz = (std::min(b->oz + b->Z, 32767) >> 3) - b->bz0 + 1;
  *ncells = box_cells(*b);
  return true;
}

// the case tables, built on first use
static int surface_mesh_tables(ratsdf_engine* e) {
  if (e->d_surface_mesh_tab) return RATSDF_OK;
  const SurfaceMeshTables h = make_surface_mesh_tables();
  DevMem t;  // (the engine keeps tables that have arrived, nothing else)
  STCHK(t.alloc(sizeof(SurfaceMeshTables)));
  HIPCHK(hipMemcpy(t.as<void>(), &h, sizeof(SurfaceMeshTables), hipMemcpyHostToDevice));
  e->d_surface_mesh_tab = std::move(t);
  return RATSDF_OK;
}

// the count pass and the two scans: vertices and triangles per cell, where each cell's start, the totals (no more than
// 3 * 1025^3 / 8 and 5 * 2^27: both fit a word, and every vertex index an int32)
static int surface_mesh_count(ratsdf_engine* e, const MapBox& b, size_t ncells, const ratsdf_surface_mesh_params& p,
                              const SurfaceMeshWork& w) {
  hipLaunchKernelGGL(k_surface_mesh<false>, dim3((unsigned)ncells), dim3(512), 0, e->stream, e->tab, e->pool, b,
                     (uint32_t)p.min_weight, e->vs, e->d_surface_mesh_tab.as<const SurfaceMeshTables>(), w.cnt_v,
                     w.cnt_t, w.code, (const uint32_t*)nullptr, (const uint32_t*)nullptr, (const uint32_t*)nullptr,
                     (uint4*)nullptr, 0ll, (int32_t*)nullptr, 0ll, (long long*)nullptr);
  HIPCHK(hipGetLastError());
  // (the tile sums of the first scan are dead when the second one starts: one stream)
  STCHK(scan_counts(e, w.cnt_v, ncells, w.tiles, w.total, w.pos_v));
  return scan_counts(e, w.cnt_t, ncells, w.tiles, w.total + 1, w.pos_t);
}

// the emit pass: the first min(total, capacity) records of either list, and the totals as two int64 at d_counts
static int surface_mesh_emit(ratsdf_engine* e, const MapBox& b, size_t ncells, const ratsdf_surface_mesh_params& p,
                             const SurfaceMeshWork& w, void* d_vertices, int64_t vcap, void* d_triangles,
                             int64_t tcap, void* d_counts) {
  hipLaunchKernelGGL(k_surface_mesh<true>, dim3((unsigned)ncells), dim3(512), 0, e->stream, e->tab, e->pool, b,
                     (uint32_t)p.min_weight, e->vs, e->d_surface_mesh_tab.as<const SurfaceMeshTables>(), w.cnt_v,
                     w.cnt_t, w.code, (const uint32_t*)w.pos_v, (const uint32_t*)w.pos_t, (const uint32_t*)w.total,
                     (uint4*)d_vertices, (long long)vcap, (int32_t*)d_triangles, (long long)tcap,
                     (long long*)d_counts);
  HIPCHK(hipGetLastError());
  return RATSDF_OK;
}

int ratsdf_surface_mesh_device(ratsdf_engine* e, const int32_t origin[3], const int32_t dims[3],
                               const ratsdf_surface_mesh_params* params, void* d_vertices, int64_t vertex_capacity,
                               void* d_triangles, int64_t triangle_capacity, void* d_counts) {
  MapBox b;
  size_t ncells = 0;
  ENTRY(e, vertex_capacity >= 0 && (d_vertices || vertex_capacity == 0) && !((uintptr_t)d_vertices & 15u) &&
               triangle_capacity >= 0 && (d_triangles || triangle_capacity == 0) && !((uintptr_t)d_triangles & 3u) &&
               d_counts && !((uintptr_t)d_counts & 7u) && surface_mesh_box(origin, dims, params, &b, &ncells));
  STCHK(box_entry(e));
  STCHK(surface_mesh_tables(e));
  SurfaceMeshWork w;
  STCHK(e->workspace(e->ws_surface_mesh, ncells, surface_mesh_layout, &w));
  STCHK(surface_mesh_count(e, b, ncells, *params, w));
  return surface_mesh_emit(e, b, ncells, *params, w, d_vertices, vertex_capacity, d_triangles, triangle_capacity,
                           d_counts);
}

int ratsdf_surface_mesh(ratsdf_engine* e, const int32_t origin[3], const int32_t dims[3],
                        const ratsdf_surface_mesh_params* params, ratsdf_surface_point** vertices,
                        size_t* n_vertices, int32_t** triangles, size_t* n_triangles) {
  MapBox b;
  size_t ncells = 0;
  ENTRY(e, vertices && n_vertices && triangles && n_triangles && surface_mesh_box(origin, dims, params, &b, &ncells));
  STCHK(box_entry(e));
  STCHK(surface_mesh_tables(e));
  SurfaceMeshWork w;
  STCHK(e->workspace(e->ws_surface_mesh, ncells, surface_mesh_layout, &w));
  STCHK(surface_mesh_count(e, b, ncells, *params, w));
  uint32_t total[2] = {0, 0};
  STCHK(e->read_small(total, w.total, 8));
  // (one total is zero iff the other is)
  const HostPart parts[2] = {{total[0], sizeof(ratsdf_surface_point), (void**)vertices, n_vertices},
                             {total[1], 12, (void**)triangles, n_triangles}};
  return hand_over(e, parts, 2, [&](uint8_t* const* d) {
    return surface_mesh_emit(e, b, ncells, *params, w, d[0], (int64_t)total[0], d[1], (int64_t)total[1], w.counts);
  });
}

}  // extern "C"
