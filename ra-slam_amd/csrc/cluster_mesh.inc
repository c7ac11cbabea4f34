// cluster_mesh.inc -- clustered mesh of a box of the map (include/ratsdf_cluster_mesh.h): the host side of
// kernels_cluster_mesh.h.  Included at the end of ratsdf_engine.hip, after surface_mesh.inc (whose box and case tables
// it shares).  Workspace: EngineMem::ws_cluster_mesh (ClusterMeshWork, workspace.h), per cell of the block grid.

extern "C" {

// argument checks of both entry points (RATSDF_ERR_BAD_ARGUMENT when false): the box and its block grid are the welded
// mesh's (surface_mesh_box: every chosen endpoint is a vertex owner's voxel or the next one, inside the same grid);
// *s: log2 of the factor
static bool cluster_mesh_box(const int32_t* origin, const int32_t* dims, const ratsdf_cluster_mesh_params* p, MapBox* b,
                             size_t* ncells, int* s) {
  if (!p || p->flags || p->reserved || (p->factor != 2 && p->factor != 4 && p->factor != 8)) return false;
  const ratsdf_surface_mesh_params sp = {p->min_weight, 0u, 0u, 0u};
  *s = p->factor == 2 ? 1 : p->factor == 4 ? 2 : 3;
  return surface_mesh_box(origin, dims, &sp, b, ncells);
}

// the count pass and the two scans: clusters and triangles per cell, where each cell's start, the totals (no more than
// the welded mesh's: both fit a word, and every vertex index an int32)
static int cluster_mesh_count(ratsdf_engine* e, const MapBox& b, size_t ncells, const ratsdf_cluster_mesh_params& p,
                              int s, const ClusterMeshWork& w) {
  hipLaunchKernelGGL(k_cluster_mesh<false>, dim3((unsigned)ncells), dim3(512), 0, e->stream, e->tab, e->pool, b,
                     (uint32_t)p.min_weight, e->vs, s, e->d_surface_mesh_tab.as<const SurfaceMeshTables>(), w.cnt_v,
                     w.cnt_t, w.mask, (const uint32_t*)nullptr, (const uint32_t*)nullptr, (const uint32_t*)nullptr,
                     (uint4*)nullptr, 0ll, (int32_t*)nullptr, 0ll, (long long*)nullptr);
  HIPCHK(hipGetLastError());
  // (the tile sums of the first scan are dead when the second one starts: one stream)
  STCHK(scan_counts(e, w.cnt_v, ncells, w.tiles, w.total, w.pos_v));
  return scan_counts(e, w.cnt_t, ncells, w.tiles, w.total + 1, w.pos_t);
}

// the emit pass: the first min(total, capacity) records of either list, and the totals as two int64 at d_counts
static int cluster_mesh_emit(ratsdf_engine* e, const MapBox& b, size_t ncells, const ratsdf_cluster_mesh_params& p,
                             int s, const ClusterMeshWork& w, void* d_vertices, int64_t vcap, void* d_triangles,
                             int64_t tcap, void* d_counts) {
  hipLaunchKernelGGL(k_cluster_mesh<true>, dim3((unsigned)ncells), dim3(512), 0, e->stream, e->tab, e->pool, b,
                     (uint32_t)p.min_weight, e->vs, s, e->d_surface_mesh_tab.as<const SurfaceMeshTables>(), w.cnt_v,
                     w.cnt_t, w.mask, (const uint32_t*)w.pos_v, (const uint32_t*)w.pos_t, (const uint32_t*)w.total,
                     (uint4*)d_vertices, (long long)vcap, (int32_t*)d_triangles, (long long)tcap,
                     (long long*)d_counts);
  HIPCHK(hipGetLastError());
  return RATSDF_OK;
}

int ratsdf_cluster_mesh_device(ratsdf_engine* e, const int32_t origin[3], const int32_t dims[3],
                               const ratsdf_cluster_mesh_params* params, void* d_vertices, int64_t vertex_capacity,
                               void* d_triangles, int64_t triangle_capacity, void* d_counts) {
  MapBox b;
  size_t ncells = 0;
  int s = 0;
  ENTRY(e, vertex_capacity >= 0 && (d_vertices || vertex_capacity == 0) && !((uintptr_t)d_vertices & 15u) &&
               triangle_capacity >= 0 && (d_triangles || triangle_capacity == 0) && !((uintptr_t)d_triangles & 3u) &&
               d_counts && !((uintptr_t)d_counts & 7u) && cluster_mesh_box(origin, dims, params, &b, &ncells, &s));
  STCHK(box_entry(e));
  STCHK(surface_mesh_tables(e));
  ClusterMeshWork w;
  STCHK(e->workspace(e->ws_cluster_mesh, ncells, cluster_mesh_layout, &w));
  STCHK(cluster_mesh_count(e, b, ncells, *params, s, w));
  return cluster_mesh_emit(e, b, ncells, *params, s, w, d_vertices, vertex_capacity, d_triangles, triangle_capacity,
                           d_counts);
}

int ratsdf_cluster_mesh(ratsdf_engine* e, const int32_t origin[3], const int32_t dims[3],
                        const ratsdf_cluster_mesh_params* params, ratsdf_surface_point** vertices,
                        size_t* n_vertices, int32_t** triangles, size_t* n_triangles) {
  MapBox b;
  size_t ncells = 0;
  int s = 0;
  ENTRY(e, vertices && n_vertices && triangles && n_triangles &&
               cluster_mesh_box(origin, dims, params, &b, &ncells, &s));
  STCHK(box_entry(e));
  STCHK(surface_mesh_tables(e));
  ClusterMeshWork w;
  STCHK(e->workspace(e->ws_cluster_mesh, ncells, cluster_mesh_layout, &w));
  STCHK(cluster_mesh_count(e, b, ncells, *params, s, w));
  uint32_t total[2] = {0, 0};
  STCHK(e->read_small(total, w.total, 8));
  // (vertices without triangles are possible: a component inside one cluster)
  const HostPart parts[2] = {{total[0], sizeof(ratsdf_surface_point), (void**)vertices, n_vertices},
                             {total[1], 12, (void**)triangles, n_triangles}};
  return hand_over(e, parts, 2, [&](uint8_t* const* d) {
    return cluster_mesh_emit(e, b, ncells, *params, s, w, d[0], (int64_t)total[0], d[1], (int64_t)total[1], w.counts);
  });
}

}  // extern "C"
