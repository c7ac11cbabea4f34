// surface_mesh.inc -- welded triangle mesh of a box of the map (include/ratsdf_surface_mesh.h): the host side of
// kernels_surface_mesh.h.  Included at the end of ratsdf_engine.hip.

extern "C" {

// the workspace of a grid of n block cells: vertices per cell | triangles per cell | where each cell's vertices start |
// where its triangles start (4n B each) | the scan's tile sums | the two totals (words) and the host entry point's two
// int64 counts, 32 bytes together | the vertex codes, 512 halfwords per cell
struct SurfaceMeshWork {
  uint32_t *cnt_v, *cnt_t, *pos_v, *pos_t, *tiles, *total;
  long long* counts;
  uint16_t* code;
};
static size_t surface_mesh_work_bytes(size_t n) {
  return 4 * esdf_round(4 * n) + esdf_round(4 * surface_tiles(n)) + esdf_round(32) + 1024 * n;
}

// argument checks of both entry points (RATSDF_ERR_BAD_ARGUMENT when false); *ncells: cells of the block grid of the
// vertex owners, the voxels [origin, origin + dims] clipped to the int16 range
static bool surface_mesh_box(const int32_t* origin, const int32_t* dims, const ratsdf_surface_mesh_params* p,
                             MeshBox* b, size_t* ncells) {
  MapBox m;
  size_t n = 0;
  if (!p || p->min_weight < 1 || p->min_weight > 255 || p->flags || p->reserved0 || p->reserved1 ||
      !esdf_box(origin, dims, 0.f, 0u, &m, &n))
    return false;
  b->ox = m.ox, b->oy = m.oy, b->oz = m.oz;
  b->X = m.X, b->Y = m.Y, b->Z = m.Z;
  b->bx0 = m.bx0, b->by0 = m.by0, b->bz0 = m.bz0;
  b->nbx = (std::min(m.ox + m.X, 32767) >> 3) - m.bx0 + 1;
  b->nby = (std::min(m.oy + m.Y, 32767) >> 3) - m.by0 + 1;
  b->nbz = (std::min(m.oz + m.Z, 32767) >> 3) - m.bz0 + 1;
  *ncells = (size_t)b->nbx * (size_t)b->nby * (size_t)b->nbz;
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

// a workspace for n cells (laid out for the number it was allocated for)
static int surface_mesh_workspace(ratsdf_engine* e, size_t n, SurfaceMeshWork* w) {
  if (e->surface_mesh_cap < n) {
    HIPCHK(hipStreamSynchronize(e->stream));  // an earlier call may still be using the old one
    e->surface_mesh_cap = 0;
    STCHK(e->d_surface_mesh.alloc(surface_mesh_work_bytes(n)));
    e->surface_mesh_cap = n;
  }
  const size_t cap = e->surface_mesh_cap;
  uint8_t* p = e->d_surface_mesh.as<uint8_t>();
  w->cnt_v = (uint32_t*)p;
  w->cnt_t = (uint32_t*)(p += esdf_round(4 * cap));
  w->pos_v = (uint32_t*)(p += esdf_round(4 * cap));
  w->pos_t = (uint32_t*)(p += esdf_round(4 * cap));
  w->tiles = (uint32_t*)(p += esdf_round(4 * cap));
  w->total = (uint32_t*)(p += esdf_round(4 * surface_tiles(cap)));
  w->counts = (long long*)(p + 8);
  w->code = (uint16_t*)(p + esdf_round(32));
  return RATSDF_OK;
}

// the count pass and the two scans: vertices and triangles per cell, where each cell's start, the totals (no more than
// 3 * 1025^3 / 8 and 5 * 2^27: both fit a word, and every vertex index an int32)
static int surface_mesh_count(ratsdf_engine* e, const MeshBox& b, size_t ncells, const ratsdf_surface_mesh_params& p,
                              const SurfaceMeshWork& w) {
  hipLaunchKernelGGL(k_surface_mesh<false>, dim3((unsigned)ncells), dim3(512), 0, e->stream, e->tab, e->pool, b,
                     (uint32_t)p.min_weight, e->vs, e->d_surface_mesh_tab.as<const SurfaceMeshTables>(), w.cnt_v,
                     w.cnt_t, w.code, (const uint32_t*)nullptr, (const uint32_t*)nullptr, (const uint32_t*)nullptr,
                     (uint4*)nullptr, 0ll, (int32_t*)nullptr, 0ll, (long long*)nullptr);
  HIPCHK(hipGetLastError());
  const uint32_t ntiles = (uint32_t)surface_tiles(ncells);
  for (int k = 0; k < 2; ++k) {  // (the tile sums of the first scan are dead when the second one starts: one stream)
    const uint32_t* cnt = k ? w.cnt_t : w.cnt_v;
    hipLaunchKernelGGL(k_mask_tile_sums, dim3(ntiles), dim3(1024), 0, e->stream, cnt, ncells, w.tiles);
    hipLaunchKernelGGL(k_scan_tile_sums, dim3(1), dim3(1024), 0, e->stream, w.tiles, ntiles, w.total + k);
    hipLaunchKernelGGL(k_mask_positions, dim3(ntiles), dim3(1024), 0, e->stream, cnt, ncells, w.tiles,
                       k ? w.pos_t : w.pos_v);
    HIPCHK(hipGetLastError());
  }
  return RATSDF_OK;
}

// the emit pass: the first min(total, capacity) records of either list, and the totals as two int64 at d_counts
static int surface_mesh_emit(ratsdf_engine* e, const MeshBox& b, size_t ncells, const ratsdf_surface_mesh_params& p,
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
  MeshBox b;
  size_t ncells = 0;
  ENTRY(e, vertex_capacity >= 0 && (d_vertices || vertex_capacity == 0) && !((uintptr_t)d_vertices & 15u) &&
               triangle_capacity >= 0 && (d_triangles || triangle_capacity == 0) && !((uintptr_t)d_triangles & 3u) &&
               d_counts && !((uintptr_t)d_counts & 7u) && surface_mesh_box(origin, dims, params, &b, &ncells));
  STCHK(e->settle());
  STCHK(sticky_raised(e));
  STCHK(surface_mesh_tables(e));
  SurfaceMeshWork w;
  STCHK(surface_mesh_workspace(e, ncells, &w));
  STCHK(surface_mesh_count(e, b, ncells, *params, w));
  return surface_mesh_emit(e, b, ncells, *params, w, d_vertices, vertex_capacity, d_triangles, triangle_capacity,
                           d_counts);
}

int ratsdf_surface_mesh(ratsdf_engine* e, const int32_t origin[3], const int32_t dims[3],
                        const ratsdf_surface_mesh_params* params, ratsdf_surface_point** vertices,
                        size_t* n_vertices, int32_t** triangles, size_t* n_triangles) {
  MeshBox b;
  size_t ncells = 0;
  ENTRY(e, vertices && n_vertices && triangles && n_triangles && surface_mesh_box(origin, dims, params, &b, &ncells));
  STCHK(e->settle());
  STCHK(sticky_raised(e));
  STCHK(surface_mesh_tables(e));
  SurfaceMeshWork w;
  STCHK(surface_mesh_workspace(e, ncells, &w));
  STCHK(surface_mesh_count(e, b, ncells, *params, w));
  uint32_t total[2] = {0, 0};
  STCHK(e->read_small(total, w.total, 8));
  *vertices = nullptr, *triangles = nullptr;
  *n_vertices = 0, *n_triangles = 0;
  if (total[0] == 0u && total[1] == 0u) return e->sticky();  // (one is zero iff the other is)
  const size_t vbytes = (size_t)total[0] * sizeof(ratsdf_surface_point), tbytes = (size_t)total[1] * 12;
  STCHK(e->staging(vbytes + tbytes, kHostChunk));
  void* hv = malloc(vbytes ? vbytes : 1);
  void* ht = malloc(tbytes ? tbytes : 1);
  int st = hv && ht ? RATSDF_OK : RATSDF_ERR_DEVICE;  // (nothing is queued: read_small drained the stream)
  uint8_t* d = e->d_out.as<uint8_t>();
  if (st == RATSDF_OK)
    st = surface_mesh_emit(e, b, ncells, *params, w, d, (int64_t)total[0], d + vbytes, (int64_t)total[1], w.counts);
  if (st == RATSDF_OK) st = e->download(hv, d, vbytes);
  if (st == RATSDF_OK) st = e->download(ht, d + vbytes, tbytes);
  if (st == RATSDF_OK) st = e->sticky();
  if (st != RATSDF_OK) {
    free(hv);
    free(ht);
    return st;
  }
  *vertices = (ratsdf_surface_point*)hv, *triangles = (int32_t*)ht;
  *n_vertices = total[0], *n_triangles = total[1];
  return RATSDF_OK;
}

}  // extern "C"
