// score_mesh.inc -- the map scored against a labelled triangle mesh (include/ratsdf_score_mesh.h): mesh sets and the
// host side of kernels_score_mesh.h.  Included at the end of ratsdf_engine.hip, after score.inc, which holds what the
// two kinds of set share: the helpers of the builds, the parameter check, the launch and the bodies of the scoring
// entry points.

static_assert(sizeof(ratsdf_labelmesh_info) == 72 && offsetof(ratsdf_labelmesh_info, refs) == 32 &&
                  offsetof(ratsdf_labelmesh_info, cell) == 40 && offsetof(ratsdf_labelmesh_info, cells) == 56,
              "ratsdf_labelmesh_info layout");

// A mesh set owns its four device buffers; it belongs to a device, not to the engine that built it.
struct ratsdf_labelmesh {
  int device = 0;
  DevMem rec, start, ref, label;
  ratsdf_labelmesh_info info{};
  MeshGrid grid{};
};

constexpr size_t kMeshMaxItems = (size_t)1 << 26;  // vertices, and triangles

static bool labelmesh_args(const void* xyz, const void* labels, size_t nv, const void* tri, size_t nt, float cell,
                           ratsdf_labelmesh** out) {
  return out && nv <= kMeshMaxItems && nt <= kMeshMaxItems && (nv == 0 || (xyz && labels)) && (nt == 0 || tri) &&
         cell >= 0.f && std::isfinite(cell);
}

// the set of nv vertices and nt triangles that lie on the device (null pointers where a count is 0); synchronous
static int labelmesh_build(ratsdf_engine* e, const float* d_xyz, const uint8_t* d_labels, size_t nv,
                           const int32_t* d_tri, size_t nt, float cell, ratsdf_labelmesh** out) {
  std::unique_ptr<ratsdf_labelmesh> s(new (std::nothrow) ratsdf_labelmesh);
  if (!s) return RATSDF_ERR_DEVICE;
  s->device = e->device;
  float c = score_cell_edge(e, cell);
  struct {
    uint32_t lo[3], hi[3], bad_label, bad_index, kept, mixed, total, pad, refs[2], pad2[2];
  } hb;
  static_assert(sizeof(hb) == 64, "bounds record");
  memset(&hb, 0, sizeof(hb));
  DevMem d_bounds, d_cnt, d_tiles;  // (temporaries: the drain below stands between their last use and their release)
  StreamDrain drain{e->stream};
  if (nv || nt) {
    STCHK(d_bounds.alloc(sizeof(hb)));
    HIPCHK(hipMemsetAsync(d_bounds.as<void>(), 0xFF, 12, e->stream));
    HIPCHK(hipMemsetAsync(d_bounds.as<uint8_t>() + 12, 0, sizeof(hb) - 12, e->stream));
    const unsigned grid = (unsigned)std::min<size_t>((std::max(nv, nt) + 255) / 256, kBoundsGrid);
    hipLaunchKernelGGL(k_mesh_bounds, dim3(grid), dim3(256), 0, e->stream, d_xyz, d_labels, nv, d_tri, nt,
                       d_bounds.as<uint32_t>());
    HIPCHK(hipGetLastError());
    STCHK(e->read_small(&hb, d_bounds.as<void>(), sizeof(hb)));
    if (hb.bad_label || hb.bad_index) return RATSDF_ERR_BAD_ARGUMENT;
  } else {
    HIPCHK(hipStreamSynchronize(e->stream));
  }
  const size_t kept = hb.kept;
  const unsigned tgrid = (unsigned)std::min<size_t>((nt + 255) / 256, kMeshRefsGrid);
  MeshGrid& g = s->grid;
  double lo[3] = {0, 0, 0}, ext[3] = {0, 0, 0}, cells[3] = {1, 1, 1};
  unsigned long long refs = 0;
  if (kept) {
    score_bounds(hb.lo, hb.hi, lo, ext);
    unsigned long long* const d_refs = (unsigned long long*)(d_bounds.as<uint32_t>() + 12);
    for (;; c *= 2.f) {
      if (!std::isfinite(c)) return RATSDF_ERR_BAD_ARGUMENT;
      if (!score_cells(ext, c, cells)) continue;
      // the references of this edge: a sum of products of spans, no pass over cells
      score_grid(s.get(), lo, c, cells);
      HIPCHK(hipMemsetAsync(d_refs, 0, 8, e->stream));
      hipLaunchKernelGGL(k_mesh_refs, dim3(tgrid), dim3(256), 0, e->stream, d_xyz, nv, d_tri, nt, g, d_refs);
      HIPCHK(hipGetLastError());
      STCHK(e->read_small(&refs, d_refs, 8));
      if (refs <= (unsigned long long)RATSDF_LABELMESH_MAX_REFS) break;
    }
  }
  const size_t ncell = (size_t)cells[0] * (size_t)cells[1] * (size_t)cells[2];
  STCHK(s->start.alloc(4 * (ncell + 1)));
  HIPCHK(hipMemsetAsync(s->start.as<void>(), 0, 4 * (ncell + 1), e->stream));
  score_grid(s.get(), lo, c, cells);
  g.start = s->start.as<const uint32_t>();
  if (kept) {
    STCHK(s->rec.alloc(48 * nt));
    STCHK(s->ref.alloc(4 * (size_t)refs));
    STCHK(s->label.alloc(nt));
    STCHK(d_cnt.alloc(4 * (ncell + 1)));
    STCHK(d_tiles.alloc(4 * scan_tiles(ncell + 1)));
    g.rec = s->rec.as<const float4>();
    g.ref = s->ref.as<const uint32_t>();
    g.label = s->label.as<const uint8_t>();
    const unsigned grid = (unsigned)std::min<size_t>((nt * kMeshLanes + 255) / 256, kMeshCellsGrid);
    uint32_t* const cnt = d_cnt.as<uint32_t>();
    HIPCHK(hipMemsetAsync(cnt, 0, 4 * (ncell + 1), e->stream));
    hipLaunchKernelGGL(k_mesh_cells<false>, dim3(grid), dim3(256), 0, e->stream, d_xyz, d_labels, nv, d_tri, nt, g,
                       cnt, (uint32_t*)nullptr, (float4*)nullptr, (uint8_t*)nullptr, 0u);
    HIPCHK(hipGetLastError());
    // (one count more than there are cells, a zero: its position is the total, the end of the last cell)
    STCHK(scan_counts(e, cnt, ncell + 1, d_tiles.as<uint32_t>(), d_bounds.as<uint32_t>() + 10,
                      s->start.as<uint32_t>()));
    HIPCHK(hipMemsetAsync(cnt, 0, 4 * (ncell + 1), e->stream));
    HIPCHK(hipMemsetAsync(s->label.as<void>(), 0, nt, e->stream));
    hipLaunchKernelGGL(k_mesh_cells<true>, dim3(grid), dim3(256), 0, e->stream, d_xyz, d_labels, nv, d_tri, nt, g, cnt,
                       s->ref.as<uint32_t>(), s->rec.as<float4>(), s->label.as<uint8_t>(), (uint32_t)refs);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipStreamSynchronize(e->stream));
  s->info.vertices = (int64_t)nv;
  s->info.triangles = (int64_t)nt;
  s->info.kept = (int64_t)kept;
  s->info.mixed = (int64_t)hb.mixed;
  s->info.refs = (int64_t)refs;
  *out = s.release();
  return RATSDF_OK;
}

extern "C" {

int ratsdf_labelmesh_create_device(ratsdf_engine* e, const void* d_xyz, const void* d_labels, size_t n_vertices,
                                   const void* d_tri, size_t n_triangles, float cell, ratsdf_labelmesh** out) {
  ENTRY(e, labelmesh_args(d_xyz, d_labels, n_vertices, d_tri, n_triangles, cell, out));
  return labelmesh_build(e, (const float*)d_xyz, (const uint8_t*)d_labels, n_vertices, (const int32_t*)d_tri,
                         n_triangles, cell, out);
}

int ratsdf_labelmesh_create(ratsdf_engine* e, const float* xyz, const uint8_t* labels, size_t n_vertices,
                            const int32_t* tri, size_t n_triangles, float cell, ratsdf_labelmesh** out) {
  ENTRY(e, labelmesh_args(xyz, labels, n_vertices, tri, n_triangles, cell, out));
  for (size_t i = 0; i < n_vertices; ++i)
    if (labels[i] > 2u) return RATSDF_ERR_BAD_ARGUMENT;
  for (size_t i = 0; i < 3 * n_triangles; ++i)
    if (tri[i] < 0 || (size_t)tri[i] >= n_vertices) return RATSDF_ERR_BAD_ARGUMENT;
  DevMem d_xyz, d_labels, d_tri;
  StreamDrain drain{e->stream};
  if (n_vertices) {
    STCHK(d_xyz.alloc(12 * n_vertices));
    STCHK(d_labels.alloc(n_vertices));
    HIPCHK(hipMemcpyAsync(d_xyz.as<void>(), xyz, 12 * n_vertices, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(d_labels.as<void>(), labels, n_vertices, hipMemcpyHostToDevice, e->stream));
  }
  if (n_triangles) {
    STCHK(d_tri.alloc(12 * n_triangles));
    HIPCHK(hipMemcpyAsync(d_tri.as<void>(), tri, 12 * n_triangles, hipMemcpyHostToDevice, e->stream));
  }
  return labelmesh_build(e, d_xyz.as<const float>(), d_labels.as<const uint8_t>(), n_vertices,
                         d_tri.as<const int32_t>(), n_triangles, cell, out);
}

int ratsdf_labelmesh_info_get(const ratsdf_labelmesh* m, ratsdf_labelmesh_info* out) { return set_info_get(m, out); }

int ratsdf_labelmesh_destroy(ratsdf_labelmesh* m) { return set_destroy(m); }

int ratsdf_score_mesh_device(ratsdf_engine* e, const ratsdf_labelmesh* m, const ratsdf_score_params* p, void* d_score,
                             void* d_per_voxel, int64_t capacity, void* d_count) {
  return score_device(e, k_score_mesh, m, p, d_score, d_per_voxel, capacity, d_count);
}

int ratsdf_score_mesh(ratsdf_engine* e, const ratsdf_labelmesh* m, const ratsdf_score_params* p,
                      ratsdf_label_score* out, ratsdf_voxel_label** per_voxel, size_t* n_out) {
  return score_host(e, k_score_mesh, m, p, out, per_voxel, n_out);
}

}  // extern "C"
