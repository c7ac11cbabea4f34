// score_mesh.inc -- the map scored against a labelled triangle mesh (include/ratsdf_score_mesh.h): mesh sets and the
// host side of kernels_score_mesh.h.  Included at the end of ratsdf_engine.hip, after score.inc (it shares score_args'
// checks of the parameters and the grid of workgroups).

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
  float c = cell == 0.f ? 8.f * e->vs : cell;
  while (c < 1e-6f) c *= 2.f;
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
    const unsigned grid = (unsigned)std::min<size_t>((std::max(nv, nt) + 255) / 256, 1024);
    hipLaunchKernelGGL(k_mesh_bounds, dim3(grid), dim3(256), 0, e->stream, d_xyz, d_labels, nv, d_tri, nt,
                       d_bounds.as<uint32_t>());
    HIPCHK(hipGetLastError());
    STCHK(e->read_small(&hb, d_bounds.as<void>(), sizeof(hb)));
    if (hb.bad_label || hb.bad_index) return RATSDF_ERR_BAD_ARGUMENT;
  } else {
    HIPCHK(hipStreamSynchronize(e->stream));
  }
  const size_t kept = hb.kept;
  const unsigned tgrid = (unsigned)std::min<size_t>((nt + 255) / 256, 4096);
  MeshGrid& g = s->grid;
  double lo[3] = {0, 0, 0}, ext[3] = {0, 0, 0}, cells[3] = {1, 1, 1};
  unsigned long long refs = 0;
  if (kept) {
    for (int a = 0; a < 3; ++a) {
      const uint32_t bl = score_unord(hb.lo[a]), bh = score_unord(hb.hi[a]);
      float fl, fh;
      memcpy(&fl, &bl, 4);
      memcpy(&fh, &bh, 4);
      lo[a] = (double)(fl + 0.f);  // (-0.0 is reported as 0.0)
      ext[a] = (double)fh - (double)fl;
    }
    g.ox = lo[0], g.oy = lo[1], g.oz = lo[2];
    unsigned long long* const d_refs = (unsigned long long*)(d_bounds.as<uint32_t>() + 12);
    for (;; c *= 2.f) {
      if (!std::isfinite(c)) return RATSDF_ERR_BAD_ARGUMENT;
      for (int a = 0; a < 3; ++a) cells[a] = std::floor(ext[a] / (double)c) + 1.0;
      if (cells[0] * cells[1] * cells[2] > kLabelMaxCells) continue;
      // the references of this edge: a sum of products of spans, no pass over cells
      g.cell = (double)c;
      g.cx = (int)cells[0], g.cy = (int)cells[1], g.cz = (int)cells[2];
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
  g.ox = lo[0], g.oy = lo[1], g.oz = lo[2], g.cell = (double)c;
  g.cx = (int)cells[0], g.cy = (int)cells[1], g.cz = (int)cells[2];
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
    const unsigned grid = (unsigned)std::min<size_t>((nt * kMeshLanes + 255) / 256, 8192);
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
  s->info.cell = c;
  for (int a = 0; a < 3; ++a) {
    s->info.origin[a] = (float)lo[a];
    s->info.cells[a] = (int32_t)cells[a];
  }
  *out = s.release();
  return RATSDF_OK;
}

// argument checks of both scoring entry points (RATSDF_ERR_BAD_ARGUMENT when false): score_args' for a mesh set
static bool score_mesh_args(const ratsdf_engine* e, const ratsdf_labelmesh* s, const ratsdf_score_params* p) {
  if (!s || !p || s->device != e->device) return false;
  const float md2 = p->max_dist * p->max_dist;
  return !std::isnan(p->tsdf_below) && !std::isnan(p->p_cutoff) && std::isfinite(p->max_dist) && p->max_dist > 0.f &&
         p->max_dist <= 64.f * s->info.cell && std::isfinite(md2) && md2 > 0.f && p->min_weight <= 255u &&
         p->flags == 0u && p->reserved[0] == 0u && p->reserved[1] == 0u && p->reserved[2] == 0u;
}

// the join over the blocks that e->select has listed: the score at d_score, the per-voxel records (if any) at d_pv
static int score_mesh_launch(ratsdf_engine* e, const ratsdf_labelmesh* s, const ratsdf_score_params& p, void* d_score,
                             void* d_pv, int64_t capacity, void* d_count) {
  HIPCHK(hipMemsetAsync(d_score, 0, sizeof(ratsdf_label_score), e->stream));
  const ScoreArgs a = {p.tsdf_below, p.max_dist * p.max_dist, p.p_cutoff, p.min_weight};
  hipLaunchKernelGGL(k_score_mesh, dim3(kScoreGrid), dim3(kScoreWG), 0, e->stream, e->pool, (const VisItem*)e->vis,
                     (const uint32_t*)&e->ctl->n_sel, e->vs, s->grid, a, (unsigned long long*)d_score, (int2*)d_pv,
                     (long long)capacity, (long long*)d_count);
  HIPCHK(hipGetLastError());
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

int ratsdf_labelmesh_info_get(const ratsdf_labelmesh* m, ratsdf_labelmesh_info* out) {
  if (!m || !out) return RATSDF_ERR_BAD_ARGUMENT;
  *out = m->info;
  return RATSDF_OK;
}

// (waits for the device first: a scoring call queued on any engine's stream may still read the set)
int ratsdf_labelmesh_destroy(ratsdf_labelmesh* m) {
  if (!m) return RATSDF_ERR_BAD_ARGUMENT;
  DeviceGuard guard(m->device);
  if (!guard.ok()) return RATSDF_ERR_DEVICE;
  const hipError_t err = hipDeviceSynchronize();
  delete m;
  return err == hipSuccess ? RATSDF_OK : RATSDF_ERR_DEVICE;
}

int ratsdf_score_mesh_device(ratsdf_engine* e, const ratsdf_labelmesh* m, const ratsdf_score_params* p, void* d_score,
                             void* d_per_voxel, int64_t capacity, void* d_count) {
  ENTRY(e, capacity >= 0 && d_score && !((uintptr_t)d_score & 7u) && !((uintptr_t)d_per_voxel & 7u) && d_count &&
               !((uintptr_t)d_count & 7u) && score_mesh_args(e, m, p));
  STCHK(box_entry(e));
  STCHK(e->select(kSelValid, GridBounds{}, &e->ctl->n_sel));
  return score_mesh_launch(e, m, *p, d_score, d_per_voxel, capacity, d_count);
}

int ratsdf_score_mesh(ratsdf_engine* e, const ratsdf_labelmesh* m, const ratsdf_score_params* p,
                      ratsdf_label_score* out, ratsdf_voxel_label** per_voxel, size_t* n_out) {
  ENTRY(e, out && (!per_voxel || n_out) && score_mesh_args(e, m, p));
  STCHK(box_entry(e));
  ScoreMeshWork w;
  STCHK(e->workspace(e->ws_score_mesh, 1, score_mesh_layout, &w));
  STCHK(e->staging(0, kHostChunk));
  STCHK(e->select(kSelValid, GridBounds{}, &e->ctl->n_sel));
  uint32_t nb = 0;
  STCHK(e->read_small(&nb, &e->ctl->n_sel, 4));
  STCHK(sticky_raised(e));
  const size_t total = per_voxel ? (size_t)nb * RATSDF_BLOCK_VOLUME : 0;
  if (total) {
    const HostPart part = {total, sizeof(ratsdf_voxel_label), (void**)per_voxel, n_out};
    STCHK(hand_over(e, &part, 1, [&](uint8_t* const* d) {
      return score_mesh_launch(e, m, *p, w.score, d[0], (int64_t)total, w.count);
    }));
  } else {
    if (per_voxel) *per_voxel = nullptr, *n_out = 0;
    STCHK(score_mesh_launch(e, m, *p, w.score, nullptr, 0, w.count));
  }
  ratsdf_label_score host;
  int st = e->download(&host, w.score, sizeof(host));
  if (st == RATSDF_OK) st = e->sticky();
  if (st != RATSDF_OK) {
    if (per_voxel && *per_voxel) {
      free(*per_voxel);
      *per_voxel = nullptr, *n_out = 0;
    }
    return st;
  }
  *out = host;
  return RATSDF_OK;
}

}  // extern "C"
