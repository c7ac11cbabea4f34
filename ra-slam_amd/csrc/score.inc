// score.inc -- the map scored against labelled points (include/ratsdf_score.h): label sets and the host side of
// kernels_score.h.  Included at the end of ratsdf_engine.hip.

static_assert(sizeof(ratsdf_labelset_info) == 48 && offsetof(ratsdf_labelset_info, cell) == 16 &&
                  offsetof(ratsdf_labelset_info, cells) == 32,
              "ratsdf_labelset_info layout");
static_assert(sizeof(ratsdf_score_params) == 32, "ratsdf_score_params layout");
static_assert(sizeof(ratsdf_label_score) == 8 * kScoreWords && offsetof(ratsdf_label_score, confusion) == 32 &&
                  offsetof(ratsdf_label_score, hist) == 64,
              "ratsdf_label_score layout");
static_assert(sizeof(ratsdf_voxel_label) == 8, "ratsdf_voxel_label layout");

// A label set owns its three device buffers; it belongs to a device, not to the engine that built it.
struct ratsdf_labelset {
  int device = 0;
  DevMem rec, start, label;
  ratsdf_labelset_info info{};
  LabelGrid grid{};
};

constexpr size_t kLabelMaxPoints = (size_t)1 << 26;
constexpr double kLabelMaxCells = (double)(1 << 24);
constexpr unsigned kScoreGrid = 2048;  // workgroups of k_score_labels: they stride over the blocks
// the most workgroups (of 256 threads) of the set builders' passes: beyond them a workgroup strides over the items
constexpr unsigned kBoundsGrid = 1024;     // k_label_bounds over the points, k_mesh_bounds over max(vertices, triangles)
constexpr unsigned kLabelFillGrid = 4096;  // k_label_count and k_label_scatter over the points
constexpr unsigned kMeshRefsGrid = 4096;   // k_mesh_refs over the triangles (score_mesh.inc)
constexpr unsigned kMeshCellsGrid = 8192;  // k_mesh_cells over the triangles, kMeshLanes lanes each (score_mesh.inc)

// ---- what the builds of a label set and of a mesh set (score_mesh.inc) share ----

// the first edge of a set's cells: the caller's, or 8 voxel sizes of the engine that builds it
static float score_cell_edge(const ratsdf_engine* e, float cell) {
  float c = cell == 0.f ? 8.f * e->vs : cell;
  while (c < 1e-6f) c *= 2.f;
  return c;
}

// the bounds words of a build's first pass (score_ord words) as the grid's origin and its extent per axis
static void score_bounds(const uint32_t lo_words[3], const uint32_t hi_words[3], double lo[3], double ext[3]) {
  for (int a = 0; a < 3; ++a) {
    const uint32_t bl = score_unord(lo_words[a]), bh = score_unord(hi_words[a]);
    float fl, fh;
    memcpy(&fl, &bl, 4);
    memcpy(&fh, &bh, 4);
    lo[a] = (double)(fl + 0.f);  // (-0.0 is reported as 0.0)
    ext[a] = (double)fh - (double)fl;
  }
}

// the cells per axis of a grid of edge c over the extent; false when they are more than a set may have
static bool score_cells(const double ext[3], float c, double cells[3]) {
  for (int a = 0; a < 3; ++a) cells[a] = std::floor(ext[a] / (double)c) + 1.0;
  return cells[0] * cells[1] * cells[2] <= kLabelMaxCells;
}

// the geometry of a set's grid, and what the set's info says of it
template <class Set>
static void score_grid(Set* s, const double lo[3], float c, const double cells[3]) {
  CellGrid& g = s->grid;
  g.ox = lo[0], g.oy = lo[1], g.oz = lo[2], g.cell = (double)c;
  g.cx = (int)cells[0], g.cy = (int)cells[1], g.cz = (int)cells[2];
  s->info.cell = c;
  for (int a = 0; a < 3; ++a) {
    s->info.origin[a] = (float)lo[a];
    s->info.cells[a] = (int32_t)cells[a];
  }
}

static bool labelset_args(const void* xyz, const void* labels, size_t n, float cell, ratsdf_labelset** out) {
  return out && n <= kLabelMaxPoints && (n == 0 || (xyz && labels)) && cell >= 0.f && std::isfinite(cell);
}

// the set of n points that lie on the device (d_xyz, d_labels: null when n == 0); synchronous
static int labelset_build(ratsdf_engine* e, const float* d_xyz, const uint8_t* d_labels, size_t n, float cell,
                          ratsdf_labelset** out) {
  std::unique_ptr<ratsdf_labelset> s(new (std::nothrow) ratsdf_labelset);
  if (!s) return RATSDF_ERR_DEVICE;
  s->device = e->device;
  float c = score_cell_edge(e, cell);
  struct {
    uint32_t lo[3], hi[3], bad, pad, kept[2], total, pad2[5];
  } hb;
  static_assert(sizeof(hb) == 64, "bounds record");
  memset(&hb, 0, sizeof(hb));
  DevMem d_bounds, d_cnt, d_tiles;  // (temporaries: the drain below stands between their last use and their release)
  StreamDrain drain{e->stream};
  if (n) {
    STCHK(d_bounds.alloc(sizeof(hb)));
    HIPCHK(hipMemsetAsync(d_bounds.as<void>(), 0xFF, 12, e->stream));
    HIPCHK(hipMemsetAsync(d_bounds.as<uint8_t>() + 12, 0, sizeof(hb) - 12, e->stream));
    const unsigned grid = (unsigned)std::min<size_t>((n + 255) / 256, kBoundsGrid);
    hipLaunchKernelGGL(k_label_bounds, dim3(grid), dim3(256), 0, e->stream, d_xyz, d_labels, n,
                       d_bounds.as<uint32_t>());
    HIPCHK(hipGetLastError());
    STCHK(e->read_small(&hb, d_bounds.as<void>(), sizeof(hb)));
    if (hb.bad) return RATSDF_ERR_BAD_ARGUMENT;
  } else {
    HIPCHK(hipStreamSynchronize(e->stream));
  }
  const size_t kept = (size_t)hb.kept[0] | ((size_t)hb.kept[1] << 32);
  double lo[3] = {0, 0, 0}, ext[3] = {0, 0, 0}, cells[3] = {1, 1, 1};
  if (kept) {
    score_bounds(hb.lo, hb.hi, lo, ext);
    for (;; c *= 2.f) {
      if (!std::isfinite(c)) return RATSDF_ERR_BAD_ARGUMENT;
      if (score_cells(ext, c, cells)) break;
    }
  }
  const size_t ncell = (size_t)cells[0] * (size_t)cells[1] * (size_t)cells[2];
  STCHK(s->start.alloc(4 * (ncell + 1)));
  HIPCHK(hipMemsetAsync(s->start.as<void>(), 0, 4 * (ncell + 1), e->stream));
  LabelGrid& g = s->grid;
  score_grid(s.get(), lo, c, cells);
  if (kept) {
    STCHK(s->rec.alloc(16 * kept));
    STCHK(s->label.alloc(n));
    STCHK(d_cnt.alloc(4 * (ncell + 1)));
    STCHK(d_tiles.alloc(4 * scan_tiles(ncell + 1)));
    g.rec = s->rec.as<const float4>();
    g.start = s->start.as<const uint32_t>();
    g.label = s->label.as<const uint8_t>();
    const unsigned grid = (unsigned)std::min<size_t>((n + 255) / 256, kLabelFillGrid);
    uint32_t* const cnt = d_cnt.as<uint32_t>();
    HIPCHK(hipMemsetAsync(cnt, 0, 4 * (ncell + 1), e->stream));
    hipLaunchKernelGGL(k_label_count, dim3(grid), dim3(256), 0, e->stream, d_xyz, n, g, cnt);
    HIPCHK(hipGetLastError());
    // (one count more than there are cells, a zero: its position is the total, the end of the last cell)
    STCHK(scan_counts(e, cnt, ncell + 1, d_tiles.as<uint32_t>(), d_bounds.as<uint32_t>() + 10,
                      s->start.as<uint32_t>()));
    HIPCHK(hipMemsetAsync(cnt, 0, 4 * (ncell + 1), e->stream));
    hipLaunchKernelGGL(k_label_scatter, dim3(grid), dim3(256), 0, e->stream, d_xyz, n, g, cnt, s->rec.as<float4>(),
                       (uint32_t)kept);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(s->label.as<void>(), d_labels, n, hipMemcpyDeviceToDevice, e->stream));
  } else {
    g.start = s->start.as<const uint32_t>();
  }
  HIPCHK(hipStreamSynchronize(e->stream));
  s->info.points = (int64_t)n;
  s->info.kept = (int64_t)kept;
  *out = s.release();
  return RATSDF_OK;
}

// ---- what the entry points of a label set and of a mesh set (score_mesh.inc) share: Set is ratsdf_labelset or
// ratsdf_labelmesh, `kernel` its join (k_score_labels, k_score_mesh) ----

template <class Set, class Info>
static int set_info_get(const Set* s, Info* out) {
  if (!s || !out) return RATSDF_ERR_BAD_ARGUMENT;
  *out = s->info;
  return RATSDF_OK;
}

// (waits for the device first: a scoring call queued on any engine's stream may still read the set)
template <class Set>
static int set_destroy(Set* s) {
  if (!s) return RATSDF_ERR_BAD_ARGUMENT;
  DeviceGuard guard(s->device);
  if (!guard.ok()) return RATSDF_ERR_DEVICE;
  const hipError_t err = hipDeviceSynchronize();
  delete s;
  return err == hipSuccess ? RATSDF_OK : RATSDF_ERR_DEVICE;
}

// argument checks of the scoring entry points (RATSDF_ERR_BAD_ARGUMENT when false), for a set of `device` with cells
// of edge `cell`
static bool score_args(const ratsdf_engine* e, int device, float cell, const ratsdf_score_params* p) {
  if (!p || device != e->device) return false;
  const float md2 = p->max_dist * p->max_dist;
  return !std::isnan(p->tsdf_below) && !std::isnan(p->p_cutoff) && std::isfinite(p->max_dist) && p->max_dist > 0.f &&
         p->max_dist <= 64.f * cell && std::isfinite(md2) && md2 > 0.f && p->min_weight <= 255u && p->flags == 0u &&
         p->reserved[0] == 0u && p->reserved[1] == 0u && p->reserved[2] == 0u;
}

// the join over the blocks that e->select has listed: the score at d_score, the per-voxel records (if any) at d_pv
template <class Set, class Kernel>
static int score_launch(ratsdf_engine* e, Kernel kernel, const Set* s, const ratsdf_score_params& p, void* d_score,
                        void* d_pv, int64_t capacity, void* d_count) {
  HIPCHK(hipMemsetAsync(d_score, 0, sizeof(ratsdf_label_score), e->stream));
  const ScoreArgs a = {p.tsdf_below, p.max_dist * p.max_dist, p.p_cutoff, p.min_weight};
  hipLaunchKernelGGL(kernel, dim3(kScoreGrid), dim3(kScoreWG), 0, e->stream, e->pool, (const VisItem*)e->vis,
                     (const uint32_t*)&e->ctl->n_sel, e->vs, s->grid, a, (unsigned long long*)d_score, (int2*)d_pv,
                     (long long)capacity, (long long*)d_count);
  HIPCHK(hipGetLastError());
  return RATSDF_OK;
}

// ratsdf_score_labels_device, ratsdf_score_mesh_device
template <class Set, class Kernel>
static int score_device(ratsdf_engine* e, Kernel kernel, const Set* s, const ratsdf_score_params* p, void* d_score,
                        void* d_per_voxel, int64_t capacity, void* d_count) {
  ENTRY(e, capacity >= 0 && d_score && !((uintptr_t)d_score & 7u) && !((uintptr_t)d_per_voxel & 7u) && d_count &&
               !((uintptr_t)d_count & 7u) && s && score_args(e, s->device, s->info.cell, p));
  STCHK(box_entry(e));
  STCHK(e->select(kSelValid, GridBounds{}, &e->ctl->n_sel));
  return score_launch(e, kernel, s, *p, d_score, d_per_voxel, capacity, d_count);
}

// ratsdf_score_labels, ratsdf_score_mesh.  (Both use ws_score: a call has downloaded the table before it returns, and
// the calls of an engine are synchronous on its one stream.)
template <class Set, class Kernel>
static int score_host(ratsdf_engine* e, Kernel kernel, const Set* s, const ratsdf_score_params* p,
                      ratsdf_label_score* out, ratsdf_voxel_label** per_voxel, size_t* n_out) {
  ENTRY(e, out && (!per_voxel || n_out) && s && score_args(e, s->device, s->info.cell, p));
  STCHK(box_entry(e));
  ScoreWork w;
  STCHK(e->workspace(e->ws_score, 1, score_layout, &w));
  STCHK(e->staging(0, kHostChunk));
  STCHK(e->select(kSelValid, GridBounds{}, &e->ctl->n_sel));
  uint32_t nb = 0;
  STCHK(e->read_small(&nb, &e->ctl->n_sel, 4));
  STCHK(sticky_raised(e));
  const size_t total = per_voxel ? (size_t)nb * RATSDF_BLOCK_VOLUME : 0;
  if (total) {
    const HostPart part = {total, sizeof(ratsdf_voxel_label), (void**)per_voxel, n_out};
    STCHK(hand_over(e, &part, 1, [&](uint8_t* const* d) {
      return score_launch(e, kernel, s, *p, w.score, d[0], (int64_t)total, w.count);
    }));
  } else {
    if (per_voxel) *per_voxel = nullptr, *n_out = 0;
    STCHK(score_launch(e, kernel, s, *p, w.score, nullptr, 0, w.count));
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

extern "C" {

int ratsdf_labelset_create_device(ratsdf_engine* e, const void* d_xyz, const void* d_labels, size_t n, float cell,
                                  ratsdf_labelset** out) {
  ENTRY(e, labelset_args(d_xyz, d_labels, n, cell, out));
  return labelset_build(e, (const float*)d_xyz, (const uint8_t*)d_labels, n, cell, out);
}

int ratsdf_labelset_create(ratsdf_engine* e, const float* xyz, const uint8_t* labels, size_t n, float cell,
                           ratsdf_labelset** out) {
  ENTRY(e, labelset_args(xyz, labels, n, cell, out));
  for (size_t i = 0; i < n; ++i)
    if (labels[i] > 2u) return RATSDF_ERR_BAD_ARGUMENT;
  DevMem d_xyz, d_labels;
  StreamDrain drain{e->stream};
  if (n) {
    STCHK(d_xyz.alloc(12 * n));
    STCHK(d_labels.alloc(n));
    HIPCHK(hipMemcpyAsync(d_xyz.as<void>(), xyz, 12 * n, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(d_labels.as<void>(), labels, n, hipMemcpyHostToDevice, e->stream));
  }
  return labelset_build(e, d_xyz.as<const float>(), d_labels.as<const uint8_t>(), n, cell, out);
}

int ratsdf_labelset_info_get(const ratsdf_labelset* s, ratsdf_labelset_info* out) { return set_info_get(s, out); }

int ratsdf_labelset_destroy(ratsdf_labelset* s) { return set_destroy(s); }

int ratsdf_score_labels_device(ratsdf_engine* e, const ratsdf_labelset* s, const ratsdf_score_params* p, void* d_score,
                               void* d_per_voxel, int64_t capacity, void* d_count) {
  return score_device(e, k_score_labels, s, p, d_score, d_per_voxel, capacity, d_count);
}

int ratsdf_score_labels(ratsdf_engine* e, const ratsdf_labelset* s, const ratsdf_score_params* p,
                        ratsdf_label_score* out, ratsdf_voxel_label** per_voxel, size_t* n_out) {
  return score_host(e, k_score_labels, s, p, out, per_voxel, n_out);
}

}  // extern "C"
