// exposure.inc -- the exposure of surface points to lamps through a box of the map (include/ratsdf_surface.h): the host
// side of kernels_exposure.h.  Included at the end of ratsdf_engine.hip.

extern "C" {

static_assert(sizeof(ratsdf_lamp) == 16 && sizeof(ratsdf_exposure_params) == 32 && sizeof(ratsdf_lamp_record) == 16 &&
                  sizeof(ratsdf_exposure_summary) == 32 && offsetof(ratsdf_exposure_summary, lamps_accepted) == 16,
              "ratsdf_lamp / ratsdf_exposure_params / ratsdf_lamp_record / ratsdf_exposure_summary layout");
static_assert(sizeof(ratsdf_surface_point) == 32 && offsetof(ratsdf_surface_point, prob) == 24,
              "k_exposure_walk reads a point as two float4");
static_assert(RATSDF_EXPOSURE_UNKNOWN_OCCUPIED == RATSDF_ESDF_UNKNOWN_OCCUPIED, "the ESDF's bit");
static_assert(RATSDF_EXPOSURE_MAX_LAMPS == kExposureMaxLamps, "the header's limit is the kernels'");

// The workspace is EngineMem::ws_exposure (ExposureWork, workspace.h), per voxel, a buffer of its own: a field, regions
// or a cost field queued before or after share nothing with it.

constexpr int64_t kExposureMaxPoints = (int64_t)1 << 24;

struct ExposureRun {
  MapBox b;
  size_t n;
  ExposureGrid g;
  ExposureWork w;
};

// argument checks of both entry points (RATSDF_ERR_BAD_ARGUMENT when false)
static bool exposure_box(const int32_t* origin, const int32_t* dims, const ratsdf_exposure_params* p, const void* points,
                         int64_t n_points, const void* lamps, int32_t n_lamps, ExposureRun* r) {
  constexpr uint32_t all = RATSDF_EXPOSURE_UNKNOWN_OCCUPIED | RATSDF_EXPOSURE_ACCUMULATE;
  if (!p || std::isnan(p->occupied_below) || !(p->max_range >= 0.0f) || std::isnan(p->min_irradiance) ||
      std::isnan(p->p_cutoff) || (p->flags & ~all) || p->reserved[0] || p->reserved[1] || p->reserved[2] ||
      n_points < 0 || n_points > kExposureMaxPoints || (n_points > 0 && !points) || n_lamps < 0 ||
      n_lamps > kExposureMaxLamps || (n_lamps > 0 && !lamps) || !map_box(origin, dims, &r->b, &r->n))
    return false;
  r->g.nbx = (r->b.X + 3) / 4, r->g.nby = (r->b.Y + 3) / 4, r->g.nbz = (r->b.Z + 3) / 4;
  r->g.nbricks = (uint32_t)r->g.nbx * (uint32_t)r->g.nby * (uint32_t)r->g.nbz;
  return (size_t)r->g.nbricks <= exposure_bricks_max(r->n);  // (always: workspace.h)
}

// states, bitmap, lamps, walks: everything on device pointers, nothing read back
static int exposure_launch(ratsdf_engine* e, const ExposureRun& r, const ratsdf_exposure_params& p, const void* d_points,
                           int64_t n_points, const void* d_lamps, int32_t n_lamps, float* d_dose, void* d_mask,
                           void* d_table, void* d_summary) {
  const ExposureWork& w = r.w;
  hipLaunchKernelGGL(k_esdf_seed, dim3((unsigned)box_cells(r.b)), dim3(256), 0, e->stream, e->tab, e->pool, r.b,
                     p.occupied_below, w.st);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_exposure_pack, dim3((r.g.nbricks + 255u) / 256u), dim3(256), 0, e->stream,
                     (const uint8_t*)w.st, r.b.X, r.b.Y, r.b.Z, r.g, p.flags & RATSDF_EXPOSURE_UNKNOWN_OCCUPIED, w.bits);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_exposure_lamps, dim3(1), dim3(64), 0, e->stream, (const float4*)d_lamps, n_lamps, r.b, e->vs,
                     (const unsigned long long*)w.bits, r.g, (int4*)w.lamp_vox, (int4*)d_table, (uint32_t*)d_summary);
  HIPCHK(hipGetLastError());
  if (n_points == 0) return RATSDF_OK;
  ExposureArgs a;
  a.points = (const float4*)d_points, a.lamps = (const float4*)d_lamps, a.lamp_vox = (const int4*)w.lamp_vox;
  a.bits = w.bits, a.dose = d_dose, a.mask = (unsigned long long*)d_mask, a.table = (int4*)d_table;
  a.summary = (uint32_t*)d_summary, a.n_points = (uint32_t)n_points, a.n_lamps = n_lamps;
  a.log_m = 0;
  while ((1 << a.log_m) < n_lamps) ++a.log_m;
  a.vs = e->vs, a.max_range = p.max_range, a.min_irradiance = p.min_irradiance, a.p_cutoff = p.p_cutoff;
  a.accumulate = p.flags & RATSDF_EXPOSURE_ACCUMULATE;
  const uint32_t per_wave = 64u >> a.log_m;
  const uint32_t n_batches = (uint32_t)(((uint64_t)n_points + per_wave - 1) / per_wave);  // (<= 2^24)
  const uint32_t grid = std::min<uint32_t>((n_batches + 3u) / 4u, kExposureMaxWG);
  hipLaunchKernelGGL(k_exposure_walk, dim3(grid), dim3(256), 0, e->stream, a, r.b, r.g, n_batches);
  HIPCHK(hipGetLastError());
  return RATSDF_OK;
}

int ratsdf_exposure_device(ratsdf_engine* e, const int32_t origin[3], const int32_t dims[3],
                           const ratsdf_exposure_params* params, const void* d_points, int64_t n_points,
                           const void* d_lamps, int32_t n_lamps, void* d_dose, void* d_mask, void* d_lamp_table,
                           void* d_summary) {
  ExposureRun r;
  ENTRY(e, d_dose && !((uintptr_t)d_dose & 3u) && d_summary && !((uintptr_t)d_summary & 7u) &&
               !((uintptr_t)d_points & 15u) && !((uintptr_t)d_lamps & 15u) && !((uintptr_t)d_lamp_table & 15u) &&
               !((uintptr_t)d_mask & 7u) &&
               exposure_box(origin, dims, params, d_points, n_points, d_lamps, n_lamps, &r));
  STCHK(box_entry(e));
  STCHK(e->workspace(e->ws_exposure, r.n, exposure_layout, &r.w));
  return exposure_launch(e, r, *params, d_points, n_points, d_lamps, n_lamps, (float*)d_dose, d_mask, d_lamp_table,
                         d_summary);
}

// `bytes` of the caller's pageable memory to the device, through h_out in pieces of what it holds (the mirror of
// ratsdf_engine::download); each piece is waited for before the next overwrites the page-locked buffer
static int exposure_upload(ratsdf_engine* e, void* d_dst, const void* src, size_t bytes) {
  const size_t step = e->h_out.size();
  if (bytes && !step) return RATSDF_ERR_DEVICE;
  for (size_t o = 0; o < bytes; o += step) {
    const size_t m = std::min(step, bytes - o);
    memcpy(e->h_out.as<void>(), (const uint8_t*)src + o, m);
    HIPCHK(hipMemcpyAsync((uint8_t*)d_dst + o, e->h_out.as<void>(), m, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
  }
  return RATSDF_OK;
}

int ratsdf_exposure(ratsdf_engine* e, const int32_t origin[3], const int32_t dims[3],
                    const ratsdf_exposure_params* params, const ratsdf_surface_point* points, int64_t n_points,
                    const ratsdf_lamp* lamps, int32_t n_lamps, float* dose, uint64_t* mask,
                    ratsdf_lamp_record* lamp_table, ratsdf_exposure_summary* summary) {
  ExposureRun r;
  ENTRY(e, dose && summary && exposure_box(origin, dims, params, points, n_points, lamps, n_lamps, &r));
  STCHK(box_entry(e));
  STCHK(e->workspace(e->ws_exposure, r.n, exposure_layout, &r.w));
  // through the staging pair: the points | the lamps | the dose | the masks
  const size_t np = (size_t)n_points, point_bytes = ws_round(32 * np), lamp_bytes = ws_round(16 * (size_t)n_lamps);
  const size_t dose_bytes = ws_round(4 * np);
  STCHK(e->staging(point_bytes + lamp_bytes + dose_bytes + (mask ? 8 * np : 0), kHostChunk));
  uint8_t* dev = e->d_out.as<uint8_t>();
  float* d_dose = (float*)(dev + point_bytes + lamp_bytes);
  uint8_t* d_mask = mask ? dev + point_bytes + lamp_bytes + dose_bytes : nullptr;
  STCHK(exposure_upload(e, dev, points, 32 * np));
  STCHK(exposure_upload(e, dev + point_bytes, lamps, 16 * (size_t)n_lamps));
  // (without ACCUMULATE too: the entries of OUTSIDE points are not written and keep what the caller's array holds)
  STCHK(exposure_upload(e, d_dose, dose, 4 * np));
  STCHK(exposure_launch(e, r, *params, dev, n_points, dev + point_bytes, n_lamps, d_dose, d_mask,
                        lamp_table ? r.w.table : nullptr, r.w.summary));
  STCHK(e->read_small(summary, r.w.summary, sizeof(ratsdf_exposure_summary)));
  if (lamp_table && n_lamps > 0) STCHK(e->download(lamp_table, r.w.table, 16 * (size_t)n_lamps));
  STCHK(e->download(dose, d_dose, 4 * np));
  if (mask) STCHK(e->download(mask, d_mask, 8 * np));
  return e->sticky();
}

}  // extern "C"
