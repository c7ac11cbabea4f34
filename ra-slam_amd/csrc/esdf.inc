// esdf.inc -- Euclidean signed distance field over a box of the map (include/ratsdf_esdf.h): the host side of
// kernels_esdf.h.  Included at the end of ratsdf_engine.hip.

extern "C" {

// argument checks of both entry points (RATSDF_ERR_BAD_ARGUMENT when false)
static bool esdf_box(const int32_t* origin, const int32_t* dims, float occupied_below, uint32_t flags, MapBox* b,
                     size_t* n) {
  return !std::isnan(occupied_below) && !(flags & ~RATSDF_ESDF_UNKNOWN_OCCUPIED) && map_box(origin, dims, b, n);
}

// the four passes; w: the workspace of EngineMem::ws_esdf (EsdfWork, workspace.h: its 8-byte records are uint2)
static int esdf_launch(ratsdf_engine* e, const MapBox& b, size_t n, float occupied_below, uint32_t flags,
                       const EsdfWork& w, float* d_out, uint8_t* d_state) {
  uint8_t* st = d_state ? d_state : w.st;
  hipLaunchKernelGGL(k_esdf_seed, dim3((unsigned)box_cells(b)), dim3(256), 0, e->stream, e->tab, e->pool, b,
                     occupied_below, st);
  HIPCHK(hipGetLastError());
  const uint32_t omask = (1u << kEsdfOccupied) | ((flags & RATSDF_ESDF_UNKNOWN_OCCUPIED) ? 1u << kEsdfUnknown : 0u);
  const uint32_t rows = (uint32_t)(n / (size_t)b.X);
  hipLaunchKernelGGL(k_esdf_x, dim3((rows + 3) / 4), dim3(256), 0, e->stream, st, omask, b.X, rows, w.gx);
  HIPCHK(hipGetLastError());
  const uint32_t cy = (uint32_t)b.X * (uint32_t)b.Z, cz = (uint32_t)b.X * (uint32_t)b.Y;
  uint2 *stk0 = (uint2*)w.stk0, *stk1 = (uint2*)w.stk1;
  hipLaunchKernelGGL(k_esdf_col<1>, dim3((cy + kEsdfColWG - 1) / kEsdfColWG), dim3(kEsdfColWG), 0, e->stream,
                     (const void*)w.gx, b.Y, b.X, (uint32_t)b.X * (uint32_t)b.Y, (uint32_t)b.X, cy, stk0, stk1,
                     (void*)w.gy, e->vs);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_esdf_col<2>, dim3((cz + kEsdfColWG - 1) / kEsdfColWG), dim3(kEsdfColWG), 0, e->stream,
                     (const void*)w.gy, b.Z, b.X, (uint32_t)b.X, (uint32_t)b.X * (uint32_t)b.Y, cz, stk0, stk1,
                     (void*)d_out, e->vs);
  HIPCHK(hipGetLastError());
  return RATSDF_OK;
}

int ratsdf_esdf_device(ratsdf_engine* e, const int32_t origin[3], const int32_t dims[3], float occupied_below,
                       uint32_t flags, void* d_out, void* d_state) {
  MapBox b;
  size_t n = 0;
  ENTRY(e, d_out && !((uintptr_t)d_out & 15u) && esdf_box(origin, dims, occupied_below, flags, &b, &n));
  STCHK(box_entry(e));
  EsdfWork w;
  STCHK(e->workspace(e->ws_esdf, n, esdf_layout, &w));
  return esdf_launch(e, b, n, occupied_below, flags, w, (float*)d_out, (uint8_t*)d_state);
}

int ratsdf_esdf(ratsdf_engine* e, const int32_t origin[3], const int32_t dims[3], float occupied_below,
                uint32_t flags, float* out, uint8_t* state) {
  MapBox b;
  size_t n = 0;
  ENTRY(e, out && esdf_box(origin, dims, occupied_below, flags, &b, &n));
  STCHK(box_entry(e));
  EsdfWork w;
  STCHK(e->workspace(e->ws_esdf, n, esdf_layout, &w));
  STCHK(e->staging(0, kHostChunk));
  // the field lands in the x pass's buffer, dead once the y pass has run
  STCHK(esdf_launch(e, b, n, occupied_below, flags, w, (float*)w.gx, nullptr));
  STCHK(e->download(out, w.gx, n * sizeof(float)));
  if (state) STCHK(e->download(state, w.st, n));
  return e->sticky();
}

}  // extern "C"
