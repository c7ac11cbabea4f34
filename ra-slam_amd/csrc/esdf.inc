// esdf.inc -- Euclidean signed distance field over a box of the map (include/ratsdf_esdf.h): the host side of
// kernels_esdf.h.  Included at the end of ratsdf_engine.hip.

extern "C" {

constexpr size_t kEsdfMaxVoxels = (size_t)1 << 27;

// the workspace of a box of n voxels: state (n B) | x pass (4n B; the host entry point's field after the z pass) |
// y pass (8n B) | stack of the transform to O (8n B) | stack of the transform to box \ O (8n B)
struct EsdfWork {
  uint8_t* st;
  uint32_t* gx;
  uint2 *gy, *stk0, *stk1;
};
static size_t esdf_round(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
static size_t esdf_work_bytes(size_t n) { return esdf_round(n) + esdf_round(4 * n) + 3 * esdf_round(8 * n); }

// argument checks of both entry points (RATSDF_ERR_BAD_ARGUMENT when false)
static bool esdf_box(const int32_t* origin, const int32_t* dims, float occupied_below, uint32_t flags, MapBox* b,
                     size_t* n) {
  if (!origin || !dims || std::isnan(occupied_below) || (flags & ~RATSDF_ESDF_UNKNOWN_OCCUPIED)) return false;
  size_t m = 1;
  for (int a = 0; a < 3; ++a) {
    if (dims[a] < 1 || dims[a] > 1024 || origin[a] < -32768 || (int64_t)origin[a] + dims[a] - 1 > 32767) return false;
    m *= (size_t)dims[a];
  }
  if (m > kEsdfMaxVoxels) return false;
  b->ox = origin[0], b->oy = origin[1], b->oz = origin[2];
  b->X = dims[0], b->Y = dims[1], b->Z = dims[2];
  b->bx0 = origin[0] >> 3, b->by0 = origin[1] >> 3, b->bz0 = origin[2] >> 3;
  b->nbx = ((origin[0] + dims[0] - 1) >> 3) - b->bx0 + 1;
  b->nby = ((origin[1] + dims[1] - 1) >> 3) - b->by0 + 1;
  *n = m;
  return true;
}

// a workspace for n voxels (laid out for the number it was allocated for)
static int esdf_workspace(ratsdf_engine* e, size_t n, EsdfWork* w) {
  if (e->esdf_cap < n) {
    HIPCHK(hipStreamSynchronize(e->stream));  // an earlier field may still be using the old one
    e->esdf_cap = 0;
    STCHK(e->d_esdf.alloc(esdf_work_bytes(n)));
    e->esdf_cap = n;
  }
  const size_t cap = e->esdf_cap;
  uint8_t* p = e->d_esdf.as<uint8_t>();
  w->st = p;
  w->gx = (uint32_t*)(p += esdf_round(cap));
  w->gy = (uint2*)(p += esdf_round(4 * cap));
  w->stk0 = (uint2*)(p += esdf_round(8 * cap));
  w->stk1 = (uint2*)(p += esdf_round(8 * cap));
  return RATSDF_OK;
}

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
  hipLaunchKernelGGL(k_esdf_col<1>, dim3((cy + kEsdfColWG - 1) / kEsdfColWG), dim3(kEsdfColWG), 0, e->stream,
                     (const void*)w.gx, b.Y, b.X, (uint32_t)b.X * (uint32_t)b.Y, (uint32_t)b.X, cy, w.stk0, w.stk1,
                     (void*)w.gy, e->vs);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_esdf_col<2>, dim3((cz + kEsdfColWG - 1) / kEsdfColWG), dim3(kEsdfColWG), 0, e->stream,
                     (const void*)w.gy, b.Z, b.X, (uint32_t)b.X, (uint32_t)b.X * (uint32_t)b.Y, cz, w.stk0, w.stk1,
                     (void*)d_out, e->vs);
  HIPCHK(hipGetLastError());
  return RATSDF_OK;
}

int ratsdf_esdf_device(ratsdf_engine* e, const int32_t origin[3], const int32_t dims[3], float occupied_below,
                       uint32_t flags, void* d_out, void* d_state) {
  MapBox b;
  size_t n = 0;
  ENTRY(e, d_out && !((uintptr_t)d_out & 15u) && esdf_box(origin, dims, occupied_below, flags, &b, &n));
  STCHK(e->settle());
  STCHK(sticky_raised(e));
  EsdfWork w;
  STCHK(esdf_workspace(e, n, &w));
  return esdf_launch(e, b, n, occupied_below, flags, w, (float*)d_out, (uint8_t*)d_state);
}

int ratsdf_esdf(ratsdf_engine* e, const int32_t origin[3], const int32_t dims[3], float occupied_below,
                uint32_t flags, float* out, uint8_t* state) {
  MapBox b;
  size_t n = 0;
  ENTRY(e, out && esdf_box(origin, dims, occupied_below, flags, &b, &n));
  STCHK(e->settle());
  STCHK(sticky_raised(e));
  EsdfWork w;
  STCHK(esdf_workspace(e, n, &w));
  STCHK(e->staging(0, kHostChunk));
  // the field lands in the x pass's buffer, dead once the y pass has run
  STCHK(esdf_launch(e, b, n, occupied_below, flags, w, (float*)w.gx, nullptr));
  STCHK(e->download(out, w.gx, n * sizeof(float)));
  if (state) STCHK(e->download(state, w.st, n));
  return e->sticky();
}

}  // extern "C"
