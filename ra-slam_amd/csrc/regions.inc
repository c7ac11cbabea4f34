// regions.inc -- connected regions of a box of the map (include/ratsdf_regions.h): the host side of
// kernels_regions.h.  Included at the end of ratsdf_engine.hip.

extern "C" {

static_assert(sizeof(ratsdf_region) == 32 && offsetof(ratsdf_region, lo) == 16 && offsetof(ratsdf_region, hi) == 22 &&
                  offsetof(ratsdf_region, reserved) == 28,
              "ratsdf_region layout");
static_assert(sizeof(ratsdf_regions_params) == 16, "ratsdf_regions_params layout");

// The workspace is EngineMem::ws_regions (RegionsWork, workspace.h), per voxel.  Its own buffer: a field of esdf.inc
// queued before or after shares nothing with it.

// argument checks of both entry points (RATSDF_ERR_BAD_ARGUMENT when false)
static bool regions_box(const int32_t* origin, const int32_t* dims, const ratsdf_regions_params* p, MapBox* b,
                        size_t* n) {
  return p && !std::isnan(p->min_prob) && !std::isnan(p->occupied_below) && p->states >= 1u && p->states <= 7u &&
         p->flags == 0u && map_box(origin, dims, b, n);
}

// seed, local pass, border merge, flatten and the scan of the root flags: labels in w.lab (and d_labels when it is
// not null), each root's rank in w.rank, the number of regions in *w.total
static int regions_label(ratsdf_engine* e, const MapBox& b, size_t n, const ratsdf_regions_params& p,
                         const RegionsWork& w, int32_t* d_labels) {
  hipLaunchKernelGGL(k_regions_seed, dim3((unsigned)box_cells(b)), dim3(256), 0, e->stream, e->tab, e->pool, b,
                     p.occupied_below, p.min_prob, p.states, w.st);
  HIPCHK(hipGetLastError());
  const int ntx = (b.X + kRegTX - 1) / kRegTX, nty = (b.Y + kRegTY - 1) / kRegTY, ntz = (b.Z + kRegTZ - 1) / kRegTZ;
  hipLaunchKernelGGL(k_regions_local, dim3((unsigned)ntx * (unsigned)nty * (unsigned)ntz), dim3(256), 0, e->stream,
                     (const uint8_t*)w.st, b.X, b.Y, b.Z, ntx, nty, w.lab);
  HIPCHK(hipGetLastError());
  const unsigned per_voxel = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(k_regions_merge, dim3(per_voxel), dim3(256), 0, e->stream, (const uint8_t*)w.st, b.X, b.Y, b.Z,
                     (uint32_t)n, w.lab);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_regions_flatten, dim3(per_voxel), dim3(256), 0, e->stream, w.lab, (uint32_t)n, d_labels,
                     w.rank);
  HIPCHK(hipGetLastError());
  // (in place: a thread of the scan's last kernel reads its four flags before it writes their positions)
  return scan_counts(e, w.rank, n, w.tiles, w.total, w.rank);
}

// the table: the first min(total, capacity) records at d_regions, the total as an int64 at d_count
static int regions_table(ratsdf_engine* e, const MapBox& b, size_t n, const RegionsWork& w, void* d_regions,
                         int64_t capacity, void* d_count) {
  // face adjacency leaves no more regions than every other voxel of a checkerboard
  const size_t most = std::min<size_t>((size_t)capacity, (n + 1) / 2);
  const unsigned per_record = (unsigned)std::max<size_t>((most + 255) / 256, 1);
  hipLaunchKernelGGL(k_regions_init, dim3(per_record), dim3(256), 0, e->stream, (uint4*)d_regions,
                     (const uint32_t*)w.total, (long long)capacity, (long long*)d_count);
  HIPCHK(hipGetLastError());
  if (capacity == 0) return RATSDF_OK;
  hipLaunchKernelGGL(k_regions_accumulate, dim3((unsigned)((n + kRegChunk - 1) / kRegChunk)), dim3(256), 0, e->stream,
                     (const uint8_t*)w.st, (const int32_t*)w.lab, (const uint32_t*)w.rank, b.X, b.Y, b.Z, (uint32_t)n,
                     (int32_t*)d_regions, (long long)capacity);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_regions_finish, dim3(per_record), dim3(256), 0, e->stream, (uint4*)d_regions,
                     (const uint32_t*)w.total, (long long)capacity, b);
  HIPCHK(hipGetLastError());
  return RATSDF_OK;
}

int ratsdf_regions_device(ratsdf_engine* e, const int32_t origin[3], const int32_t dims[3],
                          const ratsdf_regions_params* params, void* d_labels, void* d_regions, int64_t capacity,
                          void* d_count) {
  MapBox b;
  size_t n = 0;
  ENTRY(e, capacity >= 0 && (d_regions || capacity == 0) && !((uintptr_t)d_regions & 15u) &&
               !((uintptr_t)d_labels & 15u) && d_count && !((uintptr_t)d_count & 7u) &&
               regions_box(origin, dims, params, &b, &n));
  STCHK(box_entry(e));
  RegionsWork w;
  STCHK(e->workspace(e->ws_regions, n, regions_layout, &w));
  STCHK(regions_label(e, b, n, *params, w, (int32_t*)d_labels));
  return regions_table(e, b, n, w, d_regions, capacity, d_count);
}

int ratsdf_regions(ratsdf_engine* e, const int32_t origin[3], const int32_t dims[3],
                   const ratsdf_regions_params* params, int32_t* labels, ratsdf_region** out, size_t* n_out) {
  MapBox b;
  size_t n = 0;
  ENTRY(e, out && n_out && regions_box(origin, dims, params, &b, &n));
  STCHK(box_entry(e));
  RegionsWork w;
  STCHK(e->workspace(e->ws_regions, n, regions_layout, &w));
  STCHK(e->staging(0, kHostChunk));
  STCHK(regions_label(e, b, n, *params, w, nullptr));
  uint32_t total = 0;
  STCHK(e->read_small(&total, w.total, 4));
  *out = nullptr;  // (before the labels: a failed download of theirs leaves no table either)
  *n_out = 0;
  if (labels) STCHK(e->download(labels, w.lab, n * sizeof(int32_t)));
  const HostPart part = {total, sizeof(ratsdf_region), (void**)out, n_out};
  return hand_over(e, &part, 1, [&](uint8_t* const* d) {
    return regions_table(e, b, n, w, d[0], (int64_t)total, w.count);
  });
}

}  // extern "C"
