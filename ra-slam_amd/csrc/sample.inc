// sample.inc -- point sampling (include/ratsdf_sample.h): the host side of kernels_sample.h.  Included at the end of
// ratsdf_engine.hip.

extern "C" {

constexpr size_t kSampleChunk = (size_t)1 << 21;  // points per staged pass of the host entry point (88 MiB a side)
constexpr size_t kSampleRecord = 32, kSamplePoint = 12;

static int sample_launch(ratsdf_engine* e, const float* d_xyz, size_t n, void* d_out) {
  hipLaunchKernelGGL(k_sample, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e->stream, e->tab, e->pool, d_xyz,
                     (int)n, e->vs, (uint4*)d_out);
  HIPCHK(hipGetLastError());
  return RATSDF_OK;
}

int ratsdf_sample_points_device(ratsdf_engine* e, const void* d_xyz, size_t n, void* d_out) {
  ENTRY(e, (n == 0 || (d_xyz && d_out)) && n <= (size_t)INT32_MAX && !((uintptr_t)d_out & 15u) &&
               !((uintptr_t)d_xyz & 3u));
  STCHK(e->settle());
  STCHK(sticky_raised(e));
  if (n == 0) return RATSDF_OK;
  return sample_launch(e, (const float*)d_xyz, n, d_out);
}

int ratsdf_sample_points(ratsdf_engine* e, const float* xyz, size_t n, ratsdf_sample* out) {
  ENTRY(e, (n == 0 || (xyz && out)) && n <= (size_t)INT32_MAX);
  STCHK(e->settle());
  if (n == 0) return e->sticky();
  // points in and records out through the engine's staging pair, both sides laid out records | points for the chunk
  // asked for (the pair may hold more, and its sides may differ: other calls grow it too)
  const size_t chunk = std::min(n, kSampleChunk);
  STCHK(e->staging(chunk * (kSampleRecord + kSamplePoint), chunk * (kSampleRecord + kSamplePoint)));
  uint8_t* d_rec = e->d_out.as<uint8_t>();
  float* d_pts = (float*)(d_rec + chunk * kSampleRecord);
  uint8_t* h_rec = e->h_out.as<uint8_t>();
  float* h_pts = (float*)(h_rec + chunk * kSampleRecord);
  for (size_t o = 0; o < n; o += chunk) {
    const size_t m = std::min(chunk, n - o);
    memcpy(h_pts, xyz + 3 * o, m * kSamplePoint);
    HIPCHK(hipMemcpyAsync(d_pts, h_pts, m * kSamplePoint, hipMemcpyHostToDevice, e->stream));
    STCHK(sample_launch(e, d_pts, m, d_rec));
    HIPCHK(hipMemcpyAsync(h_rec, d_rec, m * kSampleRecord, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    memcpy(out + o, h_rec, m * kSampleRecord);
  }
  return e->sticky();
}

}  // extern "C"
