// query.inc -- reading the map out: ratsdf_query and the gathers of valid blocks (voxel records, the marching-cubes
// mesh), their file forms, and the ray cast.  Included at the end of ratsdf_engine.hip.  Every call settles first, selects
// into the engine's `vis` buffer and copies out through the engine's staging pair (ratsdf_engine::staging).

extern "C" {

static int download_selected(ratsdf_engine* e, bool semantic, void** out, size_t* n) {
  uint32_t cnt = 0;
  STCHK(e->read_small(&cnt, &e->ctl->n_sel, 4));
  // (the read waited for the stream: a device error of an earlier frame is known by now, and ratsdf.h has every
  // query report it -- the records of a map that lost a frame's blocks must not pass for the map)
  STCHK(sticky_raised(e));
  const size_t rec = semantic ? sizeof(ratsdf_voxel_segm) : sizeof(ratsdf_voxel_tsdf);
  const size_t total = (size_t)cnt * RATSDF_BLOCK_VOLUME;
  void* host = malloc(total ? total * rec : 1);
  if (!host) return RATSDF_ERR_DEVICE;
  if (total) {
    // the staging pair: a side that has to grow grows by a quarter more, so a map that gains a few blocks between
    // gathers does not reallocate every time (a hipMalloc / hipFree pair per Query costs more than the kernels)
    const size_t bytes = total * rec, more = bytes + bytes / 4;
    const int st = e->staging(bytes <= e->d_out.size() ? bytes : more, bytes <= e->h_out.size() ? bytes : more);
    if (st != RATSDF_OK) {
      free(host);
      return st;
    }
    float* dev = e->d_out.as<float>();
    const uint8_t* h = e->h_out.as<uint8_t>();
    const unsigned grid = cnt < 4096u ? (cnt + 3) / 4 : 1024u;
    if (semantic)
      hipLaunchKernelGGL(k_download<true>, dim3(grid), dim3(256), 0, e->stream, e->pool, e->vis,
                         &e->ctl->n_sel, e->vs, dev);
    else
      hipLaunchKernelGGL(k_download<false>, dim3(grid), dim3(256), 0, e->stream, e->pool, e->vis,
                         &e->ctl->n_sel, e->vs, dev);
    hipError_t err = hipMemcpyAsync(e->h_out.as<void>(), dev, bytes, hipMemcpyDeviceToHost, e->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
    if (err != hipSuccess) {
      free(host);
      return RATSDF_ERR_DEVICE;
    }
    // the caller owns `host` (ratsdf_free_buffer).  A large result is copied out by the engine's helper threads side
    // by side: the destination is fresh memory, and first-touch page faults (10 k of them for the 41 MB of a
    // GatherValid on the bench map) are what the single-threaded copy spent most of its time on
    HostCopyPool* cp = bytes >= ((size_t)4 << 20) ? e->ring.copy_pool() : nullptr;
    if (cp) {
      HostCopyPool::Piece pieces[16];
      int np = 0;
      const size_t step = ((bytes + 15) / 16 + 4095) & ~(size_t)4095;
      for (size_t o = 0; o < bytes; o += step)
        pieces[np++] = HostCopyPool::Piece{(uint8_t*)host + o, h + o, std::min(step, bytes - o)};
      cp->copy(pieces, np);
    } else {
      memcpy(host, h, bytes);
    }
  }
  *out = host;
  *n = total;
  return RATSDF_OK;
}

static inline int16_t host_f2s(float f) {  // static_cast<short>, BoundingCube::Scale
  if (f != f) return 0;
  if (f >= 2147483648.f) return (int16_t)2147483647;
  if (f <= -2147483648.f) return (int16_t)(-2147483647 - 1);
  return (int16_t)(int)f;
}

int ratsdf_query(ratsdf_engine* e, const ratsdf_bounds* b, ratsdf_voxel_tsdf** out, size_t* n) {
  ENTRY(e, b && out && n);
  STCHK(e->settle());
  const float scale = (float)(1. / e->vs);  // volumn.Scale<short>(1. / voxel_size_), voxel_tsdf.cu:534
  GridBounds gb{host_f2s(b->xmin * scale), host_f2s(b->xmax * scale), host_f2s(b->ymin * scale),
                host_f2s(b->ymax * scale), host_f2s(b->zmin * scale), host_f2s(b->zmax * scale)};
  STCHK(e->select(kSelBounds, gb, &e->ctl->n_sel));
  return download_selected(e, false, (void**)out, n);
}

int ratsdf_gather_valid(ratsdf_engine* e, ratsdf_voxel_tsdf** out, size_t* n) {
  ENTRY(e, out && n);
  STCHK(e->settle());
  STCHK(e->select(kSelValid, GridBounds{}, &e->ctl->n_sel));
  return download_selected(e, false, (void**)out, n);
}

int ratsdf_gather_valid_semantic(ratsdf_engine* e, ratsdf_voxel_segm** out, size_t* n) {
  ENTRY(e, out && n);
  STCHK(e->settle());
  STCHK(e->select(kSelValid, GridBounds{}, &e->ctl->n_sel));
  return download_selected(e, true, (void**)out, n);
}

int ratsdf_download_all(ratsdf_engine* e, const char* path) {
  ENTRY(e, path);
  STCHK(e->settle());
  ratsdf_voxel_segm* buf = nullptr;
  size_t n = 0;
  STCHK(ratsdf_gather_valid_semantic(e, &buf, &n));
  FILE* f = fopen(path, "wb");
  if (!f) {
    free(buf);
    return RATSDF_ERR_BAD_ARGUMENT;
  }
  fwrite(buf, sizeof(ratsdf_voxel_segm), n, f);
  fclose(f);
  free(buf);
  return RATSDF_OK;
}

int ratsdf_free_buffer(void* p) {
  free(p);
  return RATSDF_OK;
}

// rows [row0, row1) of the height x width rendering into device buffers that hold those rows (`e`: checked by ENTRY)
static int raycast_rows_device(ratsdf_engine* e, const ratsdf_intrinsics* K, int height, int width,
                               const ratsdf_pose* T, float max_depth, int row0, int row1, void* d_rgba,
                               void* d_normal) {
  if (!K || !T || height <= 0 || width <= 0 || !(max_depth > 0) || row0 < 0 || row1 > height || row0 > row1)
    return RATSDF_ERR_BAD_ARGUMENT;
  STCHK(e->settle());
  if (row0 == row1) return RATSDF_OK;
  FrameParams P = e->base_params();
  P.T = Se3{Quat{T->qx, T->qy, T->qz, T->qw}, V3{T->tx, T->ty, T->tz}};
  P.Ti = se3_inverse(P.T);                      // voxel_tsdf.cu:892 cam_T_world.Inverse()
  P.K = Intr{K->fx, K->fy, K->cx, K->cy};
  P.Ki = intr_inverse(P.K);
  P.W = width;
  P.H = height;
  const float step_size = e->trunc / 2;         // voxel_tsdf.cu:892
  const float ms = ceilf(max_depth / step_size);
  const int max_step = ms >= 2147483648.f ? 2147483647 : (int)ms;  // voxel_tsdf.cu:298
  // block-level occupancy of the map as it is now (kernels_raycast.h: empty space costs no directory probes)
  STCHK(e->d_occ.grow((kOccWords + kCellWords) * 4));
  uint32_t* const d_occ = e->d_occ.as<uint32_t>();
  HIPCHK(hipMemsetAsync(d_occ, 0, (kOccWords + kCellWords) * 4, e->stream));
  hipLaunchKernelGGL(k_occupancy_build, dim3(256), dim3(256), 0, e->stream, e->tab, (const Ctl*)e->ctl, d_occ);
  hipLaunchKernelGGL(k_raycast, dim3((width + 15) / 16, (row1 - row0 + 15) / 16), dim3(256), 0, e->stream,
                     e->tab, e->pool, P, step_size, max_step, (uint32_t*)d_rgba, (uint32_t*)d_normal, row0, row1,
                     (const uint32_t*)d_occ, e->ctl);
  HIPCHK(hipGetLastError());
  return RATSDF_OK;
}

int ratsdf_raycast_device(ratsdf_engine* e, const ratsdf_intrinsics* K, int height, int width,
                          const ratsdf_pose* T, float max_depth, void* d_rgba, void* d_normal) {
  ENTRY(e, true);  // (the arguments: raycast_rows_device)
  return raycast_rows_device(e, K, height, width, T, max_depth, 0, height, d_rgba, d_normal);
}

int ratsdf_raycast_rows(ratsdf_engine* e, const ratsdf_intrinsics* K, int height, int width,
                        const ratsdf_pose* T, float max_depth, int row0, int row1, uint8_t* rgba, uint8_t* normal) {
  ENTRY(e, height > 0 && width > 0 && row0 >= 0 && row1 <= height && row0 <= row1);  // (K, T, max_depth: raycast_rows_device)
  const size_t bytes = (size_t)(row1 - row0) * width * 4;
  if (bytes == 0) return raycast_rows_device(e, K, height, width, T, max_depth, row0, row1, nullptr, nullptr);
  // The two images leave through the engine's staging pair, in one copy: device memory for the kernel's output and
  // page-locked host memory for the copy out (until round 5: a hipMalloc / hipFree pair per call and two copies into the
  // caller's pageable buffers through the runtime's staging path -- 0.84 ms per 640x480 rendering of which the kernel was half).
  STCHK(e->staging(bytes * 2, bytes * 2));
  uint8_t* d = e->d_out.as<uint8_t>();
  uint8_t* h = e->h_out.as<uint8_t>();
  STCHK(raycast_rows_device(e, K, height, width, T, max_depth, row0, row1, d, d + bytes));
  HIPCHK(hipMemcpyAsync(h, d, bytes * 2, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));  // voxel_tsdf.cu:901
  if (rgba) memcpy(rgba, h, bytes);
  if (normal) memcpy(normal, h + bytes, bytes);
  return RATSDF_OK;
}

int ratsdf_raycast(ratsdf_engine* e, const ratsdf_intrinsics* K, int height, int width,
                   const ratsdf_pose* T, float max_depth, uint8_t* rgba, uint8_t* normal) {
  return ratsdf_raycast_rows(e, K, height, width, T, max_depth, 0, height, rgba, normal);
}

int ratsdf_gather_valid_mesh(ratsdf_engine* e, float** vertices, size_t* n_vertices,
                             int32_t** indices, size_t* n_triangles, float** vertex_prob) {
  ENTRY(e, vertices && n_vertices && indices && n_triangles && vertex_prob);
  STCHK(e->settle());
  // check_valid_kernel + GatherBlock; a sharded map meshes the blocks it owns (imported neighbours are read only)
  STCHK(e->select(e->shard_count > 1 ? kSelOwned : kSelValid, GridBounds{}, &e->ctl->n_sel));
  uint32_t nb = 0;
  STCHK(e->read_small(&nb, &e->ctl->n_sel, 4));
  // the caller owns the three arrays (ratsdf_free_buffer): placeholders while the mesh is empty or the call fails
  *vertices = (float*)malloc(4);
  *vertex_prob = (float*)malloc(4);
  *indices = (int32_t*)malloc(4);
  *n_vertices = 0;
  *n_triangles = 0;
  if (!*vertices || !*vertex_prob || !*indices) return RATSDF_ERR_DEVICE;
  if (nb == 0) return RATSDF_OK;
  const size_t nvs = (size_t)nb * kVertVolume * 3;  // candidate vertices
  const size_t nts = (size_t)nb * 512 * 5;          // candidate triangles
  if (!e->d_mc) {
    const McTables h = make_mc_tables();
    DevMem mc;  // (the engine keeps tables that have arrived, nothing else)
    STCHK(mc.alloc(sizeof(McTables)));
    HIPCHK(hipMemcpy(mc.as<void>(), &h, sizeof(McTables), hipMemcpyHostToDevice));
    e->d_mc = std::move(mc);
  }
  // one scratch allocation: verts | vprob | vmask | vpos | tids | tmask | tpos | tile sums | total
  const size_t ntile_max = scan_tiles((nts > nvs ? nts : nvs) + 1) + 1;
  const size_t bytes = nvs * 12 + nvs * 4 * 3 + nts * 12 + nts * 4 * 2 + ntile_max * 4 + 64;
  DevMem d;  // the scratch (the compacted mesh leaves through the staging pair)
  StreamDrain drain{e->stream};
  STCHK(d.alloc(bytes));
  float* verts = d.as<float>();
  float* vprob = verts + nvs * 3;
  uint32_t* vmask = (uint32_t*)(vprob + nvs);
  uint32_t* vpos = vmask + nvs;
  int32_t* tids = (int32_t*)(vpos + nvs);
  uint32_t* tmask = (uint32_t*)(tids + nts * 3);
  uint32_t* tpos = tmask + nts;
  uint32_t* tiles = tpos + nts;
  uint32_t* d_total = tiles + ntile_max;
  hipLaunchKernelGGL(k_marching_cubes, dim3(nb), dim3(512), 0, e->stream, e->tab, e->pool, e->vis,
                     e->d_mc.as<const McTables>(), e->vs, verts, vprob, vmask, tids, tmask);
  uint32_t nv = 0, nt = 0;
  STCHK(mask_positions(e, vmask, nvs, vpos, tiles, d_total, &nv));
  STCHK(mask_positions(e, tmask, nts, tpos, tiles, d_total, &nt));
  const size_t out_bytes = (size_t)nv * 16 + (size_t)nt * 12 + 64;
  STCHK(e->staging(out_bytes, std::min(out_bytes, kHostChunk)));
  float* ov = e->d_out.as<float>();
  float* op = ov + (size_t)nv * 3;
  int32_t* oi = (int32_t*)(op + nv);
  hipLaunchKernelGGL(k_compact_vertices, dim3(2048), dim3(256), 0, e->stream, verts, vprob, vmask,
                     vpos, nvs, ov, op);
  hipLaunchKernelGGL(k_compact_triangles, dim3(2048), dim3(256), 0, e->stream, tids, tmask, tpos,
                     vpos, nts, oi);
  HIPCHK(hipGetLastError());
  void* const hv = realloc(*vertices, (size_t)nv * 12 + 4);  // (a failed realloc leaves the placeholder)
  void* const hp = realloc(*vertex_prob, (size_t)nv * 4 + 4);
  void* const hi = realloc(*indices, (size_t)nt * 12 + 4);
  if (hv) *vertices = (float*)hv;
  if (hp) *vertex_prob = (float*)hp;
  if (hi) *indices = (int32_t*)hi;
  if (!hv || !hp || !hi) return RATSDF_ERR_DEVICE;
  STCHK(e->download(hv, ov, (size_t)nv * 12));
  STCHK(e->download(hp, op, (size_t)nv * 4));
  STCHK(e->download(hi, oi, (size_t)nt * 12));
  *n_vertices = nv;
  *n_triangles = nt;
  return RATSDF_OK;
}

int ratsdf_download_all_mesh(ratsdf_engine* e, const char* vp, const char* ip, const char* pp) {
  ENTRY(e, vp && ip && pp);
  float *v = nullptr, *pr = nullptr;
  int32_t* idx = nullptr;
  size_t nv = 0, nt = 0;
  int st = ratsdf_gather_valid_mesh(e, &v, &nv, &idx, &nt, &pr);
  if (st == RATSDF_OK) {  // modules/tsdf_module.cc:66-86
    FILE* fv = fopen(vp, "wb");
    FILE* fp = fopen(pp, "wb");
    FILE* fi = fopen(ip, "wb");
    if (fv && fp && fi) {
      fwrite(v, 12, nv, fv);
      fwrite(pr, 4, nv, fp);
      fwrite(idx, 12, nt, fi);
    } else {
      st = RATSDF_ERR_BAD_ARGUMENT;
    }
    if (fv) fclose(fv);
    if (fp) fclose(fp);
    if (fi) fclose(fi);
  }
  free(v);
  free(pr);
  free(idx);
  return st;
}

}  // extern "C"
