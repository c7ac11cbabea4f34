// blocks.inc -- blocks in and out of the map by position: the directory export and its delta, import and export of
// blocks with their voxels (multi-GPU seams), and the hooks the tests and tools drive the directory with
// (ratsdf_test_*, ratsdf_dump_*).  Included at the end of ratsdf_engine.hip.

extern "C" {

int ratsdf_export_directory_device(ratsdf_engine* e, void* d_blocks, int32_t capacity,
                                   void* d_count) {
  ENTRY(e, d_blocks && capacity >= 0);
  STCHK(e->settle());
  STCHK(e->select(kSelValid, GridBounds{}, &e->ctl->n_sel));
  hipLaunchKernelGGL(k_export_entries, dim3(256), dim3(256), 0, e->stream, e->vis, &e->ctl->n_sel,
                     (Entry*)d_blocks, (int32_t*)nullptr, (uint32_t)capacity, (int32_t*)d_count, e->ctl);
  HIPCHK(hipGetLastError());
  return RATSDF_OK;
}

// What the directory gained, changed and lost since the previous call (or since creation): the engine keeps a
// dirty bit per entry and a log of deleted positions (device_types.h: Table::dirty / del_log), so the delta costs
// two small kernels instead of a sort of the whole directory on the caller's side.  d_payload receives the
// added / changed entries first, then one entry {position, offset 0, idx -1} per deleted position; d_counts
// (int32[2]) the TRUE numbers of both -- more than `capacity` together means the payload was too small, and
// 0x7FFFFFFF deleted positions that the log overflowed: either way the caller takes a whole directory
// (ratsdf_export_directory_device) next.  A position deleted and inserted again is in both lists: drop, then add.
// d_payload == NULL: forget the changes so far (after a whole-directory export).  Asynchronous on the engine's stream.
int ratsdf_export_directory_delta_device(ratsdf_engine* e, void* d_payload, int32_t capacity, void* d_counts) {
  ENTRY(e, capacity >= 0 && (!d_payload || d_counts));
  STCHK(e->settle());
  const uint32_t occ_words = (e->tab.num_entry + 63) / 64;
  if (!e->tab.delta_on) {
    // The first call starts the bookkeeping (an engine nobody asks for deltas keeps none: a dirty-bit atomic per
    // commit and the delete log cost the frame 0.9 us).  Nothing has been recorded so far, so this call cannot
    // deliver a delta: a payload call reports the overflow value and the caller takes a whole directory.
    HIPCHK(hipStreamSynchronize(e->stream));
    e->tab.delta_on = 1;
    STCHK(e->upload_record());
    HIPCHK(hipMemsetAsync(e->tab.occ + occ_words, 0, (size_t)occ_words * 8, e->stream));
    HIPCHK(hipMemsetAsync(e->tab.del_count, 0, 4, e->stream));
    if (d_payload) {
      const int32_t unusable[2] = {0, 0x7FFFFFFF};
      HIPCHK(hipMemcpyAsync(d_counts, unusable, 8, hipMemcpyHostToDevice, e->stream));
      HIPCHK(hipStreamSynchronize(e->stream));
    }
    return RATSDF_OK;
  }
  if (!d_payload) {
    HIPCHK(hipMemsetAsync(e->tab.occ + occ_words, 0, (size_t)occ_words * 8, e->stream));
    HIPCHK(hipMemsetAsync(e->tab.del_count, 0, 4, e->stream));
    return RATSDF_OK;
  }
  HIPCHK(hipMemsetAsync(d_counts, 0, 8, e->stream));
  hipLaunchKernelGGL(k_delta_added, dim3(e->nwg), dim3(kVisWG), 0, e->stream, e->tab, (Entry*)d_payload,
                     (uint32_t)capacity, (uint32_t*)d_counts);
  hipLaunchKernelGGL(k_delta_deleted, dim3(64), dim3(256), 0, e->stream, e->tab, (Entry*)d_payload,
                     (uint32_t)capacity, (uint32_t*)d_counts);
  hipLaunchKernelGGL(k_delta_reset, dim3(1), dim3(1), 0, e->stream, e->tab);
  HIPCHK(hipGetLastError());
  return RATSDF_OK;
}

// ---- test hooks ------------------------------------------------------------------------------
static int upload_s3(ratsdf_engine* e, const int16_t* src, int32_t n, DevMem* dev) {
  if (n == 0) return RATSDF_OK;
  STCHK(dev->alloc((size_t)n * 6));
  HIPCHK(hipMemcpyAsync(dev->as<void>(), src, (size_t)n * 6, hipMemcpyHostToDevice, e->stream));
  return RATSDF_OK;
}

int ratsdf_test_allocate(ratsdf_engine* e, const int16_t* bp, int32_t n) {
  ENTRY(e, n >= 0 && (n == 0 || bp));
  STCHK(e->settle());
  if (n == 0) return e->sticky();
  STCHK(e->ensure_image(0, (size_t)n));
  DevMem d_bp;
  StreamDrain drain{e->stream};
  STCHK(upload_s3(e, bp, n, &d_bp));
  const int16_t* d = d_bp.as<int16_t>();
  FrameParams P = e->base_params();
  const uint32_t par = e->parity;  // an allocation pass of its own in the next frame's counters
  hipLaunchKernelGGL(k_alloc_list, dim3((n + 255) / 256), dim3(256), 0, e->stream, e->tab, P, d, n,
                     e->req, e->req_cap, e->slow, kSlowCap, e->ctl, par);
  STCHK(e->commit_pass((uint32_t)n, par));
  return e->sticky();
}

// The blocks at d_pos (device, n x 3 int16) into the directory -- whatever the engine's shard filter says -- and
// their voxels from device arrays laid out as k_import_voxels describes.  Synchronises the engine's stream (the number
// of blocks the directory still lacks after a pass is read back: control data, 4 bytes per pass).
static int import_from_device(ratsdf_engine* e, int32_t n, const int16_t* d_pos, const float* d_tsdf,
                              const uint32_t* d_rgbw, const float* d_prob, uint32_t stride) {
  e->ever_sem = true;  // (the blocks come with their probabilities: FrameParams::segm_live)
  STCHK(e->ensure_image(0, (size_t)n));
  DevMem missing_mem;
  StreamDrain drain{e->stream};
  STCHK(missing_mem.alloc(4));
  uint32_t* const d_missing = missing_mem.as<uint32_t>();
  FrameParams P = e->base_params();
  P.shard_count = 1;  // whatever the engine's shard filter says
  uint32_t missing = (uint32_t)n;
  // an insertion can lose its bucket to another one of the same pass (one per bucket and pass,
  // voxel_hash.cu:67-78): allocate, copy, and go again for whatever the directory still lacks
  for (int pass = 0; pass < 8 && missing != 0; ++pass) {
    const uint32_t par = e->parity;
    hipLaunchKernelGGL(k_alloc_list, dim3((n + 255) / 256), dim3(256), 0, e->stream, e->tab, P, d_pos, n, e->req,
                       e->req_cap, e->slow, kSlowCap, e->ctl, par);
    STCHK(e->commit_pass((uint32_t)n, par));
    HIPCHK(hipMemsetAsync(d_missing, 0, 4, e->stream));
    hipLaunchKernelGGL(k_import_voxels, dim3((n + 3) / 4), dim3(256), 0, e->stream, e->tab, e->pool, d_pos, n, d_tsdf,
                       d_rgbw, d_prob, stride, d_missing);
    HIPCHK(hipMemcpyAsync(&missing, d_missing, 4, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
  }
  STCHK(e->sticky());
  return missing != 0 ? RATSDF_ERR_CAPACITY : RATSDF_OK;
}

int ratsdf_import_blocks(ratsdf_engine* e, int32_t n, const int16_t* bp, const float* tsdf, const ratsdf_rgbw* rgbw,
                         const float* prob) {
  ENTRY(e, n >= 0 && (n == 0 || (bp && tsdf && rgbw && prob)));
  STCHK(e->settle());
  if (n == 0) return e->sticky();
  DevMem pos_mem, vox_mem;
  StreamDrain drain{e->stream};
  const size_t per = (size_t)n * 512 * 4;
  STCHK(upload_s3(e, bp, n, &pos_mem));
  STCHK(vox_mem.alloc(per * 3));
  const int16_t* d_pos = pos_mem.as<int16_t>();
  uint8_t* d_vox = vox_mem.as<uint8_t>();
  HIPCHK(hipMemcpyAsync(d_vox, tsdf, per, hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipMemcpyAsync(d_vox + per, rgbw, per, hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipMemcpyAsync(d_vox + 2 * per, prob, per, hipMemcpyHostToDevice, e->stream));
  return import_from_device(e, n, d_pos, (const float*)d_vox, (const uint32_t*)(d_vox + per),
                            (const float*)(d_vox + 2 * per), 512u);
}

int ratsdf_import_blocks_device(ratsdf_engine* e, int32_t n, const void* d_block_pos, const void* d_voxels) {
  ENTRY(e, n >= 0 && (n == 0 || (d_block_pos && d_voxels)));
  STCHK(e->settle());
  if (n == 0) return e->sticky();
  const uint32_t* rec = (const uint32_t*)d_voxels;
  return import_from_device(e, n, (const int16_t*)d_block_pos, (const float*)rec, rec + 512, (const float*)(rec + 1024),
                            1536u);
}

int ratsdf_export_blocks_device(ratsdf_engine* e, int32_t n, const void* d_block_pos, void* d_voxels,
                                void* d_missing) {
  ENTRY(e, n >= 0 && d_missing && (n == 0 || (d_block_pos && d_voxels)));
  STCHK(e->settle());
  HIPCHK(hipMemsetAsync(d_missing, 0, 4, e->stream));
  if (n == 0) return RATSDF_OK;
  hipLaunchKernelGGL(k_export_blocks, dim3((n + 3) / 4), dim3(256), 0, e->stream, e->tab, e->pool,
                     (const int16_t*)d_block_pos, n, (uint32_t*)d_voxels, (uint32_t*)d_missing);
  HIPCHK(hipGetLastError());
  return RATSDF_OK;
}

int ratsdf_test_delete(ratsdf_engine* e, const int16_t* bp, int32_t n) {
  ENTRY(e, n >= 0 && (n == 0 || bp));
  STCHK(e->settle());
  // keep the first occurrence of every position (a repeated Delete is a no-op in list order)
  std::vector<int16_t> uniq;
  uniq.reserve((size_t)n * 3);
  for (int i = 0; i < n; ++i) {
    bool dup = false;
    for (size_t j = 0; j + 2 < uniq.size() && !dup; j += 3)
      dup = uniq[j] == bp[3 * i] && uniq[j + 1] == bp[3 * i + 1] && uniq[j + 2] == bp[3 * i + 2];
    if (!dup) uniq.insert(uniq.end(), bp + 3 * i, bp + 3 * i + 3);
  }
  const int32_t m = (int32_t)(uniq.size() / 3);
  if (m == 0) return e->sticky();
  if (m > e->tab.num_block) return RATSDF_ERR_BAD_ARGUMENT;
  DevMem d_bp;
  STCHK(upload_s3(e, uniq.data(), m, &d_bp));
  const int16_t* d = d_bp.as<int16_t>();
  const uint32_t par = e->parity;
  hipLaunchKernelGGL(k_delete_list, dim3((m + 255) / 256), dim3(256), 0, e->stream, e->tab, d, m,
                     e->carve_bufs(par), e->ctl, par);
  hipLaunchKernelGGL(k_settle, dim3(1), dim3(1024), 0, e->stream, e->tab, e->pool, e->carve_bufs(par),
                     e->ctl, par, (ratsdf_frame_stats*)nullptr);
  return e->sticky();  // (synchronises: nothing queued outlives the uploaded list)
}

int ratsdf_test_retrieve(ratsdf_engine* e, const int16_t* pts, int32_t n, ratsdf_rgbw* rgbw,
                         float* tsdf, float* prob, ratsdf_block* blocks) {
  ENTRY(e, n >= 0 && (n == 0 || pts));
  STCHK(e->settle());
  if (n == 0) return RATSDF_OK;
  DevMem d_pts, d_res;
  StreamDrain drain{e->stream};
  STCHK(upload_s3(e, pts, n, &d_pts));
  STCHK(d_res.alloc((size_t)n * 24));
  const int16_t* d = d_pts.as<int16_t>();
  uint8_t* o = d_res.as<uint8_t>();
  uint32_t* o_rgbw = (uint32_t*)o;
  float* o_tsdf = (float*)(o + (size_t)n * 4);
  float* o_prob = (float*)(o + (size_t)n * 8);
  Entry* o_blk = (Entry*)(o + (size_t)n * 12);
  hipLaunchKernelGGL(k_retrieve, dim3((n + 255) / 256), dim3(256), 0, e->stream, e->tab, e->pool, d,
                     n, o_rgbw, o_tsdf, o_prob, o_blk);
  std::vector<uint8_t> h((size_t)n * 24);
  HIPCHK(hipMemcpyAsync(h.data(), o, h.size(), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  if (rgbw) memcpy(rgbw, h.data(), (size_t)n * 4);
  if (tsdf) memcpy(tsdf, h.data() + (size_t)n * 4, (size_t)n * 4);
  if (prob) memcpy(prob, h.data() + (size_t)n * 8, (size_t)n * 4);
  if (blocks) memcpy(blocks, h.data() + (size_t)n * 12, (size_t)n * 12);
  return RATSDF_OK;
}

int ratsdf_test_assign_rgbw(ratsdf_engine* e, const int16_t* pts, const ratsdf_rgbw* vals,
                            int32_t n) {
  ENTRY(e, n >= 0 && (n == 0 || (pts && vals)));
  STCHK(e->settle());
  if (n == 0) return RATSDF_OK;
  DevMem d_pts, d_vals;
  StreamDrain drain{e->stream};
  STCHK(upload_s3(e, pts, n, &d_pts));
  STCHK(d_vals.alloc((size_t)n * 4));
  const int16_t* d = d_pts.as<int16_t>();
  uint32_t* v = d_vals.as<uint32_t>();
  HIPCHK(hipMemcpyAsync(v, vals, (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
  hipLaunchKernelGGL(k_assign_rgbw, dim3((n + 255) / 256), dim3(256), 0, e->stream, e->tab, e->pool,
                     d, v, n);
  HIPCHK(hipStreamSynchronize(e->stream));
  return RATSDF_OK;
}

// the `cnt` entries selected into e->vis, as blocks and entry indices in host arrays; returns with the stream drained
static int dump_selected_entries(ratsdf_engine* e, uint32_t cnt, ratsdf_block* bl, int32_t* ei) {
  DevMem b_mem, e_mem;
  StreamDrain drain{e->stream};
  STCHK(b_mem.alloc((size_t)cnt * 12));
  STCHK(e_mem.alloc((size_t)cnt * 4));
  Entry* d_b = b_mem.as<Entry>();
  int32_t* d_e = e_mem.as<int32_t>();
  hipLaunchKernelGGL(k_export_entries, dim3(256), dim3(256), 0, e->stream, e->vis, &e->ctl->n_sel,
                     d_b, d_e, cnt, (int32_t*)nullptr, (Ctl*)nullptr);
  HIPCHK(hipMemcpyAsync(bl, d_b, (size_t)cnt * 12, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipMemcpyAsync(ei, d_e, (size_t)cnt * 4, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return RATSDF_OK;
}

int ratsdf_dump_directory(ratsdf_engine* e, int32_t** entry_index, ratsdf_block** blocks,
                          size_t* n) {
  ENTRY(e, entry_index && blocks && n);
  STCHK(e->settle());
  STCHK(e->select(kSelValid, GridBounds{}, &e->ctl->n_sel));
  uint32_t cnt = 0;
  HIPCHK(hipMemcpyAsync(&cnt, &e->ctl->n_sel, 4, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  // the caller owns both arrays (ratsdf_free_buffer) -- once the call has succeeded
  int32_t* ei = (int32_t*)malloc(cnt ? (size_t)cnt * 4 : 1);
  ratsdf_block* bl = (ratsdf_block*)malloc(cnt ? (size_t)cnt * 12 : 1);
  int st = ei && bl ? RATSDF_OK : RATSDF_ERR_DEVICE;
  if (st == RATSDF_OK && cnt) st = dump_selected_entries(e, cnt, bl, ei);
  if (st != RATSDF_OK) {
    free(ei);
    free(bl);
    return st;
  }
  *entry_index = ei;
  *blocks = bl;
  *n = cnt;
  return RATSDF_OK;
}

int ratsdf_dump_voxels(ratsdf_engine* e, const int32_t* pool_idx, int32_t n, float* tsdf,
                       ratsdf_rgbw* rgbw, float* prob) {
  ENTRY(e, n >= 0 && (n == 0 || pool_idx));
  STCHK(e->settle());
  if (n == 0) return RATSDF_OK;
  for (int i = 0; i < n; ++i)
    if (pool_idx[i] < 0 || pool_idx[i] >= e->tab.num_block) return RATSDF_ERR_BAD_ARGUMENT;
  DevMem idx_mem, out_mem;
  StreamDrain drain{e->stream};
  const size_t per = (size_t)n * 512 * 4;
  STCHK(idx_mem.alloc((size_t)n * 4));
  STCHK(out_mem.alloc(per * 3));
  int32_t* d_idx = idx_mem.as<int32_t>();
  uint8_t* d_out = out_mem.as<uint8_t>();
  HIPCHK(hipMemcpyAsync(d_idx, pool_idx, (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
  hipLaunchKernelGGL(k_gather_voxels, dim3((n + 3) / 4), dim3(256), 0, e->stream, e->pool, d_idx, n,
                     (float*)d_out, (uint32_t*)(d_out + per), (float*)(d_out + 2 * per));
  if (tsdf) HIPCHK(hipMemcpyAsync(tsdf, d_out, per, hipMemcpyDeviceToHost, e->stream));
  if (rgbw) HIPCHK(hipMemcpyAsync(rgbw, d_out + per, per, hipMemcpyDeviceToHost, e->stream));
  if (prob) HIPCHK(hipMemcpyAsync(prob, d_out + 2 * per, per, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return RATSDF_OK;
}

int ratsdf_dump_heap(ratsdf_engine* e, int32_t* num_free, int32_t* heap) {
  ENTRY(e, true);
  STCHK(e->settle());
  if (num_free)
    HIPCHK(hipMemcpyAsync(num_free, &e->ctl->num_free, 4, hipMemcpyDeviceToHost, e->stream));
  if (heap)
    HIPCHK(hipMemcpyAsync(heap, e->pool.heap, (size_t)e->tab.num_block * 4, hipMemcpyDeviceToHost,
                          e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return RATSDF_OK;
}

}  // extern "C"
