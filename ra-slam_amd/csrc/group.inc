// group.inc -- engine groups (ratsdf_group_* of include/ratsdf.h).  Included at the end of ratsdf_engine.hip (it
// launches through enqueue_jobs).
//
// Several engines (maps) of one device stepped together: frame i of every member stream goes through
// ONE k_front / k_alloc_rank / k_integrate triple whose grids have one slice per engine (blockIdx.y).
// A single 640x480 frame leaves most of the chip waiting on memory round trips and launch ramps; S
// frames per launch fill it.  Operands come from device tables: the engine records (device_types.h:
// EngineDev) and a per-batch table of FrameJob {parameters, image pointers, parity} per frame and slot.
struct ratsdf_group {
  int device = 0;
  int S = 0;
  std::vector<ratsdf_engine*> eng;
  int split_a = 100, split_b = 0;  // look-ahead share of k_front / k_alloc_rank (rest: k_integrate)
  // What the group owns leaves in the reverse of these declarations, behind the drain of its stream: the device
  // tables, their page-locked staging, the events, the timer's events, the stream.
  HipStream stream;
  KernelTimer timer;  // (mode 1: every fourth frame)
  HipEvent ev_done;                 // group stream -> member streams
  std::vector<HipEvent> ev_member;  // member stream -> group stream
  // page-locked staging of both tables, EngineDev[S] | FrameJob[frames of a batch x S]: two sides used alternately (a
  // copy may still be pending when the next batch is being prepared), one event per side behind both copies
  TwinTable tables;
  DevMem d_engs, d_jobs;  // EngineDev[S]; FrameJob[frames of a batch x S], grown on demand
  size_t jobs_off() const { return ((size_t)S * sizeof(EngineDev) + 255) & ~(size_t)255; }

  ~ratsdf_group() {
    if (stream) (void)hipStreamSynchronize(stream);
  }
};

extern "C" {

int ratsdf_group_create(ratsdf_engine* const* engines, int n, ratsdf_group** out) {
  if (!engines || !out || n < 1 || n > 64) return RATSDF_ERR_BAD_ARGUMENT;
  for (int i = 0; i < n; ++i) {
    const ratsdf_engine* a = engines[i];
    if (!a) return RATSDF_ERR_BAD_ARGUMENT;
    const ratsdf_engine* b = engines[0];
    // one launch geometry for all members
    if (a->device != b->device || a->vs != b->vs || a->trunc != b->trunc ||
        a->block_bits != b->block_bits || a->bucket_bits != b->bucket_bits || a->vpl != b->vpl)
      return RATSDF_ERR_BAD_ARGUMENT;
    for (int j = 0; j < i; ++j)
      if (engines[j] == a) return RATSDF_ERR_BAD_ARGUMENT;
  }
  DeviceGuard guard(engines[0]->device);  // (not ENTRY: there is no group yet, the device is the members')
  if (!guard.ok()) return RATSDF_ERR_DEVICE;
  ratsdf_group* g = new (std::nothrow) ratsdf_group();
  if (!g) return RATSDF_ERR_DEVICE;
  g->device = engines[0]->device;
  g->S = n;
  g->eng.assign(engines, engines + n);
  g->ev_member.resize((size_t)n);
#ifdef RATSDF_STAMPS
  if (const char* v = getenv("RATSDF_GROUP_SPLIT")) {  // "a[,b]" like RATSDF_CAND_SPLIT
    const int x = atoi(v);
    if (x >= 0 && x <= 100) {
      g->split_a = x;
      g->split_b = 0;
      if (const char* c = strchr(v, ',')) {
        const int y = atoi(c + 1);
        if (y >= 0 && x + y <= 100) g->split_b = y;
      }
    }
  }
#endif
#define GROUP_CHK(expr)                                                  \
  do {                                                                   \
    if ((expr) != hipSuccess) {                                          \
      fprintf(stderr, "[ratsdf] group create failed: %s\n", #expr);      \
      delete g;                                                          \
      return RATSDF_ERR_DEVICE;                                          \
    }                                                                    \
  } while (0)
  GROUP_CHK(g->stream.create(hipStreamNonBlocking));
  GROUP_CHK(g->d_engs.alloc((size_t)n * sizeof(EngineDev)));
  GROUP_CHK(g->tables.grow(g->jobs_off()));
  for (HipEvent& ev : g->ev_member) GROUP_CHK(ev.create(hipEventDisableTiming));
  GROUP_CHK(g->ev_done.create(hipEventDisableTiming));
#undef GROUP_CHK
  *out = g;
  return RATSDF_OK;
}

int ratsdf_group_destroy(ratsdf_group* g) {
  ENTRY(g, true);
  delete g;
  return RATSDF_OK;
}

int ratsdf_group_size(ratsdf_group* g, int32_t* out) {
  if (!g || !out) return RATSDF_ERR_BAD_ARGUMENT;
  *out = g->S;
  return RATSDF_OK;
}

// Frame f of member s is element [f * S + s] of every array.
int ratsdf_group_integrate_device_batch(ratsdf_group* g, int n, const void* const* d_rgb,
                                        const void* const* d_depth, const void* const* d_ht,
                                        const void* const* d_lt, int height, int width,
                                        float max_depth, const ratsdf_intrinsics* K,
                                        const ratsdf_pose* T) {
  if (!g || n < 0 || (n > 0 && (!d_rgb || !d_depth || !K || !T)) || height <= 0 || width <= 0)
    return RATSDF_ERR_BAD_ARGUMENT;
  if (n == 0) return RATSDF_OK;
  const int S = g->S;
  const size_t npix = (size_t)height * width;
  for (size_t i = 0; i < (size_t)n * S; ++i)
    if (!d_rgb[i] || !d_depth[i] || !finite_frame(K[i], T[i], max_depth)) return RATSDF_ERR_BAD_ARGUMENT;
  DeviceGuard guard(g->device);  // (not ENTRY: every frame's arguments are checked, and an empty batch returns, first)
  if (!guard.ok()) return RATSDF_ERR_DEVICE;
  ratsdf_engine* e0 = g->eng[0];
  if (npix * (size_t)e0->S >= 0xFFFFFFFFull) return RATSDF_ERR_BAD_ARGUMENT;
  for (ratsdf_engine* e : g->eng) {
    if (e->cand_ready) return RATSDF_ERR_BAD_ARGUMENT;  // cannot happen between complete calls
    STCHK(e->ensure_image(npix, npix * (size_t)e->S));
  }
  // ---- tables ----
  const size_t njobs = (size_t)n * S;
  const size_t job_bytes = njobs * sizeof(FrameJob), jobs_off = g->jobs_off();
  if (job_bytes > g->d_jobs.size() || jobs_off + job_bytes > g->tables.size()) {
    HIPCHK(hipStreamSynchronize(g->stream));
    STCHK(g->d_jobs.grow(job_bytes));
    STCHK(g->tables.grow(jobs_off + job_bytes));
  }
  FrameJob* const d_jobs = g->d_jobs.as<FrameJob>();
  EngineDev* const d_engs = g->d_engs.as<EngineDev>();
  void* side = nullptr;
  STCHK(g->tables.acquire(&side));  // (the copies that last used this side are done)
  EngineDev* he = static_cast<EngineDev*>(side);
  for (int s = 0; s < S; ++s) he[s] = g->eng[(size_t)s]->record();
  FrameJob* hj = reinterpret_cast<FrameJob*>(static_cast<uint8_t*>(side) + jobs_off);
  for (int f = 0; f < n; ++f)
    for (int s = 0; s < S; ++s) {
      const size_t i = (size_t)f * S + s;
      const ratsdf_engine* e = g->eng[(size_t)s];
      e->fill_job(hj[i], ratsdf_engine::FrameIn::at(i, d_rgb, d_depth, d_ht, d_lt, K, T), height, width, max_depth,
                  e->parity + (unsigned)f);
    }
  // ---- ordering with the members' own streams (queries, single-engine frames) ----
  for (int s = 0; s < S; ++s) {
    HIPCHK(hipEventRecord(g->ev_member[(size_t)s], g->eng[(size_t)s]->stream));
    HIPCHK(hipStreamWaitEvent(g->stream, g->ev_member[(size_t)s], 0));
  }
  STCHK(g->tables.copy(d_engs, 0, (size_t)S * sizeof(EngineDev), g->stream));
  STCHK(g->tables.commit(d_jobs, jobs_off, job_bytes, g->stream));

  // ---- launches ----
  const bool fused = e0->fused_serial && e0->vpl != 1;
  ratsdf_engine::Geom g1 = e0->geometry(height, width, true, e0->vpl == 1 ? 100 : g->split_a,
                                        (fused || e0->vpl == 1) ? 0 : g->split_b, !fused);
  ratsdf_engine::Geom g0 = e0->geometry(height, width, false, 0, 0, false);
  // Several members at VGA-sized images: a member's slice of 1 536 update workgroups (two blocks each at 640x480 /
  // 5 mm) instead of 4 096 -- a quarter of those are idle and still have to be dispatched, slice after slice
  // (4 members, round 4: 46.3 k frames/s at 4 096, 47.1 k at 3 072, 48.0 k at 2 048, 48.9 k at 1 536 and 1 024;
  // a single stream measures the same from 1 536 to 4 096)
  if (!e0->grid_from_env && S >= 2 && g0.grid == 4096u) g0.grid = g1.grid = 1536u;
  const unsigned grid0 = g0.grid;
  const uint32_t commit_rot = fused ? e0->commit_rotation(grid0, grid0 * (unsigned)S) : 0u;
  // events for every frame that will be timed: created before anything is launched
  if (g->timer.on) STCHK(g->timer.reserve((size_t)n / 4 + 2));
  // A failure from here on leaves launches queued on the group's stream on behalf of members that do
  // not know about them: the members are brought to a consistent state before the error is returned.
  auto abandon = [&](int frames_launched) {
    (void)hipStreamSynchronize(g->stream);
    for (ratsdf_engine* e : g->eng) e->abandon_pipeline(frames_launched, true);
  };
  const Enqueued q = enqueue_jobs(g->stream, (EnginePtr)d_engs, d_jobs, n, S, g0, g1, commit_rot, fused ? 8u : 0u,
                                  (e0->tab.tail_on ? 1u : 0u) | e0->front_prio, e0->vpl, &g->timer);
  if (q.status != RATSDF_OK) {
    abandon(q.frames);
    return q.status;
  }
  if (hipEventRecord(g->ev_done, g->stream) != hipSuccess) {
    abandon(n);
    return RATSDF_ERR_DEVICE;
  }
  int st_all = RATSDF_OK;
  for (ratsdf_engine* e : g->eng) {
    if (hipStreamWaitEvent(e->stream, g->ev_done, 0) != hipSuccess) st_all = RATSDF_ERR_DEVICE;
    e->parity = (e->parity + (unsigned)n) & 1u;
    e->cand_ready = false;
    e->pending = true;
  }
  if (st_all != RATSDF_OK) (void)hipStreamSynchronize(g->stream);  // ordering by waiting instead
  return st_all;
}

int ratsdf_group_synchronize(ratsdf_group* g) {
  ENTRY(g, true);
  HIPCHK(hipStreamSynchronize(g->stream));
  int worst = RATSDF_OK;
  for (ratsdf_engine* e : g->eng) {
    const int st = ratsdf_synchronize(e);
    if (st != RATSDF_OK && worst == RATSDF_OK) worst = st;
  }
  return worst;
}

int ratsdf_group_profile_enable(ratsdf_group* g, int enable) {
  ENTRY(g, true);
  const int st = g->timer.drain(g->stream);
  g->timer.on = enable != 0;
  return st;
}

int ratsdf_group_profile_read(ratsdf_group* g, double* ms, int64_t* launches) {
  ENTRY(g, true);
  return g->timer.read(g->stream, ms, launches);
}

}  // extern "C"
