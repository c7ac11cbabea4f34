// cost.inc -- the cost-to-go field of a box of the map (include/ratsdf_cost.h): the host side of kernels_cost.h.
// Included at the end of ratsdf_engine.hip.

extern "C" {

static_assert(sizeof(ratsdf_cost_params) == 16 && sizeof(ratsdf_cost_summary) == 32 &&
                  offsetof(ratsdf_cost_summary, pending) == 16,
              "ratsdf_cost_params / ratsdf_cost_summary layout");
static_assert(RATSDF_COST_UNKNOWN_OCCUPIED == RATSDF_ESDF_UNKNOWN_OCCUPIED, "the ESDF's bit");
static_assert(RATSDF_COST_NONE == kCostNone && RATSDF_COST_AT_GOAL == kCostAtGoal && RATSDF_COST_NO_STEP == kCostNoStep,
              "the header's codes are the kernels'");

// The workspace is EngineMem::ws_cost (CostWork, workspace.h), per voxel, with an ESDF workspace of its own inside: a
// field of esdf.inc or regions of regions.inc queued before or after share nothing with it.

constexpr int32_t kCostMaxGoals = 1 << 20, kCostMaxRounds = 4096;
constexpr int kCostBatch = 32;  // rounds the host form enqueues between two looks at the dirty count (even: the parity
                                // of a batch's first round is always 0)

// the tiles of a box and the state of a run that the launches below share
struct CostRun {
  MapBox b;
  size_t n;
  int ntx, nty, ntz;
  uint32_t ntiles;
  bool faces_only;
  CostWork w;
};

// argument checks of both entry points (RATSDF_ERR_BAD_ARGUMENT when false)
static bool cost_box(const int32_t* origin, const int32_t* dims, const ratsdf_cost_params* p, const void* goals,
                     int32_t n_goals, CostRun* r) {
  constexpr uint32_t all = RATSDF_COST_UNKNOWN_OCCUPIED | RATSDF_COST_THROUGH_UNKNOWN | RATSDF_COST_FACES_ONLY |
                           RATSDF_COST_CONTINUE;
  if (!p || std::isnan(p->occupied_below) || std::isnan(p->clearance) || (p->flags & ~all) ||
      ((p->flags & RATSDF_COST_UNKNOWN_OCCUPIED) && (p->flags & RATSDF_COST_THROUGH_UNKNOWN)) || n_goals < 0 ||
      n_goals > kCostMaxGoals || (n_goals > 0 && !goals) || !map_box(origin, dims, &r->b, &r->n))
    return false;
  r->ntx = (r->b.X + kRegTX - 1) / kRegTX, r->nty = (r->b.Y + kRegTY - 1) / kRegTY;
  r->ntz = (r->b.Z + kRegTZ - 1) / kRegTZ;
  r->ntiles = (uint32_t)r->ntx * (uint32_t)r->nty * (uint32_t)r->ntz;
  r->faces_only = (p->flags & RATSDF_COST_FACES_ONLY) != 0u;
  return (size_t)r->ntiles <= cost_tiles_max(r->n);  // (always: workspace.h)
}

// the ESDF of the box into the workspace, the seed and the goals: afterwards the field is ready for round 0
static int cost_begin(ratsdf_engine* e, const CostRun& r, const ratsdf_cost_params& p, const int32_t* d_goals,
                      int32_t n_goals, uint32_t* d_cost) {
  const CostWork& w = r.w;
  // (the field lands in the x pass's buffer, dead once the y pass has run: as ratsdf_esdf's host form)
  STCHK(esdf_launch(e, r.b, r.n, p.occupied_below, p.flags & RATSDF_ESDF_UNKNOWN_OCCUPIED, w.esdf, (float*)w.esdf.gx,
                    nullptr));
  const size_t items = std::max<size_t>(r.n, 2 * (size_t)r.ntiles);
  hipLaunchKernelGGL(k_cost_seed, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, e->stream,
                     (const uint8_t*)w.esdf.st, (const float*)w.esdf.gx, p.clearance,
                     p.flags & RATSDF_COST_THROUGH_UNKNOWN, p.flags & RATSDF_COST_CONTINUE, (uint32_t)r.n, r.ntiles,
                     w.trav, d_cost, w.dirty, w.counts);
  HIPCHK(hipGetLastError());
  if (n_goals > 0) {
    const dim3 grid((unsigned)((n_goals + 255) / 256));
    if (r.faces_only)
      hipLaunchKernelGGL(k_cost_goals<true>, grid, dim3(256), 0, e->stream, d_goals, (uint32_t)n_goals, r.b, r.ntx,
                         r.nty, r.ntz, (const uint8_t*)w.trav, d_cost, w.dirty, w.counts);
    else
      hipLaunchKernelGGL(k_cost_goals<false>, grid, dim3(256), 0, e->stream, d_goals, (uint32_t)n_goals, r.b, r.ntx,
                         r.nty, r.ntz, (const uint8_t*)w.trav, d_cost, w.dirty, w.counts);
    HIPCHK(hipGetLastError());
  }
  return RATSDF_OK;
}

// rounds first .. first + count - 1, one launch each; round k reads the flags of parity k & 1
static int cost_rounds(ratsdf_engine* e, const CostRun& r, uint32_t* d_cost, int first, int count) {
  const CostWork& w = r.w;
  for (int k = first; k < first + count; ++k) {
    const int now = k & 1, next = now ^ 1;
    uint32_t *fn = w.dirty + (size_t)now * r.ntiles, *fx = w.dirty + (size_t)next * r.ntiles;
    if (r.faces_only)
      hipLaunchKernelGGL(k_cost_relax<true>, dim3(r.ntiles), dim3(256), 0, e->stream, (const uint8_t*)w.trav, r.b.X,
                         r.b.Y, r.b.Z, r.ntx, r.nty, r.ntz, d_cost, fn, w.counts + now, fx, w.counts + next);
    else
      hipLaunchKernelGGL(k_cost_relax<false>, dim3(r.ntiles), dim3(256), 0, e->stream, (const uint8_t*)w.trav, r.b.X,
                         r.b.Y, r.b.Z, r.ntx, r.nty, r.ntz, d_cost, fn, w.counts + now, fx, w.counts + next);
    HIPCHK(hipGetLastError());
  }
  return RATSDF_OK;
}

// the summary at d_summary (pending: the dirty count the round after `rounds` would start from) and the moves at
// d_next when it is not null
static int cost_finish(ratsdf_engine* e, const CostRun& r, const uint32_t* d_cost, int rounds, uint8_t* d_next,
                       uint32_t* d_summary) {
  const CostWork& w = r.w;
  HIPCHK(hipMemsetAsync(d_summary, 0, sizeof(ratsdf_cost_summary), e->stream));
  hipLaunchKernelGGL(k_cost_summary, dim3((unsigned)((r.n + kCostChunk - 1) / kCostChunk)), dim3(256), 0, e->stream,
                     (const uint8_t*)w.trav, d_cost, (uint32_t)r.n, (const uint32_t*)(w.counts + (rounds & 1)),
                     (uint32_t)rounds, d_summary);
  HIPCHK(hipGetLastError());
  if (!d_next) return RATSDF_OK;
  const unsigned per_voxel = (unsigned)((r.n + 255) / 256);
  if (r.faces_only)
    hipLaunchKernelGGL(k_cost_next<true>, dim3(per_voxel), dim3(256), 0, e->stream, d_cost, r.b.X, r.b.Y, r.b.Z,
                       (uint32_t)r.n, d_next);
  else
    hipLaunchKernelGGL(k_cost_next<false>, dim3(per_voxel), dim3(256), 0, e->stream, d_cost, r.b.X, r.b.Y, r.b.Z,
                       (uint32_t)r.n, d_next);
  HIPCHK(hipGetLastError());
  return RATSDF_OK;
}

int ratsdf_cost_to_go_device(ratsdf_engine* e, const int32_t origin[3], const int32_t dims[3],
                             const ratsdf_cost_params* params, const void* d_goals, int32_t n_goals, void* d_cost,
                             void* d_next, void* d_summary) {
  CostRun r;
  ENTRY(e, d_cost && !((uintptr_t)d_cost & 15u) && !((uintptr_t)d_goals & 15u) && d_summary &&
               !((uintptr_t)d_summary & 7u) && cost_box(origin, dims, params, d_goals, n_goals, &r) &&
               params->rounds >= 1 && params->rounds <= kCostMaxRounds);
  STCHK(box_entry(e));
  STCHK(e->workspace(e->ws_cost, r.n, cost_layout, &r.w));
  STCHK(cost_begin(e, r, *params, (const int32_t*)d_goals, n_goals, (uint32_t*)d_cost));
  STCHK(cost_rounds(e, r, (uint32_t*)d_cost, 0, params->rounds));
  return cost_finish(e, r, (const uint32_t*)d_cost, params->rounds, (uint8_t*)d_next, (uint32_t*)d_summary);
}

int ratsdf_cost_to_go(ratsdf_engine* e, const int32_t origin[3], const int32_t dims[3],
                      const ratsdf_cost_params* params, const int32_t* goals, int32_t n_goals, uint32_t* cost,
                      uint8_t* next, ratsdf_cost_summary* summary) {
  CostRun r;
  ENTRY(e, cost && summary && cost_box(origin, dims, params, goals, n_goals, &r) && params->rounds == 0 &&
               !(params->flags & RATSDF_COST_CONTINUE));
  STCHK(box_entry(e));
  STCHK(e->workspace(e->ws_cost, r.n, cost_layout, &r.w));
  // through the staging pair: the goals | the cost words | the moves
  const size_t goal_bytes = ws_round((size_t)n_goals * 12);
  STCHK(e->staging(goal_bytes + 4 * r.n + (next ? r.n : 0), kHostChunk));
  uint8_t* dev = e->d_out.as<uint8_t>();
  uint32_t* d_cost = (uint32_t*)(dev + goal_bytes);
  uint8_t* d_next = next ? dev + goal_bytes + 4 * r.n : nullptr;
  if (n_goals > 0) {
    memcpy(e->h_out.as<void>(), goals, (size_t)n_goals * 12);  // (12 MB at most: kHostChunk holds it)
    HIPCHK(hipMemcpyAsync(dev, e->h_out.as<void>(), (size_t)n_goals * 12, hipMemcpyHostToDevice, e->stream));
  }
  STCHK(cost_begin(e, r, *params, (const int32_t*)dev, n_goals, d_cost));
  // Batches of rounds until no tile is dirty.  Every round that starts with a dirty tile either lowers a word or
  // leaves fewer dirty tiles, and a shortest path crosses fewer tile borders than the box has voxels: the bound below
  // is never reached by a field of this engine.  (Nothing is queued at that exit: read_small has drained the stream.)
  int rounds = 0;
  uint32_t counts[2] = {1u, 0u};
  while (counts[0] != 0u) {
    if ((size_t)rounds > r.n + 1024) return RATSDF_ERR_DEVICE;
    STCHK(cost_rounds(e, r, d_cost, rounds, kCostBatch));
    rounds += kCostBatch;
    STCHK(e->read_small(counts, r.w.counts, 8));
  }
  STCHK(cost_finish(e, r, d_cost, rounds, d_next, r.w.summary));
  STCHK(e->read_small(summary, r.w.summary, sizeof(ratsdf_cost_summary)));
  STCHK(e->download(cost, d_cost, 4 * r.n));
  if (next) STCHK(e->download(next, d_next, r.n));
  return e->sticky();
}

}  // extern "C"
