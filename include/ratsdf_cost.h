/*
 * ratsdf_cost.h -- the cost-to-go field of a box of the HIP engine's map: for every traversable voxel the length of the
 * shortest path to a goal voxel that stays in free space with a given clearance, and the neighbour to step to.  What a
 * planner consumes after the ESDF (clearance) and the regions (reachability): without it a caller downloads the ESDF
 * and the states and runs Dijkstra on the host.
 *
 * Kept apart from ratsdf.h because the CPU oracle does not implement these entry points (as ratsdf_esdf.h).  No
 * reference counterpart.
 *
 * The contract (bit-exact: a test restates it).  The box, its limits and the index
 *   i = (x - ox) + X * ((y - oy) + Y * (z - oz))          (X, Y, Z = dims; ox, oy, oz = origin)
 * are those of ratsdf_esdf.h.  Only the voxels of the box exist.
 *   state(v), esdf(v)  exactly ratsdf_esdf's `state` and `out` for this box with params->occupied_below and the
 *                 RATSDF_ESDF_UNKNOWN_OCCUPIED bit of params->flags -- including that header's rule that an obstacle
 *                 just outside the box is not seen.
 *   traversable(v)  v is not in the ESDF's obstacle set O; state(v) is FREE, or UNKNOWN with
 *                 RATSDF_COST_THROUGH_UNKNOWN; and not esdf(v) < params->clearance (fp32 comparison as written: a voxel
 *                 exactly at the clearance is traversable, clearance <= 0 admits every voxel outside O).
 *   Moves         between two traversable voxels, both inside the box, that are 26-neighbours.  Integer weights: 10
 *                 across a face, 14 across an edge, 17 across a corner.  With RATSDF_COST_FACES_ONLY only face moves
 *                 exist.  No corner-cutting rule: the clearance is the safety margin.
 *   Goals         n_goals absolute voxel triples (int32 x, y, z), 0 <= n_goals <= 2^20.  A goal outside the box or not
 *                 traversable is ignored; duplicates count once; no accepted goal at all is a valid input (everything
 *                 is unreachable).
 *   Cost          cost[i], uint32: the least total weight of a path from v to any accepted goal; 0 at an accepted goal;
 *                 RATSDF_COST_NONE for a voxel that is not traversable or reaches no goal.  (At most 2^27 * 17 < 2^32.)
 *                 The unique solution of the shortest-path equations: it does not depend on scheduling.
 *   Next step     next[i], one byte (optional).  Direction code d = (dx + 1) + 3 * (dy + 1) + 9 * (dz + 1).  Among the
 *                 moves from v to neighbours u with a finite cost, the one that minimises cost[u] + w; ties go to the
 *                 smallest code.  RATSDF_COST_AT_GOAL at an accepted goal, RATSDF_COST_NO_STEP at cost NONE.  Computed
 *                 from the delivered cost array in a last pass.
 *   Summary       ratsdf_cost_summary, below.  `rounds` is the one field the map does not define: the relaxation
 *                 rounds this call ran (device form: params->rounds; host form: as many as it took).
 *
 * Host form: cost receives X * Y * Z uint32, next (may be NULL) as many bytes.  Synchronous.  Always runs to
 * convergence: pending == 0 and the result is exact.  params->rounds must be 0; RATSDF_COST_CONTINUE is refused.
 * Device form: asynchronous on the engine's stream, ordered after everything enqueued on it before.  It enqueues exactly
 * params->rounds relaxation rounds, 1 <= rounds <= 4096, and reads nothing back.  If summary.pending != 0 the field is
 * not yet exact, but: every value is >= the exact cost; accepted goals are 0 and voxels that are not traversable are
 * NONE; every finite value of a voxel that is no goal is accounted for by a neighbour, min over moves (cost[u] + w) <=
 * cost[v].  So following `next` strictly lowers the cost and ends at a goal.  With RATSDF_COST_CONTINUE d_cost holds the
 * output of an earlier call with the same map, box, params (but for rounds and this flag) and goals, and the call goes on
 * from it.  A d_cost that does not come from such a call gives an undefined field, never a fault.
 * Alignment: d_cost and d_goals 16 bytes, d_summary 8 bytes.
 *
 * RATSDF_ERR_BAD_ARGUMENT, with nothing launched and nothing written, for: a box ratsdf_esdf refuses; a NULL origin,
 * dims, params, cost / d_cost or summary / d_summary; a NaN occupied_below or clearance; unknown flag bits;
 * RATSDF_COST_UNKNOWN_OCCUPIED together with RATSDF_COST_THROUGH_UNKNOWN; n_goals out of range, or NULL goals with
 * n_goals > 0; rounds out of range for the form; RATSDF_COST_CONTINUE in the host form; a misaligned pointer.
 * Both calls apply the last frame's deferred pool releases first.  The map is only read (directory, pool, free list and
 * directory-delta record stay as they are).  A sticky engine error is returned, never hidden.  Workspace is engine-owned
 * and grows on demand; a failed allocation is RATSDF_ERR_DEVICE (not sticky: the next call tries again).  The host form
 * also returns RATSDF_ERR_DEVICE, with the stream drained and cost / next / summary unwritten, if tiles are still dirty
 * after more rounds than the box has voxels -- which no map can cause: a guard against a loop without end.
 */
#ifndef RATSDF_COST_H_
#define RATSDF_COST_H_

#include "ratsdf_esdf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RATSDF_COST_UNKNOWN_OCCUPIED 1u /* flags: RATSDF_ESDF_UNKNOWN_OCCUPIED, unobserved voxels are obstacles */
#define RATSDF_COST_THROUGH_UNKNOWN 2u  /* flags: UNKNOWN voxels outside O are traversable */
#define RATSDF_COST_FACES_ONLY 4u       /* flags: only the six face moves exist */
#define RATSDF_COST_CONTINUE 8u         /* flags (device form): go on from the field in d_cost */

#define RATSDF_COST_NONE 0xFFFFFFFFu /* cost: not traversable, or no goal reached */
#define RATSDF_COST_AT_GOAL 255      /* next: an accepted goal */
#define RATSDF_COST_NO_STEP 254      /* next: cost NONE */

typedef struct ratsdf_cost_params { /* 16 bytes */
  float occupied_below; /* as in ratsdf_esdf.h; NaN refused */
  float clearance;      /* metres; see traversable(v); NaN refused */
  uint32_t flags;       /* RATSDF_COST_* */
  int32_t rounds;       /* host form: 0; device form: 1..4096 relaxation rounds to enqueue */
} ratsdf_cost_params;

typedef struct ratsdf_cost_summary { /* 32 bytes */
  int32_t goals;        /* voxels with cost 0 */
  int32_t traversable;  /* traversable voxels */
  int32_t reached;      /* voxels with finite cost */
  uint32_t max_cost;    /* largest finite cost; 0 if none */
  int32_t pending;      /* 0 if and only if the field has converged */
  int32_t rounds;       /* rounds run */
  uint32_t reserved[2]; /* written as 0 */
} ratsdf_cost_summary;

int ratsdf_cost_to_go(ratsdf_engine* e, const int32_t origin[3], const int32_t dims[3],
                      const ratsdf_cost_params* params, const int32_t* goals, int32_t n_goals, uint32_t* cost,
                      uint8_t* next /* may be NULL */, ratsdf_cost_summary* summary);
int ratsdf_cost_to_go_device(ratsdf_engine* e, const int32_t origin[3], const int32_t dims[3],
                             const ratsdf_cost_params* params, const void* d_goals, int32_t n_goals, void* d_cost,
                             void* d_next /* may be NULL */, void* d_summary);

#ifdef __cplusplus
}
#endif
#endif /* RATSDF_COST_H_ */
