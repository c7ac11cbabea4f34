/*
 * ratsdf_score.h -- the map scored against labelled points: every near-surface voxel of the HIP engine's map takes the
 * label of its nearest labelled point, and the voxel's probability is counted against that label.  The last step of
 * the reference's evaluation (python_utils/scannet_eval/scanneteval.py: a KD-tree over the ground-truth mesh vertices,
 * TP / FP / FN / TN at prob > p_cutoff, IoU), done on the device instead of on a download of every voxel; the histogram
 * over probability bins gives the counts at any cutoff k / 256 (the PR curve that script's TODO asks for).
 *
 * Kept apart from ratsdf.h because the CPU oracle does not implement these entry points (as ratsdf_esdf.h).
 *
 * 1. A label set: n points with a label each (IGNORE, LOW, HIGH), built once, immutable, kept on the device of the
 *    creating engine.  Points with a non-finite coordinate are dropped ("kept" counts the others): they can never be a
 *    voxel's nearest, and the indices of the rest stay the original ones.  Creation is synchronous (it drains the
 *    engine's stream).  Any engine of the same device may score against the set; with an engine of another device the
 *    scoring calls return RATSDF_ERR_BAD_ARGUMENT.  The set must be destroyed before the process ends its device, and
 *    not while a scoring call that uses it may still be queued (ratsdf_synchronize the engines first).
 *    n == 0 is a valid, empty set.  RATSDF_ERR_BAD_ARGUMENT, with nothing left allocated, for: n > 2^26, a label above
 *    2 (the device form counts them in its build kernel and reads that count), a NaN, negative or infinite cell, NULL
 *    pointers with n > 0, a NULL out.
 *    The points are held in a dense grid of cubic cells over the kept points' bounding box (origin = its lower corner,
 *    cells[a] = floor((max[a] - min[a]) / cell) + 1, in double precision).  cell == 0 asks for 8 * voxel_size of the
 *    creating engine; the edge is doubled until it is at least 1e-6 and the grid has at most 2^24 cells.  info reports
 *    what was used (an empty set: cells = {1, 1, 1}, origin = {0, 0, 0}).  The grid only accelerates the search: no
 *    result below depends on it.
 *
 * 2. Scoring (bit-exact: tests/score_ref.py restates it).
 *    Voxels, order, position: those of ratsdf_gather_valid_semantic -- every voxel of every allocated block, blocks
 *    ascending in hash-entry index, voxels in x + 8y + 64z order; the position is (float)grid_index * voxel_size per
 *    axis (voxel_tsdf.cu:53-55).  per_voxel[i] belongs to record i of that gather taken on the same map.
 *    Selection: a voxel is selected iff fabsf(tsdf) < tsdf_below and weight >= min_weight (a NaN tsdf never is).
 *    Nearest: over the kept points, with p the point and g the voxel position, in fp32 and as written (no contraction)
 *        dx = px - gx, dy = py - gy, dz = pz - gz,  d2 = (dx * dx + dy * dy) + dz * dz
 *    the nearest point minimises (d2, original index) lexicographically among the points with
 *    d2 <= max_dist * max_dist (the fp32 product): ties and duplicates have a defined winner.
 *    Per-voxel record: matched -- the original index and its d2; selected but unmatched -- nearest = -2; not selected
 *    -- nearest = -1; in both latter cases dist2 is the quiet NaN 0x7FC00000.
 *    Score: voxels = 512 * allocated blocks.  A matched voxel whose nearest label is IGNORE counts in unannotated only
 *    (scanneteval.py:49-51).  Otherwise it counts in confusion[] = {TP, FP, FN, TN} (get_confusion_matrix() row-major,
 *    scanneteval.py:127-146: TP = predicted high & labelled HIGH, FP = predicted high & LOW, FN = predicted low &
 *    HIGH, TN = predicted low & LOW) with "predicted high" = prob > p_cutoff (a NaN probability predicts low), and in
 *    hist[label - 1][bin(prob)],  bin(p) = p >= 1 ? 255 : p > 0 ? (int)(p * 256.0f) : 0  (the product is exact; NaN
 *    and -0.0 fall in bin 0).  selected == unmatched + unannotated + sum(confusion); sum(hist) == sum(confusion).
 *    All of it is integers, independent of scheduling.
 *
 * Host form: *per_voxel / *n (per_voxel may be NULL: then n may be too) receive the records in a buffer for
 * ratsdf_free_buffer, NULL / 0 for an empty map.  Synchronous.
 * Device form: d_score (8-byte aligned) receives the ratsdf_label_score; at most the first min(count, capacity)
 * per-voxel records go to d_per_voxel (8-byte aligned; NULL: none, capacity is then ignored but must not be negative;
 * capacity 0 is a pure count) and the count of voxels as an int64 to d_count (8-byte aligned).  Asynchronous on the
 * engine's stream, ordered after everything enqueued on it before.
 *
 * RATSDF_ERR_BAD_ARGUMENT, with nothing launched and nothing written, for: a NULL engine, set, params, out / d_score or
 * d_count; a set of another device; a NaN tsdf_below or p_cutoff; max_dist not finite, <= 0, above 64 * cell of the
 * set, or with a square that is not a finite positive fp32 number; min_weight > 255; non-zero flags or reserved words;
 * a misaligned pointer; a negative capacity.
 * Both calls apply the last frame's deferred pool releases first, only read the map (directory, pool, free list and
 * directory-delta record stay as they are) and return a sticky engine error, never hide it.  Workspace is engine-owned.
 */
#ifndef RATSDF_SCORE_H_
#define RATSDF_SCORE_H_

#include "ratsdf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RATSDF_LABEL_IGNORE 0 /* unannotated: a voxel whose nearest point has it is dropped (scanneteval.py:49-51) */
#define RATSDF_LABEL_LOW 1
#define RATSDF_LABEL_HIGH 2

typedef struct ratsdf_labelset ratsdf_labelset;

typedef struct ratsdf_labelset_info { /* 48 bytes */
  int64_t points;    /* points given */
  int64_t kept;      /* points with three finite coordinates: only these can ever be nearest */
  float cell;        /* cell edge actually used, metres */
  float origin[3];   /* lower corner of the grid */
  int32_t cells[3];
  uint32_t reserved;
} ratsdf_labelset_info;

typedef struct ratsdf_score_params { /* 32 bytes */
  float tsdf_below;     /* voxel selected iff fabsf(tsdf) < tsdf_below (reference: 0.1); NaN refused */
  float max_dist;       /* metres, finite, > 0: a point farther than this is never a voxel's nearest */
  float p_cutoff;       /* predicted high-touch iff prob > p_cutoff (scanneteval.py:58); NaN refused */
  uint32_t min_weight;  /* selected iff weight >= min_weight; 0..255; 0 = the reference (no weight test) */
  uint32_t flags;       /* must be 0 */
  uint32_t reserved[3]; /* must be 0 */
} ratsdf_score_params;

typedef struct ratsdf_label_score { /* 4160 bytes, all int64 */
  int64_t voxels;       /* 512 * allocated blocks */
  int64_t selected;
  int64_t unmatched;    /* selected, no kept point with d2 <= max_dist*max_dist */
  int64_t unannotated;  /* matched, nearest label IGNORE */
  int64_t confusion[4]; /* TP, FP, FN, TN: get_confusion_matrix() row-major, scanneteval.py:127-146 */
  int64_t hist[2][256]; /* [0]: nearest label LOW, [1]: HIGH; by probability bin */
} ratsdf_label_score;

typedef struct ratsdf_voxel_label { /* 8 bytes */
  int32_t nearest;
  float dist2;
} ratsdf_voxel_label;

int ratsdf_labelset_create(ratsdf_engine* e, const float* xyz, const uint8_t* labels, size_t n, float cell,
                           ratsdf_labelset** out);
int ratsdf_labelset_create_device(ratsdf_engine* e, const void* d_xyz, const void* d_labels, size_t n, float cell,
                                  ratsdf_labelset** out);
int ratsdf_labelset_info_get(const ratsdf_labelset* s, ratsdf_labelset_info* out);
int ratsdf_labelset_destroy(ratsdf_labelset* s);

int ratsdf_score_labels(ratsdf_engine* e, const ratsdf_labelset* s, const ratsdf_score_params* p,
                        ratsdf_label_score* out, ratsdf_voxel_label** per_voxel /* may be NULL */, size_t* n);
int ratsdf_score_labels_device(ratsdf_engine* e, const ratsdf_labelset* s, const ratsdf_score_params* p, void* d_score,
                               void* d_per_voxel /* may be NULL */, int64_t capacity, void* d_count);

#ifdef __cplusplus
}
#endif
#endif /* RATSDF_SCORE_H_ */
