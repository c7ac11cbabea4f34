/*
 * ratsdf_surface.h -- the surface inside a box of the HIP engine's map as oriented, labelled points, compacted on the
 * device: where the TSDF changes sign between two neighbouring voxels, which way the surface faces there, and the
 * high-touch probability, colour and weight of the nearer voxel.
 *
 * Kept apart from ratsdf.h because the CPU oracle does not implement these entry points (as ratsdf_esdf.h).  No
 * reference counterpart: the reference's only surface read-out is the marching-cubes mesh of the whole map.
 *
 * The contract (bit-exact: a test restates it).  All arithmetic is fp32, evaluated as written, no contraction, sqrtf
 * and division correctly rounded.  vs: the engine's voxel size; t(w), weight(w), prob(w), rgbw(w): the map's values
 * of voxel w; e_a: the unit step along axis a.
 *   observed(w)  w lies in the int16 voxel range, its block is in the directory with a pool block (an entry still
 *                pending -- a placeholder left by a failed frame -- does not count, as in ratsdf_esdf.h),
 *                weight(w) >= min_weight, and w is not the fresh voxel of ratsdf_fuse.h (weight == 1 and tsdf bits
 *                0xBF800000)
 *   Edge (v, a), a in {0, 1, 2}, runs from voxel v to v + e_a and is owned by v.  It is a CROSSING iff v is in the
 *   box (origin[b] <= v[b] < origin[b] + dims[b]), observed(v), observed(v + e_a) and (t0 < 0) != (t1 < 0), with
 *   t0 = t(v), t1 = t(v + e_a): -0.0f and 0.0f are not negative.  The upper endpoint may lie one voxel outside the
 *   box, so boxes that tile space give every crossing exactly once.
 *   A crossing's point:
 *     f         = t0 / (t0 - t1)
 *     pos[a]    = ((float)v[a] + f) * vs;   pos[b] = (float)v[b] * vs for the two other axes
 *     d_b(w)    for an endpoint w and axis b, by which of w + e_b, w - e_b are observed:
 *                 both: (t(w + e_b) - t(w - e_b)) * 0.5f;  only the upper: t(w + e_b) - t(w);
 *                 only the lower: t(w) - t(w - e_b);       neither: 0.0f
 *     g_b       = d_b(v) * (1.0f - f) + d_b(v + e_a) * f
 *     len       = sqrtf(g_0 * g_0 + g_1 * g_1 + g_2 * g_2)
 *     normal[b] = g_b / len, or all three 0.0f when len is 0 or not finite (the tsdf is positive in free space, so
 *                 the normal points out of the surface)
 *     the chosen endpoint is v + e_a iff f >= 0.5f, else v; prob and rgbw are its values
 *   The point is dropped iff prob < min_prob.
 *   Order: ascending in block z, then block y, then block x (block = voxel index >> 3 of the owner v), then the
 *   owner's index within its block, x + 8 y + 64 z, then the axis a.
 * Limits (those of ratsdf_esdf.h): every dims[a] in [1, 1024]; dims[0] * dims[1] * dims[2] <= 2^27; origin[a] and
 * origin[a] + dims[a] - 1 in the int16 voxel range [-32768, 32767].  Anything else is RATSDF_ERR_BAD_ARGUMENT, and
 * so are a NULL origin, dims or params, min_weight outside [1, 255], a NaN min_prob, non-zero flags or reserved, a
 * NULL out or n (host form), a negative capacity, a NULL d_points with capacity > 0, a d_points that is not 16-byte
 * aligned and a d_count that is NULL or not 8-byte aligned (device form).  Nothing is launched then.
 * Both calls apply the last frame's deferred pool releases first, so points taken right after a frame see that
 * frame's map.  The map is only read (directory, pool, free list and directory-delta record stay as they are).  A
 * sticky engine error is returned, never hidden.  Workspace is engine-owned and grows on demand; a failed
 * allocation is RATSDF_ERR_DEVICE (not sticky: the next call tries again).
 */
#ifndef RATSDF_SURFACE_H_
#define RATSDF_SURFACE_H_

#include "ratsdf.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ratsdf_surface_point { /* 32 bytes */
  float pos[3];     /* metres, world axes */
  float normal[3];  /* unit length, pointing into free space; (0,0,0) when the gradient is zero */
  float prob;       /* probability of the chosen endpoint */
  ratsdf_rgbw rgbw; /* colour and weight of the chosen endpoint */
} ratsdf_surface_point;

typedef struct ratsdf_surface_params {
  int32_t min_weight; /* 1..255 */
  float min_prob;     /* points with prob < min_prob are dropped; 0 keeps all; NaN refused */
  uint32_t flags;     /* must be 0 */
  uint32_t reserved;  /* must be 0 */
} ratsdf_surface_params;

/* origin: voxel index of the box's minimum corner; dims: voxels per axis.  Synchronous, host memory: *out receives
 * *n points in the order above, owned by the caller until ratsdf_free_buffer; an empty result is *out = NULL,
 * *n = 0.  (The points pass through a device buffer of *n records that the engine keeps.) */
int ratsdf_surface_points(ratsdf_engine* e, const int32_t origin[3], const int32_t dims[3],
                          const ratsdf_surface_params* params, ratsdf_surface_point** out, size_t* n);
/* Same on device pointers of the engine's device.  Asynchronous on the engine's stream, ordered after everything
 * enqueued on it before.  Writes the first min(total, capacity) points of the order above to d_points (records
 * capacity and beyond are not touched) and the total as an int64 to d_count.  capacity == 0 with a NULL d_points is
 * a pure count. */
int ratsdf_surface_points_device(ratsdf_engine* e, const int32_t origin[3], const int32_t dims[3],
                                 const ratsdf_surface_params* params, void* d_points, int64_t capacity,
                                 void* d_count);

/*
 * Exposure of surface points to lamps: which points of a list a set of point lamps lights, given the voxels of a box
 * that stand in between, and how strongly (P cos(theta) / 4 pi r^2, summed over the lamps).  What ranks candidate lamp
 * poses of a disinfection run and accounts for the dose along a trajectory.  A box read-out in the family of
 * ratsdf_esdf.h: it reads the box's integer states and nothing else of the map; the line of sight is an integer voxel
 * walk, not a march of the TSDF.  No reference counterpart; the CPU oracle does not implement it.
 *
 * The contract (bit-exact: a test restates it).  All float arithmetic is fp32, evaluated as written, no contraction,
 * sqrtf and division correctly rounded.  vs: the engine's voxel size.
 *   Box, states   the box, its limits and state(v) are exactly those of ratsdf_esdf.h with params->occupied_below.  A
 *                 voxel is BLOCKING iff it is OCCUPIED, or UNKNOWN with RATSDF_EXPOSURE_UNKNOWN_OCCUPIED.  Only the
 *                 voxels of the box exist.
 *   in_box(f, b)  for a float f and an axis b: (float)origin[b] <= f < (float)(origin[b] + dims[b]).  A NaN fails it.
 *   Lamp k        (0 <= k < n_lamps <= 64).  f[b] = lamp.pos[b] / vs + 0.5f, its voxel L[b] = (int)floorf(f[b]).
 *                 ACCEPTED iff in_box(f[b], b) on all three axes and L is not BLOCKING.  A lamp that is not accepted
 *                 lights nothing.
 *   Point i       q[b] = pos[b] / vs + normal[b], f[b] = q[b] + 0.5f, its start voxel s[b] = (int)floorf(f[b]): one
 *                 voxel off the surface into free space.  OUTSIDE iff in_box(f[b], b) fails on an axis: then mask[i]
 *                 is 0, dose[i] is not written and the point counts in points_outside.
 *   Pair (i, k)   d[b] = lamp.pos[b] - pos[b];  r2 = d[0]*d[0] + d[1]*d[1] + d[2]*d[2];
 *                 c = normal[0]*d[0] + normal[1]*d[1] + normal[2]*d[2]  (both sums left to right)
 *                 facing iff c > 0.0f;  in range iff not r2 > max_range * max_range
 *                 e = lamp.power * (c / (r2 * sqrtf(r2))) * 0.07957747f
 *   Walk s -> L   integers only.  n[a] = |L[a] - s[a]|, k[a] = 0, the position starts at s.  While the position is not
 *                 L: among the axes with k[a] < n[a] take the one with the smallest (2 k[a] + 1) / n[a] -- two axes
 *                 compared exactly, (2 k[a] + 1) * n[b] against (2 k[b] + 1) * n[a], at most 2047 * 1023; a tie goes
 *                 to the lowest axis -- step one voxel towards L on it and increment k[a].  The visited voxels are s,
 *                 every position after a step, and L: n[0] + n[1] + n[2] + 1 voxels, 6-connected.  The walk is CLEAR
 *                 iff none of them is BLOCKING.
 *   visible(i, k) the lamp is accepted, the point is not OUTSIDE, and the pair is facing, in range and clear.
 *   mask[i]       bit k is set iff visible(i, k).
 *   dose[i]       acc = (RATSDF_EXPOSURE_ACCUMULATE ? the dose[i] passed in : 0.0f); for k ascending over the visible
 *                 lamps acc = acc + e; acc is written.  (Where that sum meets a NaN, which NaN it delivers is not part
 *                 of the contract.)
 *   Lamp table    accepted: 0 or 1; lit: the points with visible(i, k) and e >= min_irradiance; lit_high: those of
 *                 them with prob >= p_cutoff; reserved: 0.
 *   Summary       lit_pairs: the visible pairs; points_lit: the points with a non-zero mask; points_outside;
 *                 lamps_accepted; reserved: 0.
 * Limits: 0 <= n_points <= 2^24, 0 <= n_lamps <= RATSDF_EXPOSURE_MAX_LAMPS; more lamps are a chain of calls with
 * RATSDF_EXPOSURE_ACCUMULATE.  RATSDF_ERR_BAD_ARGUMENT, with nothing launched and nothing written, for: a box
 * ratsdf_esdf refuses; a NULL origin, dims or params; a NULL dose or summary; NULL points with n_points > 0 or NULL
 * lamps with n_lamps > 0; a count out of range; a NaN occupied_below, min_irradiance or p_cutoff; a max_range that is
 * NaN or negative; unknown flag bits or a non-zero reserved word.  The device form also refuses a d_points, d_lamps or
 * d_lamp_table that is not 16-byte aligned, a d_mask or d_summary that is not 8-byte aligned and a d_dose that is not
 * 4-byte aligned.
 * Both calls apply the last frame's deferred pool releases first.  The map is only read.  A sticky engine error is
 * returned, never hidden.  Workspace is engine-owned and grows on demand; a failed allocation is RATSDF_ERR_DEVICE
 * (not sticky: the next call tries again).
 */
#define RATSDF_EXPOSURE_UNKNOWN_OCCUPIED 1u /* == RATSDF_ESDF_UNKNOWN_OCCUPIED: unobserved voxels block light */
#define RATSDF_EXPOSURE_ACCUMULATE 2u       /* dose is in/out: the sums start from what it holds */
#define RATSDF_EXPOSURE_MAX_LAMPS 64

typedef struct ratsdf_lamp { /* 16 bytes */
  float pos[3]; /* metres, world axes */
  float power;  /* watts (or joules: power x dwell) */
} ratsdf_lamp;

typedef struct ratsdf_exposure_params { /* 32 bytes */
  float occupied_below; /* as ratsdf_esdf.h; NaN refused */
  float max_range;      /* metres, >= 0, +INFINITY allowed; NaN and negatives refused */
  float min_irradiance; /* for the lamp table's counts only; NaN refused */
  float p_cutoff;       /* for lit_high only; NaN refused */
  uint32_t flags;       /* RATSDF_EXPOSURE_*; unknown bits refused */
  uint32_t reserved[3]; /* must be 0 */
} ratsdf_exposure_params;

typedef struct ratsdf_lamp_record { /* 16 bytes */
  int32_t accepted;
  int32_t lit;
  int32_t lit_high;
  int32_t reserved;
} ratsdf_lamp_record;

typedef struct ratsdf_exposure_summary { /* 32 bytes */
  int64_t lit_pairs;
  int32_t points_lit;
  int32_t points_outside;
  int32_t lamps_accepted;
  uint32_t reserved[3]; /* written as 0 */
} ratsdf_exposure_summary;

/* Synchronous, host memory.  points: n_points records; lamps: n_lamps records; dose: n_points floats, in/out (read
 * only with RATSDF_EXPOSURE_ACCUMULATE; the entries of OUTSIDE points keep what they held); mask: n_points words;
 * lamp_table: n_lamps records. */
int ratsdf_exposure(ratsdf_engine* e, const int32_t origin[3], const int32_t dims[3],
                    const ratsdf_exposure_params* params, const ratsdf_surface_point* points, int64_t n_points,
                    const ratsdf_lamp* lamps, int32_t n_lamps, float* dose, uint64_t* mask /* may be NULL */,
                    ratsdf_lamp_record* lamp_table /* may be NULL */, ratsdf_exposure_summary* summary);
/* Same on device pointers of the engine's device.  Asynchronous on the engine's stream, ordered after everything
 * enqueued on it before; it reads nothing back.  d_mask and d_lamp_table may be NULL. */
int ratsdf_exposure_device(ratsdf_engine* e, const int32_t origin[3], const int32_t dims[3],
                           const ratsdf_exposure_params* params, const void* d_points, int64_t n_points,
                           const void* d_lamps, int32_t n_lamps, void* d_dose, void* d_mask, void* d_lamp_table,
                           void* d_summary);

#ifdef __cplusplus
}
#endif
#endif /* RATSDF_SURFACE_H_ */
