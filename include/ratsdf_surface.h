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

#ifdef __cplusplus
}
#endif
#endif /* RATSDF_SURFACE_H_ */
