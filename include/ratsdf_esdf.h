/*
 * ratsdf_esdf.h -- a Euclidean signed distance field (ESDF) over a box of the HIP engine's map: clearance in metres
 * to the nearest obstacle voxel, well beyond the truncation band where the TSDF stops carrying distance.
 *
 * Kept apart from ratsdf.h because the CPU oracle does not implement these entry points (as ratsdf_map.h and
 * ratsdf_sample.h).  No reference counterpart: the reference hands a planner the TSDF of a box
 * (disinfect_slam::query_tsdf), which reads 1 (or nothing) one truncation away from any surface.
 *
 * The ESDF contract (bit-exact: a test restates it).  The box is the voxels (x, y, z) with origin[a] <= v[a] <
 * origin[a] + dims[a]; only they exist for the transform.
 *   State of voxel v (written to `state` when it is not NULL):
 *     UNKNOWN   v's block is not in the directory, or its entry is still pending (a placeholder left by a failed
 *               frame: no pool block), or v's weight (rgbw >> 24) is 0
 *     OCCUPIED  otherwise, if tsdf(v) <= occupied_below (the map's TSDF units: sdf / truncation; 0 means "at or
 *               behind the surface")
 *     FREE      everything else
 *   Obstacle set O: the OCCUPIED voxels of the box; with RATSDF_ESDF_UNKNOWN_OCCUPIED also the UNKNOWN ones.
 *   Distance (d2: an integer squared distance between voxel indices; vs: the engine's voxel size):
 *     v not in O:  d2 = min over o in O of |v - o|^2;        out = sqrtf((float)d2) * vs      (+INFINITY if O is empty)
 *     v in O:      d2 = min over u in box \ O of |v - u|^2;  out = -(sqrtf((float)d2) * vs)   (-INFINITY if box \ O
 *                                                                                              is empty)
 *   fp32, sqrtf correctly rounded.  Since only voxels inside the box count, a caller that needs distances up to r
 *   metres must pad the box by ceil(r / vs) voxels on every side: within that band of the box's faces |out| may
 *   exceed the whole map's distance (an obstacle just outside the box is not seen), never fall short of it.
 * Limits: every dims[a] in [1, 1024]; dims[0] * dims[1] * dims[2] <= 2^27 (512 MB of output); origin[a] and
 * origin[a] + dims[a] - 1 in the int16 voxel range [-32768, 32767].  Anything else is RATSDF_ERR_BAD_ARGUMENT, and
 * so are a NaN occupied_below, unknown flag bits, a NULL out / d_out and a d_out that is not 16-byte aligned.  (The
 * 1024 cap keeps d2 <= 3 * 1023^2 < 2^24, so (float)d2 is exact.)
 * Both calls apply the last frame's deferred pool releases first, so a field taken right after a frame sees that
 * frame's map.  The map is only read (directory, pool, free list and directory-delta record stay as they are).  A
 * sticky engine error is returned, never hidden.  Workspace is engine-owned and grows on demand; a failed
 * allocation is RATSDF_ERR_DEVICE (not sticky: the next call tries again).
 */
#ifndef RATSDF_ESDF_H_
#define RATSDF_ESDF_H_

#include "ratsdf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RATSDF_ESDF_UNKNOWN_OCCUPIED 1u /* flags: unobserved voxels count as obstacles (conservative planning) */
#define RATSDF_ESDF_STATE_UNKNOWN 0
#define RATSDF_ESDF_STATE_FREE 1
#define RATSDF_ESDF_STATE_OCCUPIED 2

/* origin: voxel index of the box's minimum corner; dims: voxels per axis.  out: dims[0]*dims[1]*dims[2] floats,
 * index (x-ox) + dims[0]*((y-oy) + dims[1]*(z-oz)); state (may be NULL): one byte per voxel, same order.
 * Synchronous, host memory. */
int ratsdf_esdf(ratsdf_engine* e, const int32_t origin[3], const int32_t dims[3], float occupied_below,
                uint32_t flags, float* out, uint8_t* state);
/* Same on device pointers of the engine's device (d_out 16-byte aligned; d_state may be NULL).  Asynchronous on the
 * engine's stream, ordered after everything enqueued on it before. */
int ratsdf_esdf_device(ratsdf_engine* e, const int32_t origin[3], const int32_t dims[3], float occupied_below,
                       uint32_t flags, void* d_out, void* d_state);

#ifdef __cplusplus
}
#endif
#endif /* RATSDF_ESDF_H_ */
