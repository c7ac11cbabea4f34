/*
 * ratsdf_sample.h -- batched point sampling of the HIP engine's map: the TSDF, its gradient, the high-touch
 * probability and whether the map has seen a spot, at n world points.
 *
 * Kept apart from ratsdf.h because the CPU oracle does not implement these entry points (as ratsdf_map.h).  No
 * reference counterpart: the reference's one consumer of the map outside rendering (disinfect_slam::query_tsdf,
 * disinfect_slam/disinfect_slam.cc:58) pulls every voxel of a box to the host and works from that.
 *
 * The sampling contract (bit-exact: a test restates it).  All arithmetic is fp32, evaluated as written, with no
 * contraction.  vs is the engine's voxel size; the voxel at integer grid index i sits at i * vs (voxel_tsdf.cu:41).
 * Per axis:
 *   g = p / vs;  l = floorf(g);  f = g - l;  u = 1 - f
 *   corner t_ijk = tsdf of voxel (lx + i, ly + j, lz + k)
 *   c00 = t000*uz + t001*fz   c01 = t010*uz + t011*fz   c10 = t100*uz + t101*fz   c11 = t110*uz + t111*fz
 *   c0  = c00*uy + c01*fy     c1  = c10*uy + c11*fy
 *   tsdf = c0*ux + c1*fx
 *   grad[0] = (c1 - c0) / vs
 *   grad[1] = ((c01 - c00)*ux + (c11 - c10)*fx) / vs
 *   grad[2] = (((t001 - t000)*uy + (t011 - t010)*fy)*ux + ((t101 - t100)*uy + (t111 - t110)*fy)*fx) / vs
 *   nearest = roundf(g)  (half away from zero, as the ray cast's final grid point; always one of the 8 corners)
 * Flags:
 *   ALLOCATED  all 8 corners lie in allocated blocks
 *   OBSERVED   ALLOCATED, and every corner has weight >= 1
 *   NEAREST    the nearest voxel's block is allocated
 * Defaults: with ALLOCATED clear, tsdf and grad are the quiet NaN 0x7FC00000 (outputs compare byte for byte) and
 * min_weight is 0; with NEAREST clear, prob and rgbw are 0 (VoxelSEGM(), VoxelRGBW()).  A non-finite point, or one
 * whose corners leave the int16 voxel range [-32768, 32767], gets flags = 0 and every field at its default -- it never
 * wraps around onto a real block.
 *
 * Deliberately NOT VoxelHashTable::RetrieveTSDF (utils/tsdf/voxel_hash.cu:161-188, restated for the ray cast as
 * retrieve_tsdf in kernels_raycast.h): that pairs the corner at floor + 1 with the weight (floor + 1 - g) and the
 * corner at floor with (g - floor), i.e. mirrored trilinear interpolation: exact only at cell centres (at an integer
 * point it returns the voxel one step up every axis).  The ray cast keeps it for parity with the reference; a point
 * query must not inherit it.
 *
 * Both calls: n == 0 is OK and launches nothing; a NULL pointer with n > 0, n > INT32_MAX or a d_out that is not
 * 16-byte aligned (d_xyz: 4-byte) is RATSDF_ERR_BAD_ARGUMENT.  The last frame's deferred pool releases are applied
 * first, so a sample taken right after a frame sees that frame's map.  The map is only read (directory, pool, free
 * list and directory-delta record stay as they are).  A sticky engine error is returned, never hidden.
 */
#ifndef RATSDF_SAMPLE_H_
#define RATSDF_SAMPLE_H_

#include "ratsdf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RATSDF_SAMPLE_ALLOCATED 1
#define RATSDF_SAMPLE_OBSERVED 2
#define RATSDF_SAMPLE_NEAREST 4

typedef struct ratsdf_sample { /* 32 bytes */
  float tsdf;          /* trilinear TSDF in the map's units (sdf / truncation, clipped to 1); NaN unless ALLOCATED */
  float grad[3];       /* d tsdf / d metre of the same interpolant (world axes); NaN unless ALLOCATED            */
  float prob;          /* probability of the nearest voxel; 0 if its block is absent (VoxelSEGM() = 0)           */
  ratsdf_rgbw rgbw;    /* colour and weight of the nearest voxel; 0 if its block is absent (VoxelRGBW())         */
  uint8_t min_weight;  /* smallest weight of the 8 corners; 0 unless ALLOCATED                                     */
  uint8_t flags;       /* RATSDF_SAMPLE_ALLOCATED 1 | RATSDF_SAMPLE_OBSERVED 2 | RATSDF_SAMPLE_NEAREST 4        */
  uint8_t reserved[6]; /* written as 0                                                                           */
} ratsdf_sample;

/* xyz: n x 3 float32 world points (metres), host memory; out: n records.  Synchronous. */
int ratsdf_sample_points(ratsdf_engine* e, const float* xyz, size_t n, ratsdf_sample* out);
/* Same on device pointers of the engine's device; out must be 16-byte aligned.
 * Asynchronous on the engine's stream, ordered after everything enqueued on it before. */
int ratsdf_sample_points_device(ratsdf_engine* e, const void* d_xyz, size_t n, void* d_out);

#ifdef __cplusplus
}
#endif
#endif /* RATSDF_SAMPLE_H_ */
