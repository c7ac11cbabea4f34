/*
 * ratsdf_resample.h -- transformed map fusion: a source map resampled onto the destination's voxel lattice under a
 * rigid pose, on the device, and fused there (ratsdf_fuse.h).  For maps that do not share a lattice: two robots' maps in
 * their own odometry frames, a submap whose anchor moved after loop closure, a checkpoint registered again.
 *
 * Kept apart from ratsdf.h because the CPU oracle does not implement these entry points (as ratsdf_fuse.h).  No
 * reference counterpart.
 *
 * dst_T_src maps source-map coordinates to destination-map coordinates, in metres: p_dst = R(q) p_src + t.  It is NOT
 * a camera pose.  Every component must be finite and | |q|^2 - 1 | <= 1e-3, else RATSDF_ERR_BAD_ARGUMENT.
 *
 * The resampling contract (bit-exact: a test restates it).  All arithmetic is fp32, evaluated as written, with no
 * contraction; quat_rotate / se3_apply / se3_inverse are those of the frame update (SE3, lie_group.cuh:25-40).  vs is
 * the engines' voxel size.  On the host, once per call:
 *   Ti = se3_inverse(dst_T_src)
 *   G  = { Ti.q, (Ti.t.x / vs, Ti.t.y / vs, Ti.t.z / vs) }             -- the transform in voxel units
 * (voxel units keep the destination index exact as a float: (i * vs) / vs != i for one index in six at 5 mm).
 * Per destination voxel with integer grid index d = 8 * block + local:
 *   g = se3_apply(G, ((float)dx, (float)dy, (float)dz))
 *   per axis: l = floorf(g);  f = g - l;  u = 1 - f
 *   range:    any l outside [-32768, 32766], or g not finite: the voxel does not contribute (it never wraps around
 *             onto a real block -- the rule of ratsdf_sample.h)
 *   corner (i, j, k) = source voxel (lx + i, ly + j, lz + k); it is NEEDED iff all three of its weight factors are
 *             non-zero (the factor of an axis is u for index 0, f for index 1).  A corner that is not needed is not
 *             looked at and reads as 0.0f below.  So a lattice-preserving transform (f == 0 on every axis) needs one
 *             voxel, and a surface block next to unallocated space is not eaten away by it.
 *   the voxel CONTRIBUTES iff every needed corner lies in an allocated source block and passes contributes() of the
 *             fusion contract (weight != 0 and not the fresh voxel {weight 1, tsdf bits 0xBF800000})
 *   c00 = t000*uz + t001*fz   c01 = t010*uz + t011*fz   c10 = t100*uz + t101*fz   c11 = t110*uz + t111*fz
 *   c0  = c00*uy + c01*fy     c1  = c10*uy + c11*fy
 *   tsdf   = c0*ux + c1*fx                                             -- as ratsdf_sample.h
 *   weight = the smallest weight among the needed corners
 *   r, g, b, prob = those of the nearest voxel roundf(g) (half away from zero; always a needed corner)
 *   record of a contributing voxel:      { tsdf, r | g << 8 | b << 16 | weight << 24, prob }
 *   record of a non-contributing voxel:  three zero words (weight 0: fusion leaves the destination voxel alone)
 *
 * Why trilinear tsdf but nearest colour / probability / smallest weight: the tsdf is a smooth field and the surface
 * must not move by up to half a voxel; colours and probabilities of neighbours are not a field to interpolate across an
 * edge, and the smallest weight never claims more confidence than the weakest voxel the sample leans on.
 *
 * The identity pose reproduces plain fusion bit for bit only where Ti.t / vs and the lattice arithmetic are exact
 * (f == 0 everywhere): always for a zero translation, and for a translation by whole voxels when vs is a power of two
 * (or the quotient happens to be exact).  Callers with an identity pose should call ratsdf_fuse_map: it reads the
 * source once and needs no staging.
 */
#ifndef RATSDF_RESAMPLE_H_
#define RATSDF_RESAMPLE_H_

#include "ratsdf_fuse.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Blocks of the DESTINATION lattice, filled from `src` seen through dst_T_src.  d_block_pos: n x 3 int16; d_voxels: n
 * records of 1536 32-bit words {tsdf[512] | rgbw[512] | prob[512]}, voxel order x + 8y + 64z, 16-byte aligned -- the
 * layout ratsdf_export_blocks_device writes and ratsdf_fuse_blocks_device reads; d_contrib: int32 per block, the number
 * of contributing voxels, may be NULL.  All device pointers of src's device.  src is only read (directory, pool, free
 * list and directory-delta record stay as they are); its deferred pool releases are applied first, as for sampling.
 * Asynchronous on src's stream.  n == 0 is RATSDF_OK and launches nothing; n < 0, a NULL pose or pointer with n > 0, a
 * misaligned d_voxels or a refused pose is RATSDF_ERR_BAD_ARGUMENT.  A sticky engine error is returned, never hidden. */
int ratsdf_resample_blocks_device(ratsdf_engine* src, const ratsdf_pose* dst_T_src, int32_t n,
                                  const void* d_block_pos, void* d_voxels, void* d_contrib);

/* The whole map of `src`, resampled and fused into `dst`.  dst == src, a NULL handle or pose, engines on two devices,
 * unequal bits of voxel size or truncation, or a refused pose: RATSDF_ERR_BAD_ARGUMENT, nothing launched, both maps
 * unchanged.  An empty source is RATSDF_OK and changes nothing.
 *
 * The candidate blocks of the destination come from the positions of the source's live entries (control data, read as
 * ratsdf_dump_directory reads them; no voxel crosses to the host): per source block the 8 corners of its reach
 * [8b - 1, 8b + 8] per axis go through the forward transform in voxel units, in double; every destination block inside
 * [-4096, 4095] that holds an integer voxel of their padded axis-aligned box is listed, once.  The list is conservative.
 * Candidates are resampled in chunks of 2048 blocks (12 MiB of staging records); a candidate without a contributing
 * voxel is dropped and NOT allocated; the others go through the record path of ratsdf_fuse_blocks_device, so all that
 * ratsdf_fuse.h promises holds: the voxel update, up to 8 allocation passes per chunk, the shard filter and
 * blocks_skipped, the directory-delta record, captured graphs and groups staying valid, the sticky-error rules, and
 * "what was fused stays fused".  blocks_seen is the number of non-empty candidate blocks offered.  src is only read.
 * Returns when the fusion is done. */
int ratsdf_fuse_map_transformed(ratsdf_engine* dst, ratsdf_engine* src, const ratsdf_pose* dst_T_src,
                                ratsdf_fuse_stats* stats);

#ifdef __cplusplus
}
#endif
#endif /* RATSDF_RESAMPLE_H_ */
