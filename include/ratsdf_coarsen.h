/*
 * ratsdf_coarsen.h -- map coarsening: a source map restricted onto the lattice of TWICE its voxel size, on the device,
 * and fused into an engine of that voxel size (ratsdf_fuse.h).  For consumers that want a coarser map than the one the
 * frames were integrated on: a planner's clearance field of a whole room (ratsdf_esdf.h takes boxes of at most 1024
 * voxels per axis), a checkpoint or an exchange of 1/8 of the bytes, two maps of different resolutions brought together.
 * The coarse map is an engine like any other: sampling, ESDF, surface points, meshes, fusion and checkpoints work on it.
 *
 * Kept apart from ratsdf.h because the CPU oracle does not implement these entry points (as ratsdf_resample.h).  No
 * reference counterpart.
 *
 * There is one factor, two.  Larger factors are chains through engines of the intermediate sizes; each level holds an
 * eighth of the previous level's voxels, so a chain costs little -- the standard pyramid.
 *
 * The coarsening contract (bit-exact: a test restates it).  Voxel i sits at i * vs, so the coarse voxel with integer grid
 * index D = 8 * block + local coincides with the fine voxel c = 2 * D.  The filter is full weighting -- the restriction
 * operator adjoint to the trilinear interpolation of ratsdf_sample.h and ratsdf_resample.h -- normalised over the taps
 * that exist, so a surface block next to unknown space is not eaten away.
 *   taps:     the 27 fine voxels c + o, o in {-1, 0, 1}^3
 *   present:  a tap is PRESENT iff every coordinate of c + o lies in the int16 voxel range [-32768, 32767] (a coordinate
 *             outside it is never wrapped onto a real block -- the rule of ratsdf_sample.h), its block is in the source's
 *             directory with a pool block (a pending placeholder entry does not count, as in ratsdf_esdf.h), and it
 *             passes contributes() of ratsdf_fuse.h (weight != 0 and not the fresh voxel {weight 1, tsdf bits 0xBF800000})
 *   the coarse voxel CONTRIBUTES iff its centre tap o = 0 is present: geometry is never invented where the centre was
 *             not observed.  (So D outside [-16384, 16383] on any axis never contributes.)
 *   k(o) = (2 - |ox|) * (2 - |oy|) * (2 - |oz|)                          -- one of 1, 2, 4, 8
 *   present tap:  c_o = (float)k(o) * (float)weight(c + o),  t_o = tsdf(c + o)
 *   absent tap:   c_o = 0.0f,  t_o = 0.0f                                -- changes neither sum
 *   all arithmetic is fp32, evaluated as written, with no contraction:
 *       num = 0.0f;  den = 0.0f
 *       for oz in -1, 0, 1:  for oy in -1, 0, 1:  for ox in -1, 0, 1:    -- ox fastest
 *           num = num + c_o * t_o
 *           den = den + c_o
 *       tsdf = num / den
 *   (every c_o and every partial den is an integer no larger than 64 * 255, so den is exact)
 *   r, g, b, weight, prob = those of the centre voxel, word for word
 *   record of a contributing voxel:      { tsdf, the centre's rgbw word, the centre's prob }
 *   record of a non-contributing voxel:  three zero words (weight 0: fusion leaves the destination voxel alone)
 *
 * Why the centre's colour, weight and probability: as in ratsdf_resample.h, colours and probabilities of neighbours are
 * not a field to average across an edge, and the coarse voxel claims no more confidence than the voxel it sits on.
 *
 * What coarsening is NOT:
 *   - it is not equal to integrating the frames at the coarse voxel size;
 *   - with taps missing on one side, the value leans towards the side that was observed;
 *   - the tsdf is stored in units of the truncation, and the truncation carries over unchanged: a caller should keep it
 *     at several COARSE voxels, or the band becomes too thin to mesh.  The engine does not police that.
 */
#ifndef RATSDF_COARSEN_H_
#define RATSDF_COARSEN_H_

#include "ratsdf_fuse.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Blocks of the COARSE lattice (voxel size 2 * src's), filled from `src`.  d_block_pos: n x 3 int16 (any int16 value; a
 * block whose voxels lie outside the fine grid comes out empty); d_voxels: n records of 1536 32-bit words
 * {tsdf[512] | rgbw[512] | prob[512]}, voxel order x + 8y + 64z, 16-byte aligned -- the layout
 * ratsdf_export_blocks_device writes and ratsdf_fuse_blocks_device reads; d_contrib: int32 per block, the number of
 * contributing voxels, may be NULL.  All device pointers of src's device.  src is only read (directory, pool, free list
 * and directory-delta record stay as they are); its deferred pool releases are applied first, as for sampling.
 * Asynchronous on src's stream.  n == 0 is RATSDF_OK and launches nothing; n < 0, a NULL pointer with n > 0 or a
 * misaligned d_voxels is RATSDF_ERR_BAD_ARGUMENT.  A sticky engine error is returned, never hidden. */
int ratsdf_coarsen_blocks_device(ratsdf_engine* src, int32_t n, const void* d_block_pos, void* d_voxels,
                                 void* d_contrib);

/* The whole map of `src`, coarsened by two and fused into `dst`.  Requires dst != src, both handles, one device,
 * bits(dst.voxel_size) == bits(2.0f * src.voxel_size) and bit-equal truncation (the tsdf is stored in units of the
 * truncation, so the values carry over unchanged).  Anything else: RATSDF_ERR_BAD_ARGUMENT, nothing launched, both maps
 * unchanged.  An empty source is RATSDF_OK and changes nothing.
 *
 * The candidate blocks come from the positions of the source's live entries (control data, read as
 * ratsdf_dump_directory reads them; no voxel crosses to the host): coarse block (x >> 1, y >> 1, z >> 1), arithmetic
 * shift, of every live source block, sorted and distinct.  The list is exact, not conservative: a coarse block's centres
 * lie only in the fine blocks 2B and 2B + 1.  Candidates are coarsened in chunks of 2048 blocks (12 MiB of staging
 * records); a candidate without a contributing voxel is dropped and NOT allocated; the others go through the record path
 * of ratsdf_fuse_blocks_device, so all that ratsdf_fuse.h promises holds: the voxel update, up to 8 allocation passes per
 * chunk, the shard filter and blocks_skipped, the directory-delta record, captured graphs and groups staying valid, the
 * sticky-error rules, and "what was fused stays fused".  blocks_seen is the number of non-empty candidate blocks offered.
 * src is only read.  Returns when the fusion is done. */
int ratsdf_fuse_map_coarsened(ratsdf_engine* dst, ratsdf_engine* src, ratsdf_fuse_stats* stats);

#ifdef __cplusplus
}
#endif
#endif /* RATSDF_COARSEN_H_ */
