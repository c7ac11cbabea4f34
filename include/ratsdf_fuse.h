/*
 * ratsdf_fuse.h -- map fusion: the blocks of a source map merged into an engine's map with the reference's own
 * weighted-average voxel update, on the device.  From another engine, from block records (host or device) and from a
 * checkpoint file (ratsdf_map.h).
 *
 * Kept apart from ratsdf.h because the CPU oracle does not implement these entry points (as ratsdf_sample.h).  No
 * reference counterpart: the reference has one map per process and no call that takes voxels in.
 *
 * The fusion contract (a test restates it).  Source and destination must have bit-equal voxel_size and truncation (the
 * tsdf is stored in units of the truncation); table sizes and shard settings may differ.  A block of the source that
 * the destination lacks is allocated in the destination by the ordinary allocation pass (fresh voxels: weight 1,
 * tsdf -1, prob 0.5, colour as found in the pool block, voxel_mem.cu:43-51); then every voxel of the block is fused.
 * a = destination voxel, b = source voxel, all arithmetic fp32, evaluated as written, no contraction (as
 * tsdf_integrate_kernel, voxel_tsdf.cu:224-248, with wo = wa, wn = wb):
 *
 *   contributes(v) = v.weight != 0  and not (v.weight == 1 and bits(v.tsdf) == 0xBF800000)      -- not a fresh voxel
 *   if not contributes(b):   a stays as it is, all three words (colour included)
 *   elif not contributes(a): a = b, all three words copied
 *   else:
 *     wa, wb = (float)a.weight, (float)b.weight;  wc = wa + wb
 *     a.tsdf  = (a.tsdf*wa + b.tsdf*wb) / wc
 *     a.r/g/b = (uint8) roundf(((float)a.r*wa + (float)b.r*wb) / wc)                            -- per channel
 *     a.weight = (uint8) fminf(wc, 40)
 *     a.prob  = 1 / (1 + expf(-(wa*L(a.prob) + wb*L(b.prob)) / wc)),   L(p) = logf(p / (1 - p))
 *
 * tsdf, colour and weight are exact.  The probability is the log-odds form the frame update uses (weighted geometric
 * pooling of p and 1 - p, voxel_tsdf.cu:242-248) on the hardware's log / exp / reciprocal: within 1e-4 of the line
 * above evaluated in fp32, NaN exactly where that is NaN (p = 0 on one side and p = 1 on the other).  That holds for
 * every float a map can carry, a probability below FLT_MIN included: the hardware's log2 reads a subnormal input as
 * zero, so the odds of such a voxel are scaled into the normal range before their logarithm is taken.
 *
 * What fusion is NOT: it is not equal to integrating all frames of both maps into one map.  Each map carries the fresh
 * voxel's prior (weight 1, tsdf -1) in its averages, weights are rounded to bytes and capped at 40 in each map before
 * they meet, and a block that space carving removed from one map comes back from the other.
 *
 * All forms: honour the destination's shard filter (a block another shard owns is counted in blocks_skipped, not an
 * error: one whole map fused into each of N shard engines gives the N shards of the fused map); mark the map as
 * carrying probabilities; go through the allocation path of ratsdf_import_blocks, so the directory-delta record stays
 * right and captured batch graphs and groups stay valid; return a sticky engine error, never hide it; report pool
 * exhaustion (RATSDF_ERR_POOL_EXHAUSTED) and a full work list (RATSDF_ERR_CAPACITY) as allocation does.  An insertion
 * can lose its bucket to another one of the same pass, so a call makes up to 8 allocation passes per chunk of blocks; a
 * block is fused exactly once, in the first pass that finds it.  Blocks that still have no place after 8 passes:
 * RATSDF_ERR_CAPACITY -- as after every error but RATSDF_ERR_BAD_ARGUMENT, the blocks already fused STAY fused (there
 * is no un-fusing), and *stats says how far the call got.  This RATSDF_ERR_CAPACITY is the call's own status, not a
 * sticky engine error: ratsdf_synchronize reports nothing afterwards, the engine stays usable, and the blocks that
 * found no place (the listed positions the directory still lacks) may be offered again.  n == 0 is RATSDF_OK and
 * launches nothing; an empty source is RATSDF_OK and leaves the destination as it is (only the source's directory is
 * looked at).
 * Every call returns when the fusion is done (it synchronises the engine's stream).
 */
#ifndef RATSDF_FUSE_H_
#define RATSDF_FUSE_H_

#include "ratsdf.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ratsdf_fuse_stats { /* 40 bytes; out, may be NULL */
  int64_t blocks_seen;      /* blocks of the source offered to the destination                               */
  int64_t blocks_allocated; /* ... that the destination lacked and allocated                                 */
  int64_t blocks_skipped;   /* ... that the destination's shard filter refused                               */
  int64_t voxels_copied;    /* voxels taken over as they are (the destination's did not contribute)          */
  int64_t voxels_averaged;  /* voxels averaged (both contributed)                                            */
} ratsdf_fuse_stats;

/* The map of `src` into the map of `dst`.  Both engines on one device; dst == src, a NULL handle, two devices or an
 * unequal voxel size / truncation: RATSDF_ERR_BAD_ARGUMENT.  Both engines are settled (pending pool releases applied);
 * the source's live directory entries are walked on the device and its pool is read in place: no intermediate
 * records, no host copy of voxel data.  The source is only read. */
int ratsdf_fuse_map(ratsdf_engine* dst, ratsdf_engine* src, ratsdf_fuse_stats* stats);

/* n blocks as ratsdf_import_blocks takes them: block_pos n x 3 int16, tsdf / rgbw / prob n x 512 each (x + 8y + 64z).
 * The positions must be distinct (checked: RATSDF_ERR_BAD_ARGUMENT, the map unchanged). */
int ratsdf_fuse_blocks(ratsdf_engine* dst, int32_t n, const int16_t* block_pos, const float* tsdf,
                       const ratsdf_rgbw* rgbw, const float* prob, ratsdf_fuse_stats* stats);
/* The same on device pointers of the engine's device: d_block_pos n x 3 int16, d_voxels n records of 1536 32-bit words
 * {tsdf[512] | rgbw[512] | prob[512]}, 16-byte aligned -- the layout of ratsdf_export_blocks_device.  The positions
 * must be distinct; this form does NOT check it (the voxels of a block listed twice are undefined: two waves fuse into
 * it at once). */
int ratsdf_fuse_blocks_device(ratsdf_engine* dst, int32_t n, const void* d_block_pos, const void* d_voxels,
                              ratsdf_fuse_stats* stats);

/* A checkpoint written by ratsdf_save_map, fused into the map.  The file is validated on the host exactly as
 * ratsdf_load_map validates it (header, sections, entries, free list, checksum), except that of the configuration only
 * voxel size and truncation must equal the engine's, and that the live entries' positions must be distinct (a load does
 * not need that; a fusion does); on refusal (RATSDF_ERR_BAD_ARGUMENT) nothing has been launched
 * and the map is unchanged.  The blocks go through the record path in chunks of 2048 (12 MiB of staging). */
int ratsdf_fuse_map_file(ratsdf_engine* dst, const char* path, ratsdf_fuse_stats* stats);

/* Test hook: allocation passes made by fusion calls since the library was loaded (all engines). */
long long ratsdf_debug_fuse_passes(void);

#ifdef __cplusplus
}
#endif
#endif /* RATSDF_FUSE_H_ */
