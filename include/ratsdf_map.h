/*
 * ratsdf_map.h -- map checkpoints of the HIP engine: save an engine's map to a file and resume it exactly.
 *
 * Kept apart from ratsdf.h because the CPU oracle does not implement these entry points (the reference has no
 * TSDF load path at all).  A map saved after frame A and loaded into an engine of the same
 * configuration continues bit-exactly: the same directory entries, the same free list in its LIFO order, the
 * same voxels -- frames A+1 .. produce what an engine that was never interrupted produces.
 *
 * File format, version 1 (all fields little-endian; DESIGN.md 3 "Map files"):
 *   header   64 bytes:
 *              char     magic[8] = "RATSDFMP"
 *              uint32   version = 1, header_size = 64
 *              float32  voxel_size, truncation
 *              int32    block_bits, bucket_bits, shard_rank, shard_count, shard_slab_bits
 *              int32    segm_live   (1: the map has seen probabilities -- a frame with ht / lt, or imported blocks)
 *              int32    num_free, free_low   (free count; its lowest value ever: pool indices below it never used)
 *              uint32   n_entries, n_blocks
 *   entries  n_entries x {uint32 entry index, int16 x, y, z, offset, int32 idx}, ascending entry index: every
 *            entry with idx >= 0 (a block) and every entry with idx = -1 and offset != 0 (a dead chain node)
 *   heap     num_free x int32: heap[0 : num_free], the free list bottom to top (AquireBlock pops the top);
 *            heap[i] = i for i < free_low
 *   voxels   n_blocks x 1536 uint32: {tsdf[512] | rgbw[512] | prob[512]}, voxel order x + 8y + 64z, the blocks of
 *            the entries with idx >= 0 in entry order
 *   colour   (num_free - free_low) x 512 uint32: rgbw[512] of the free blocks heap[free_low : num_free], in heap
 *            order -- blocks that have been in use: AquireBlock leaves a block's colour as found (voxel_mem.cu:43-51),
 *            so it is part of the map's future.  The never-used blocks below free_low hold colour 0
 *   trailer  uint64 checksum of every byte before it: FNV-1a over 64-bit words -- the bytes read as consecutive
 *            little-endian uint64 (the last one zero-padded to 8 bytes); h = 0xcbf29ce484222325, then for each
 *            word w: h = (h ^ w) * 0x100000001b3 (mod 2^64)
 *
 * The directory rule.  The kernels that read a loaded directory check nothing, so a file is refused unless its
 * entries are a hash table that lookups can walk.  An entry that is not stored reads as {offset 0, idx -1}; an entry
 * is live if idx >= 0; mask = 2^(bucket_bits+1) - 1; hash(p) = (x * 73856093 ^ y * 19349669 ^ z * 83492791) mod
 * 2^bucket_bits in uint32 arithmetic; an offset is sign-extended, added to the entry index modulo 2^32 and masked.
 * lookup(p): e0 = 2 * hash(p); e0 if it is live with position p; else e0 + 1 if it is; else last = e0 + 1 and, while
 * offset(last) != 0, last = (last + offset(last)) & mask, which is the answer if it is live with position p; else
 * p is absent.
 *   D1  walks end: following the offsets from any stored entry reaches an entry with offset 0 within n_entries steps
 *       (no cycle, whether live or dead nodes form it, through the table's end or by an offset that is a multiple of
 *       the table's size)
 *   D2  a block is where lookups find it: lookup(position(e)) == e for every live entry e (no block in a wrong
 *       bucket, none behind a cut link, no position held twice)
 *   D3  no block behind a dead node: every entry whose offset lookup(position(e)) follows on its way to a live
 *       entry e is live.  An allocation fills an empty home entry with offset 0 (voxel_hash.cu:67-78), which would
 *       cut the chain at a dead node and lose the blocks behind it; Delete unlinks a node (voxel_hash.cu:135-187),
 *       so no engine writes such a file
 *   H   the header names a configuration ratsdf_create_ex accepts: voxel_size and truncation finite and > 0;
 *       shard_count >= 1; with shard_count > 1, 0 <= shard_rank < shard_count; 1 <= shard_slab_bits <=
 *       RATSDF_MAX_SHARD_SLAB_BITS (31: an engine never holds less, ratsdf_create_ex reads <= 0 as 2)
 * A dead chain node with no block behind it is accepted (D1 holds for it as for any stored entry).  Which shard owns
 * a position is not checked: blocks of other shards come in through ratsdf_import_blocks too.  Voxel words are not
 * checked either: a frame onto a loaded map updates them as the reference's expressions evaluate in IEEE fp32, NaN and
 * +-inf included, the weight capped at 40 by the first update (ratsdf_import_blocks in ratsdf.h).
 *
 * Every call returns a ratsdf_status: an I/O failure, or a malformed, corrupted or mismatched file, is
 * RATSDF_ERR_BAD_ARGUMENT.
 */
#ifndef RATSDF_MAP_H_
#define RATSDF_MAP_H_

#include "ratsdf.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Waits for the engine's work (the last frame's deferred pool releases included) and writes the map to
 * path + ".tmp", renamed to `path` once complete: a failed save leaves an earlier file at `path` as it was.
 * Refuses with the sticky status if one is set (ratsdf_recover first), and with RATSDF_ERR_DEVICE if the directory
 * names a pool block twice (such a map cannot be resumed; nothing is written).  The map is not changed. */
int ratsdf_save_map(ratsdf_engine* e, const char* path);
/* Validates the whole file on the host first, the directory rule above included; its voxel size, truncation, table
 * bits and shard fields must equal the engine's.  Then replaces the engine's map with the file's (no engine buffer
 * is reallocated: captured batch graphs and groups stay valid), clears a sticky error and tells a consumer of
 * directory deltas to take a whole directory next.  On refusal the map is unchanged. */
int ratsdf_load_map(ratsdf_engine* e, const char* path);
/* Host only -- no device, no engine: validates the whole file, fills cfg's voxel_size, truncation, block_bits,
 * bucket_bits and shard_* (the other fields are zeroed) and *n_blocks (live blocks).  Either pointer may be NULL. */
int ratsdf_map_file_info(const char* path, ratsdf_config* cfg, int64_t* n_blocks);

#ifdef __cplusplus
}
#endif
#endif /* RATSDF_MAP_H_ */
