// coarsen.inc -- map coarsening (include/ratsdf_coarsen.h): the host side of kernels_coarsen.h.  Included at the end of
// ratsdf_engine.hip, behind resample.inc, whose fuse_source_blocks / fuse_candidate_records it shares: the coarse
// records take the path of the resampled ones (k_resample_mark for the empty candidates, fuse_chunk for the others).
#include "../../include/ratsdf_coarsen.h"

namespace {

static int coarsen_launch(ratsdf_engine* src, hipStream_t stream, int32_t n, const int16_t* d_pos, uint32_t* d_rec,
                          int32_t* d_contrib) {
  hipLaunchKernelGGL(k_coarsen_blocks, dim3((unsigned)n), dim3(512), 0, stream, src->tab, src->pool, d_pos, d_rec,
                     d_contrib);
  HIPCHK(hipGetLastError());
  return RATSDF_OK;
}

// The coarse blocks that can hold a contributing voxel, sorted and distinct, as n x 3 int16: a coarse voxel contributes
// only where its centre, fine voxel 2D, is present, and the centres of coarse block B lie in the fine blocks 2B and
// 2B + 1 -- so the list is (x >> 1, y >> 1, z >> 1) of the live blocks, exactly.
static std::vector<int16_t> coarsen_candidates(const std::vector<ratsdf_block>& blocks, int32_t src_num_block) {
  std::vector<uint64_t> keys;
  keys.reserve(blocks.size());
  for (const ratsdf_block& bl : blocks) {
    if (bl.idx < 0 || bl.idx >= src_num_block) continue;  // (a pending entry names no block)
    const int x = bl.x >> 1, y = bl.y >> 1, z = bl.z >> 1;
    keys.push_back((uint64_t)(z + 4096) << 26 | (uint64_t)(y + 4096) << 13 | (uint64_t)(x + 4096));
  }
  std::sort(keys.begin(), keys.end());
  keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
  std::vector<int16_t> out;
  out.reserve(keys.size() * 3);
  for (uint64_t k : keys) {
    out.push_back((int16_t)((int)(k & 8191u) - 4096));
    out.push_back((int16_t)((int)((k >> 13) & 8191u) - 4096));
    out.push_back((int16_t)((int)((k >> 26) & 8191u) - 4096));
  }
  return out;
}

// bits(dst.voxel_size) == bits(2.0f * src.voxel_size)
static bool coarsen_sizes_ok(const ratsdf_engine* dst, const ratsdf_engine* src) {
  const float twice = 2.0f * src->vs;
  return memcmp(&dst->vs, &twice, 4) == 0 && memcmp(&dst->trunc, &src->trunc, 4) == 0;
}

}  // namespace

extern "C" {

int ratsdf_coarsen_blocks_device(ratsdf_engine* src, int32_t n, const void* d_block_pos, void* d_voxels,
                                 void* d_contrib) {
  ENTRY(src, n >= 0 && (n == 0 || (d_block_pos && d_voxels)) && ((uintptr_t)d_voxels & 15u) == 0 &&
                 ((uintptr_t)d_contrib & 3u) == 0);
  STCHK(src->settle());
  STCHK(sticky_raised(src));
  if (n == 0) return RATSDF_OK;
  return coarsen_launch(src, src->stream, n, (const int16_t*)d_block_pos, (uint32_t*)d_voxels, (int32_t*)d_contrib);
}

int ratsdf_fuse_map_coarsened(ratsdf_engine* dst, ratsdf_engine* src, ratsdf_fuse_stats* stats) {
  ENTRY(dst, src && dst != src && dst->device == src->device && coarsen_sizes_ok(dst, src));
  if (stats) memset(stats, 0, sizeof(*stats));
  std::vector<ratsdf_block> blocks;
  STCHK(fuse_source_blocks(src, &blocks));
  return fuse_candidate_records(
      dst, coarsen_candidates(blocks, src->tab.num_block),
      [&](hipStream_t stream, int32_t m, const int16_t* d_pos, uint32_t* d_rec, int32_t* d_contrib) {
        return coarsen_launch(src, stream, m, d_pos, d_rec, d_contrib);
      },
      stats);
}

}  // extern "C"
