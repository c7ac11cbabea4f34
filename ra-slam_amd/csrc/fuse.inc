// fuse.inc -- map fusion (include/ratsdf_fuse.h): the host side of kernels_fuse.h.  Included at the end of
// ratsdf_engine.hip, behind mapfile.inc (ratsdf_fuse_map_file reads a checkpoint with its validator).
//
// Every form ends in fuse_chunk: at most kFuseChunk listed blocks, "allocate what is missing, fuse what has a place"
// up to 8 times (import_from_device explains the repetition), with a done-bit per listed block so that no block is
// fused twice.  The chunk bounds the allocation pass's work lists: every request of a pass fits the chained-bucket
// resolver's sort (kSlowSortCap) whatever the directory looks like, so a large source cannot raise RATSDF_ERR_CAPACITY
// through list sizes.
#include <unordered_set>

#include "../../include/ratsdf_fuse.h"

static_assert(sizeof(ratsdf_fuse_stats) == 40 && offsetof(ratsdf_fuse_stats, voxels_averaged) == 32,
              "ratsdf_fuse_stats layout");

namespace {

constexpr uint32_t kFuseChunk = kSlowSortCap;  // blocks per allocation pass
constexpr int kFusePasses = 8;
// allocation passes made since the library was loaded (all engines): ratsdf_debug_fuse_passes, for tests that must
// show that a call needed more than one pass per chunk
std::atomic<long long> acc_passes{0};

// Views of the engine's fusion scratch (EngineMem::d_fuse): positions | source pool indices | done bits | counters.
struct FuseScratch {
  int16_t* pos;
  int32_t* idx;
  uint32_t* done;  // kFuseChunk / 32 words, the counters right behind them (cleared with one memset)
  FuseCounters* cnt;
  static constexpr size_t kPosBytes = (size_t)kFuseChunk * 6, kIdxBytes = (size_t)kFuseChunk * 4,
                          kDoneBytes = kFuseChunk / 8;
  static constexpr size_t kBytes = kPosBytes + kIdxBytes + kDoneBytes + sizeof(FuseCounters);
};
static_assert(FuseScratch::kPosBytes % 16 == 0 && sizeof(FuseCounters) == 24, "fusion scratch layout");

static int fuse_scratch(ratsdf_engine* e, FuseScratch* s) {
  if (e->d_fuse.size() < FuseScratch::kBytes) {
    HIPCHK(hipStreamSynchronize(e->stream));
    e->d_fuse.reset();
    STCHK(e->d_fuse.alloc(FuseScratch::kBytes));
  }
  uint8_t* p = e->d_fuse.as<uint8_t>();
  s->pos = (int16_t*)p;
  s->idx = (int32_t*)(p + FuseScratch::kPosBytes);
  s->done = (uint32_t*)(p + FuseScratch::kPosBytes + FuseScratch::kIdxBytes);
  s->cnt = (FuseCounters*)(p + FuseScratch::kPosBytes + FuseScratch::kIdxBytes + FuseScratch::kDoneBytes);
  return RATSDF_OK;
}
static int fuse_clear(ratsdf_engine* e, const FuseScratch& s) {  // done bits and counters of a new chunk
  HIPCHK(hipMemsetAsync(s.done, 0, FuseScratch::kDoneBytes + sizeof(FuseCounters), e->stream));
  return RATSDF_OK;
}

// What a call starts with: the engine settled, no sticky error, the rank buffers sized for a chunk, the map marked as
// carrying probabilities, the scratch, and the free-list level (blocks_allocated is its drop).
static int fuse_begin(ratsdf_engine* e, FuseScratch* s, int32_t* free_before) {
  STCHK(e->settle());
  STCHK(e->sticky());
  STCHK(e->ensure_image(0, (size_t)kFuseChunk));
  STCHK(fuse_scratch(e, s));
  e->ever_sem = true;  // (the blocks come with their probabilities: FrameParams::segm_live)
  return e->read_small(free_before, &e->ctl->num_free, 4);
}
static int fuse_end(ratsdf_engine* e, int status, int32_t free_before, ratsdf_fuse_stats* acc, ratsdf_fuse_stats* out) {
  int32_t free_after = free_before;
  const int rs = e->read_small(&free_after, &e->ctl->num_free, 4);  // (waits for the stream)
  acc->blocks_allocated = (int64_t)free_before - free_after;
  if (out) *out = *acc;
  const int st = e->sticky();
  if (st != RATSDF_OK) return st;
  return status != RATSDF_OK ? status : rs;
}

// One chunk: n <= kFuseChunk blocks at d_pos (device), their voxels as k_fuse_blocks describes; the chunk's done bits
// and counters have been cleared (fuse_clear) or prepared (k_fuse_unpack).  Returns with the stream drained.
static int fuse_chunk(ratsdf_engine* e, const FuseScratch& s, int32_t n, const int16_t* d_pos, const int32_t* d_idx,
                      const uint32_t* tsdf, const uint32_t* rgbw, const uint32_t* prob, uint32_t stride,
                      ratsdf_fuse_stats* acc) {
  const FrameParams P = e->base_params();  // (with the engine's shard filter)
  FuseCounters hc;
  memset(&hc, 0, sizeof(hc));
  hc.missing = (uint32_t)n;
  const unsigned grid = (unsigned)std::min<uint32_t>(((uint32_t)n + 3u) / 4u, 2048u);
  int st = RATSDF_OK;
  for (int pass = 0; pass < kFusePasses && hc.missing != 0 && st == RATSDF_OK; ++pass) {
    const uint32_t par = e->parity;  // an allocation pass of its own in the next frame's counters
    hipLaunchKernelGGL(k_fuse_alloc, dim3((n + 255) / 256), dim3(256), 0, e->stream, e->tab, P, d_pos, n, s.done, e->req,
                       e->req_cap, e->slow, kSlowCap, e->ctl, par);
    st = e->commit_pass(kFuseChunk, par);
    if (st != RATSDF_OK) break;
    if (hipMemsetAsync(&s.cnt->missing, 0, 4, e->stream) != hipSuccess) {
      st = RATSDF_ERR_DEVICE;
      break;
    }
    hipLaunchKernelGGL(k_fuse_blocks, dim3(grid), dim3(256), 0, e->stream, e->tab, e->pool, P, d_pos, n, d_idx, tsdf, rgbw,
                       prob, stride, s.done, s.cnt);
    if (hipGetLastError() != hipSuccess) {
      st = RATSDF_ERR_DEVICE;
      break;
    }
    st = e->read_small(&hc, s.cnt, sizeof(hc));  // (control data: 24 bytes per pass; waits for the stream)
    ++acc_passes;
    if (*(volatile uint32_t*)e->h_err != 0u) break;  // pool exhausted, a list full: more passes change nothing
  }
  // every way out: the stream drained, and what the chunk's passes did so far in the statistics (the voxel counters
  // only grow, so a read that failed above is made up for here)
  if (st != RATSDF_OK) {
    (void)hipStreamSynchronize(e->stream);
    FuseCounters late;
    if (e->read_small(&late, s.cnt, sizeof(late)) == RATSDF_OK) hc = late;
  }
  acc->blocks_skipped += hc.skipped;
  acc->voxels_copied += (int64_t)(hc.voxels & 0xFFFFFFFFull);
  acc->voxels_averaged += (int64_t)(hc.voxels >> 32);
  if (st != RATSDF_OK) return st;
  if (*(volatile uint32_t*)e->h_err != 0u) return e->sticky();
  return hc.missing != 0 ? RATSDF_ERR_CAPACITY : RATSDF_OK;
}

// n records of 1536 words in device memory, chunk by chunk
static int fuse_records(ratsdf_engine* e, const FuseScratch& s, int32_t n, const int16_t* d_pos, const uint32_t* rec,
                        ratsdf_fuse_stats* acc) {
  for (int32_t first = 0; first < n; first += (int32_t)kFuseChunk) {
    const int32_t m = std::min<int32_t>((int32_t)kFuseChunk, n - first);
    const uint32_t* r = rec + (size_t)first * 1536u;
    STCHK(fuse_clear(e, s));
    acc->blocks_seen += m;
    STCHK(fuse_chunk(e, s, m, d_pos + (size_t)first * 3, nullptr, r, r + 512, r + 1024, 1536u, acc));
  }
  return RATSDF_OK;
}

// distinct positions: a block listed twice would be fused twice, by two waves at once
static bool fuse_positions_distinct(const int16_t* bp, size_t n) {
  std::unordered_set<uint64_t> seen;
  seen.reserve(n * 2);
  for (size_t i = 0; i < n; ++i) {
    const uint64_t k = (uint64_t)(uint16_t)bp[3 * i] | (uint64_t)(uint16_t)bp[3 * i + 1] << 16 |
                       (uint64_t)(uint16_t)bp[3 * i + 2] << 32;
    if (!seen.insert(k).second) return false;
  }
  return true;
}

}  // namespace

extern "C" {

// test hook: allocation passes made by fusion calls since the library was loaded
long long ratsdf_debug_fuse_passes(void) { return acc_passes.load(); }

int ratsdf_fuse_map(ratsdf_engine* dst, ratsdf_engine* src, ratsdf_fuse_stats* stats) {
  ENTRY(dst, src && dst != src && dst->device == src->device && memcmp(&dst->vs, &src->vs, 4) == 0 &&
                 memcmp(&dst->trunc, &src->trunc, 4) == 0);
  ratsdf_fuse_stats acc;
  memset(&acc, 0, sizeof(acc));
  if (stats) *stats = acc;
  // the source: settled, sound, its live entries listed in its own selection buffer (as ratsdf_dump_directory)
  STCHK(src->settle());
  STCHK(src->sticky());
  STCHK(src->select(kSelValid, GridBounds{}, &src->ctl->n_sel));
  uint32_t n_sel = 0;
  STCHK(src->read_small(&n_sel, &src->ctl->n_sel, 4));  // (the source's stream is idle from here on)
  if (n_sel > src->vis_cap) return RATSDF_ERR_CAPACITY;
  if (n_sel == 0) {  // an empty source: nothing to launch
    STCHK(dst->settle());
    return dst->sticky();
  }
  FuseScratch s;
  int32_t free_before = 0;
  STCHK(fuse_begin(dst, &s, &free_before));
  int st = RATSDF_OK;
  for (uint32_t first = 0; first < n_sel && st == RATSDF_OK; first += kFuseChunk) {
    const uint32_t m = std::min(kFuseChunk, n_sel - first);
    st = fuse_clear(dst, s);
    if (st != RATSDF_OK) break;
    hipLaunchKernelGGL(k_fuse_unpack, dim3((m + 255) / 256), dim3(256), 0, dst->stream, src->vis + first, m,
                       src->tab.num_block, s.pos, s.idx, s.done, s.cnt);
    st = fuse_chunk(dst, s, (int32_t)m, s.pos, s.idx, (const uint32_t*)src->pool.tsdf, src->pool.rgbw,
                    (const uint32_t*)src->pool.segm, 512u, &acc);
    uint32_t listed = 0;  // (the counters of the chunk are still there: fuse_chunk returns with the stream drained)
    if (dst->read_small(&listed, &s.cnt->listed, 4) == RATSDF_OK) acc.blocks_seen += listed;
  }
  return fuse_end(dst, st, free_before, &acc, stats);
}

int ratsdf_fuse_blocks_device(ratsdf_engine* e, int32_t n, const void* d_block_pos, const void* d_voxels,
                              ratsdf_fuse_stats* stats) {
  ENTRY(e, n >= 0 && (n == 0 || (d_block_pos && d_voxels)) && ((uintptr_t)d_voxels & 15u) == 0);
  ratsdf_fuse_stats acc;
  memset(&acc, 0, sizeof(acc));
  if (stats) *stats = acc;
  if (n == 0) {
    STCHK(e->settle());
    return e->sticky();
  }
  FuseScratch s;
  int32_t free_before = 0;
  STCHK(fuse_begin(e, &s, &free_before));
  const int st = fuse_records(e, s, n, (const int16_t*)d_block_pos, (const uint32_t*)d_voxels, &acc);
  return fuse_end(e, st, free_before, &acc, stats);
}

int ratsdf_fuse_blocks(ratsdf_engine* e, int32_t n, const int16_t* bp, const float* tsdf, const ratsdf_rgbw* rgbw,
                       const float* prob, ratsdf_fuse_stats* stats) {
  ENTRY(e, n >= 0 && (n == 0 || (bp && tsdf && rgbw && prob)) && fuse_positions_distinct(bp, (size_t)n));
  ratsdf_fuse_stats acc;
  memset(&acc, 0, sizeof(acc));
  if (stats) *stats = acc;
  if (n == 0) {
    STCHK(e->settle());
    return e->sticky();
  }
  FuseScratch s;
  int32_t free_before = 0;
  STCHK(fuse_begin(e, &s, &free_before));
  // the three host arrays go up in chunks of kMapChunk blocks: {tsdf | rgbw | prob} of the chunk side by side
  DevMem stage;
  StreamDrain drain{e->stream};
  STCHK(stage.alloc((size_t)kMapChunk * kMapRecordBytes));
  uint8_t* d = stage.as<uint8_t>();
  int st = RATSDF_OK;
  for (int32_t first = 0; first < n && st == RATSDF_OK; first += (int32_t)kMapChunk) {
    const int32_t m = std::min<int32_t>((int32_t)kMapChunk, n - first);
    const size_t per = (size_t)m * 2048, off = (size_t)first * 512;
    if (hipMemcpyAsync(s.pos, bp + (size_t)first * 3, (size_t)m * 6, hipMemcpyHostToDevice, e->stream) != hipSuccess ||
        hipMemcpyAsync(d, tsdf + off, per, hipMemcpyHostToDevice, e->stream) != hipSuccess ||
        hipMemcpyAsync(d + per, rgbw + off, per, hipMemcpyHostToDevice, e->stream) != hipSuccess ||
        hipMemcpyAsync(d + 2 * per, prob + off, per, hipMemcpyHostToDevice, e->stream) != hipSuccess) {
      st = RATSDF_ERR_DEVICE;
      break;
    }
    st = fuse_clear(e, s);
    if (st != RATSDF_OK) break;
    acc.blocks_seen += m;
    st = fuse_chunk(e, s, m, s.pos, nullptr, (const uint32_t*)d, (const uint32_t*)(d + per),
                    (const uint32_t*)(d + 2 * per), 512u, &acc);
  }
  return fuse_end(e, st, free_before, &acc, stats);
}

int ratsdf_fuse_map_file(ratsdf_engine* e, const char* path, ratsdf_fuse_stats* stats) {
  // host work first: a file that is refused has not touched the device
  if (!path) return RATSDF_ERR_BAD_ARGUMENT;
  MapContents m;
  FILE* f = nullptr;
  STCHK(map_read_validate(path, nullptr, &m, &f));
  FileCloser fc{f};
  if (!e || memcmp(&m.h.voxel_size, &e->vs, 4) != 0 || memcmp(&m.h.truncation, &e->trunc, 4) != 0)
    return RATSDF_ERR_BAD_ARGUMENT;
  if (fseek(f, (long)m.voxel_offset, SEEK_SET) != 0) return RATSDF_ERR_BAD_ARGUMENT;
  std::vector<int16_t> pos;  // of the live entries, in entry order = voxel record order
  pos.reserve((size_t)m.h.n_blocks * 3);
  for (const MapEntry& me : m.entries)
    if (me.e.idx >= 0) pos.insert(pos.end(), {me.e.x, me.e.y, me.e.z});
  const int32_t n = (int32_t)m.h.n_blocks;
  // (the checkpoint reader checks entry and pool indices, not that a position sits in one live entry only)
  if (!fuse_positions_distinct(pos.data(), (size_t)n)) return RATSDF_ERR_BAD_ARGUMENT;
  DeviceGuard guard(e->device);  // (not ENTRY: the file is read and checked first, see above)
  if (!guard.ok()) return RATSDF_ERR_DEVICE;
  ratsdf_fuse_stats acc;
  memset(&acc, 0, sizeof(acc));
  if (stats) *stats = acc;
  if (n == 0) {
    STCHK(e->settle());
    return e->sticky();
  }
  FuseScratch s;
  int32_t free_before = 0;
  STCHK(fuse_begin(e, &s, &free_before));
  // one page-locked chunk and its device copy: read, upload, fuse (fuse_chunk returns with the stream drained, so the
  // pair is free again when the next chunk is read)
  HostMem host;
  DevMem dev;
  StreamDrain drain{e->stream};
  STCHK(host.alloc((size_t)kMapChunk * kMapRecordBytes));
  STCHK(dev.alloc((size_t)kMapChunk * kMapRecordBytes));
  int st = RATSDF_OK;
  for (int32_t first = 0; first < n && st == RATSDF_OK; first += (int32_t)kMapChunk) {
    const int32_t c = std::min<int32_t>((int32_t)kMapChunk, n - first);
    if (!read_all(f, host.as<void>(), (size_t)c * kMapRecordBytes)) {
      st = RATSDF_ERR_BAD_ARGUMENT;  // (the file changed under us: it was whole when it was validated)
      break;
    }
    if (hipMemcpyAsync(s.pos, pos.data() + (size_t)first * 3, (size_t)c * 6, hipMemcpyHostToDevice, e->stream) != hipSuccess ||
        hipMemcpyAsync(dev.as<void>(), host.as<void>(), (size_t)c * kMapRecordBytes, hipMemcpyHostToDevice,
                       e->stream) != hipSuccess) {
      st = RATSDF_ERR_DEVICE;
      break;
    }
    st = fuse_records(e, s, c, s.pos, dev.as<uint32_t>(), &acc);
  }
  return fuse_end(e, st, free_before, &acc, stats);
}

}  // extern "C"
