// mapfile.inc -- map checkpoints (include/ratsdf_map.h): the file format, its host-side validation, and the save /
// load paths of the engine.  Included at the end of ratsdf_engine.hip (it needs the engine record).
//
// What a checkpoint holds is exactly the state that is NOT derived from the directory: the stored entries (live
// blocks and dead chain nodes), the free list in its real LIFO order with num_free and free_low, the semantics flag,
// the voxels of the live blocks, and the colour of the free blocks that have been in use -- AquireBlock re-initialises
// weight, tsdf and probability of a block it hands out but leaves the colour as found (voxel_mem.cu:43-51), so a
// recycled block carries its old colour into its next life.  Everything else -- occupancy bits, Table::active, claims, counters -- is rebuilt
// by rebuild_derived, the helper ratsdf_recover runs, with the heap kept as loaded.  No reference counterpart (the
// reference cannot load a map back, SURVEY 5).
#include <sys/stat.h>

#include <string>
#include <unordered_map>

#include "../../include/ratsdf_map.h"

namespace {

constexpr uint32_t kMapVersion = 1;
constexpr uint32_t kMapRecordWords = 3 * 512;                 // {tsdf[512] | rgbw[512] | prob[512]}
constexpr size_t kMapRecordBytes = (size_t)kMapRecordWords * 4;
constexpr size_t kMapRgbBytes = 512 * 4;                      // rgbw[512] of a free block that has been in use
constexpr uint32_t kMapChunk = 2048;                          // records per staging buffer (12 MiB)
// k_map_pack / k_map_unpack take two records per workgroup in grids of at most 2048: a chunk never makes one stride
static_assert((kMapChunk + 1) / 2 <= 2048u, "the pack and unpack grids cover a chunk in one sweep");

struct MapHeader {  // 64 bytes, little-endian (the engine's hosts are)
  char magic[8];
  uint32_t version, header_size;
  float voxel_size, truncation;
  int32_t block_bits, bucket_bits, shard_rank, shard_count, shard_slab_bits;
  int32_t segm_live, num_free, free_low;
  uint32_t n_entries, n_blocks;
};
static_assert(sizeof(MapHeader) == 64, "map file header is 64 bytes");
struct MapEntry {  // 16 bytes: entry index + the 12-byte directory entry
  uint32_t entry;
  Entry e;
};
static_assert(sizeof(MapEntry) == 16, "map file entry record is 16 bytes");
constexpr char kMapMagic[8] = {'R', 'A', 'T', 'S', 'D', 'F', 'M', 'P'};

// FNV-1a over the byte stream read as little-endian 64-bit words, the last one zero-padded (ratsdf_map.h)
class MapHash {
 public:
  void update(const void* data, size_t n) {
    const uint8_t* p = static_cast<const uint8_t*>(data);
    while (n && fill_) {  // complete a word begun by an earlier call
      part_[fill_++] = *p++;
      --n;
      if (fill_ == 8) word(part_), fill_ = 0;
    }
    uint64_t h = h_;
    for (; n >= 8; p += 8, n -= 8) {
      uint64_t w;
      memcpy(&w, p, 8);
      h = (h ^ w) * 0x100000001b3ull;
    }
    h_ = h;
    for (; n; --n) part_[fill_++] = *p++;
  }
  uint64_t final() {
    if (fill_) {
      memset(part_ + fill_, 0, 8 - fill_);
      word(part_);
      fill_ = 0;
    }
    return h_;
  }

 private:
  void word(const uint8_t* b) {
    uint64_t w;
    memcpy(&w, b, 8);
    h_ = (h_ ^ w) * 0x100000001b3ull;
  }
  uint64_t h_ = 0xcbf29ce484222325ull;
  uint8_t part_[8] = {};
  int fill_ = 0;
};

// voxels of pool blocks idx[0 .. n) -> records out[0 .. n): 128 lanes per record, 16 bytes of each array per lane.
// kFull: {tsdf | rgbw | prob} (a live block); otherwise rgbw only (a free block's colour)
template <bool kFull>
__global__ __launch_bounds__(256) void k_map_pack(Pool pool, const int32_t* idx, uint32_t n, uint4* out) {
  const uint32_t l = threadIdx.x & 127u;
  for (uint32_t r = blockIdx.x * 2u + (threadIdx.x >> 7); r < n; r += gridDim.x * 2u) {
    const size_t src = (size_t)idx[r] * 128u + l;
    if (kFull) {
      uint4* o = out + (size_t)r * 384u;
      o[l] = reinterpret_cast<const uint4*>(pool.tsdf)[src];
      o[128u + l] = reinterpret_cast<const uint4*>(pool.rgbw)[src];
      o[256u + l] = reinterpret_cast<const uint4*>(pool.segm)[src];
    } else {
      out[(size_t)r * 128u + l] = reinterpret_cast<const uint4*>(pool.rgbw)[src];
    }
  }
}
// ... and back (the indices were checked against num_block on the host)
template <bool kFull>
__global__ __launch_bounds__(256) void k_map_unpack(Pool pool, const int32_t* idx, uint32_t n, const uint4* in) {
  const uint32_t l = threadIdx.x & 127u;
  for (uint32_t r = blockIdx.x * 2u + (threadIdx.x >> 7); r < n; r += gridDim.x * 2u) {
    const size_t dst = (size_t)idx[r] * 128u + l;
    if (kFull) {
      const uint4* s = in + (size_t)r * 384u;
      reinterpret_cast<uint4*>(pool.tsdf)[dst] = s[l];
      reinterpret_cast<uint4*>(pool.rgbw)[dst] = s[128u + l];
      reinterpret_cast<uint4*>(pool.segm)[dst] = s[256u + l];
    } else {
      reinterpret_cast<uint4*>(pool.rgbw)[dst] = in[(size_t)r * 128u + l];
    }
  }
}

// The voxel sections as chunks of at most kMapChunk records: the live blocks' full records, then the colour of the
// free blocks that have been in use (heap[free_low : num_free]); `first` indexes the staging index list, which holds
// the live blocks' pool indices followed by those free ones.
struct MapChunk {
  uint32_t first, n;
  bool full;
  size_t bytes() const { return (size_t)n * (full ? kMapRecordBytes : kMapRgbBytes); }
};
static std::vector<MapChunk> map_chunks(uint32_t n_blocks, uint32_t n_rgb) {
  std::vector<MapChunk> c;
  for (uint32_t r = 0; r < n_blocks; r += kMapChunk) c.push_back(MapChunk{r, std::min(kMapChunk, n_blocks - r), true});
  for (uint32_t r = 0; r < n_rgb; r += kMapChunk) c.push_back(MapChunk{n_blocks + r, std::min(kMapChunk, n_rgb - r), false});
  return c;
}
// stored entries into the freshly initialised table (entry indices checked against num_entry on the host)
__global__ __launch_bounds__(256) void k_map_scatter_entries(Table tab, const uint4* rec, uint32_t n) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint4 r = rec[i];
  uint32_t* pe = reinterpret_cast<uint32_t*>(tab.entries + r.x);
  pe[0] = r.y;
  pe[1] = r.z;
  pe[2] = r.w;
}

struct FileCloser {
  FILE* f;
  ~FileCloser() {
    if (f) fclose(f);
  }
};

// Page-locked double buffers and device staging for the voxel records of a save or a load.
struct MapStaging {
  HostMem host_mem[2];
  DevMem dev_mem[2], idx_mem;
  uint8_t* host[2] = {nullptr, nullptr};  // (views of the above)
  uint8_t* dev[2] = {nullptr, nullptr};
  int32_t* d_idx = nullptr;
  HipEvent ev[2];  // (declared behind the memory: they go first)
  ~MapStaging() {  // (the copies the events stand for have finished before the members free their memory)
    for (HipEvent& x : ev)
      if (x) (void)hipEventSynchronize(x);
  }
  int init(const std::vector<int32_t>& idx, hipStream_t s) {
    const size_t bytes = (size_t)kMapChunk * kMapRecordBytes;
    for (int i = 0; i < 2; ++i) {
      STCHK(host_mem[i].alloc(bytes));
      STCHK(dev_mem[i].alloc(bytes));
      STCHK(ev[i].create(hipEventDisableTiming));
      host[i] = host_mem[i].as<uint8_t>();
      dev[i] = dev_mem[i].as<uint8_t>();
    }
    STCHK(idx_mem.alloc(std::max<size_t>(idx.size(), 1) * 4));
    d_idx = idx_mem.as<int32_t>();
    if (!idx.empty()) HIPCHK(hipMemcpyAsync(d_idx, idx.data(), idx.size() * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    return RATSDF_OK;
  }
};

// What a map file holds apart from its voxels, read and checked.
struct MapContents {
  MapHeader h;
  std::vector<MapEntry> entries;
  std::vector<int32_t> heap;
  std::vector<int32_t> pool_idx;  // of the live entries, in entry order (= voxel record order), then heap[free_low ..)
  size_t voxel_offset = 0;
};

static bool read_all(FILE* f, void* dst, size_t n) { return n == 0 || fread(dst, 1, n, f) == n; }

// Rule H of ratsdf_map.h: the header's configuration is one an engine can have (ratsdf_create_ex)
static bool map_header_ok(const MapHeader& h) {
  if (!std::isfinite(h.voxel_size) || !(h.voxel_size > 0) || !std::isfinite(h.truncation) || !(h.truncation > 0))
    return false;
  if (h.shard_count < 1 || (h.shard_count > 1 && (h.shard_rank < 0 || h.shard_rank >= h.shard_count))) return false;
  return h.shard_slab_bits >= 1 && h.shard_slab_bits <= RATSDF_MAX_SHARD_SLAB_BITS;
}

// Rules D1, D2 and D3 of ratsdf_map.h: the stored entries (ascending, in range -- checked by the caller) are a hash
// table the kernels' lookups can walk.  An entry that is not stored reads as {offset 0, idx -1}.  The device code
// checks nothing of this: find_block, alloc_request, block_present_pre and resolve_block follow offsets until one
// is 0.
static bool map_directory_ok(const std::vector<MapEntry>& ent, int bucket_bits) {
  const uint32_t n = (uint32_t)ent.size();
  const uint32_t entry_mask = (2u << bucket_bits) - 1u, bucket_mask = (1u << bucket_bits) - 1u;
  std::unordered_map<uint32_t, uint32_t> record_of;  // entry index -> its record
  record_of.reserve(n);
  for (uint32_t i = 0; i < n; ++i) record_of.emplace(ent[i].entry, i);
  auto next = [&](uint32_t i) -> uint32_t {  // the record that record i's offset leads to; n: an entry not stored
    const auto it = record_of.find((ent[i].entry + (uint32_t)(int32_t)ent[i].e.offset) & entry_mask);
    return it == record_of.end() ? n : it->second;
  };
  // D1: the walk from every stored entry reaches offset 0.  Each record is stepped over once: a walk stops at a
  // record an earlier walk has shown to end, and one that meets a record of its own path has found a cycle.
  enum : uint8_t { kNotWalked = 0, kOnPath = 1, kEnds = 2 };
  std::vector<uint8_t> state(n, kNotWalked);
  std::vector<uint32_t> path;
  for (uint32_t i = 0; i < n; ++i) {
    path.clear();
    uint32_t j = i;
    while (j != n && state[j] == kNotWalked) {
      state[j] = kOnPath;
      path.push_back(j);
      j = ent[j].e.offset ? next(j) : n;
    }
    if (j != n && state[j] == kOnPath) return false;
    for (uint32_t k : path) state[k] = kEnds;
  }
  // D2 and D3: lookup(position(e)) == e for every live entry e, over live entries only.  A lookup of a position of
  // bucket b reads entry 2b, entry 2b + 1 and the chain behind 2b + 1, and takes the first live entry with that
  // position: every bucket with a stored home entry is walked once, the first entry of each of ITS positions is
  // marked, and no live entry may stay unmarked.
  struct Seen {
    uint64_t pos;
    uint32_t order, rec;
  };
  std::vector<uint8_t> found(n, 0);
  std::vector<Seen> seen;
  for (uint32_t i = 0; i < n;) {
    const uint32_t b = ent[i].entry >> 1;
    seen.clear();
    auto visit = [&](uint32_t r) {
      const Entry& e = ent[r].e;
      if (e.idx >= 0 && block_hash(e.x, e.y, e.z, bucket_mask) == b)
        seen.push_back(Seen{(uint64_t)(uint16_t)e.x | (uint64_t)(uint16_t)e.y << 16 | (uint64_t)(uint16_t)e.z << 32,
                            (uint32_t)seen.size(), r});
    };
    if (!(ent[i].entry & 1u)) visit(i++);
    if (i < n && ent[i].entry == 2u * b + 1u) {  // the list head
      uint32_t j = i++;
      visit(j);
      // D3: the walk goes on over a dead node, but a block behind one is not marked
      for (bool dead = ent[j].e.idx < 0; ent[j].e.offset && (j = next(j)) != n; dead = dead || ent[j].e.idx < 0)
        if (!dead) visit(j);
    }
    std::sort(seen.begin(), seen.end(),
              [](const Seen& x, const Seen& y) { return x.pos != y.pos ? x.pos < y.pos : x.order < y.order; });
    for (size_t k = 0; k < seen.size(); ++k)
      if (k == 0 || seen[k].pos != seen[k - 1].pos) found[seen[k].rec] = 1;
  }
  for (uint32_t i = 0; i < n; ++i)
    if (ent[i].e.idx >= 0 && !found[i]) return false;
  return true;
}

// Opens and validates the WHOLE file (header, sections against it, entries, heap, the directory rule, checksum) on
// the host.  `want`, if given, is the engine's configuration: a file of another one is refused before its sections
// are read.
static int map_read_validate(const char* path, const MapHeader* want, MapContents* out, FILE** keep_open) {
  if (!path) return RATSDF_ERR_BAD_ARGUMENT;
  FILE* f = fopen(path, "rb");
  if (!f) return RATSDF_ERR_BAD_ARGUMENT;
  FileCloser fc{f};
  struct stat sb;
  if (fstat(fileno(f), &sb) != 0) return RATSDF_ERR_BAD_ARGUMENT;
  const uint64_t fsize = (uint64_t)sb.st_size;
  MapHeader& h = out->h;
  if (fsize < sizeof(h) + 8 || !read_all(f, &h, sizeof(h))) return RATSDF_ERR_BAD_ARGUMENT;
  if (memcmp(h.magic, kMapMagic, 8) != 0 || h.version != kMapVersion || h.header_size != sizeof(MapHeader))
    return RATSDF_ERR_BAD_ARGUMENT;
  if (h.block_bits < 1 || h.block_bits > 24 || h.bucket_bits < 9 || h.bucket_bits > 26) return RATSDF_ERR_BAD_ARGUMENT;
  if (want && (memcmp(&h.voxel_size, &want->voxel_size, 4) != 0 || memcmp(&h.truncation, &want->truncation, 4) != 0 ||
               h.block_bits != want->block_bits || h.bucket_bits != want->bucket_bits ||
               h.shard_rank != want->shard_rank || h.shard_count != want->shard_count ||
               h.shard_slab_bits != want->shard_slab_bits))
    return RATSDF_ERR_BAD_ARGUMENT;
  const int64_t num_block = (int64_t)1 << h.block_bits;
  const uint64_t num_entry = (uint64_t)2 << h.bucket_bits;
  if (h.segm_live != 0 && h.segm_live != 1) return RATSDF_ERR_BAD_ARGUMENT;
  if (h.num_free < 0 || h.num_free > num_block || h.free_low < 0 || h.free_low > h.num_free)
    return RATSDF_ERR_BAD_ARGUMENT;
  if (h.n_entries > num_entry || h.n_blocks > (uint64_t)num_block || h.n_blocks > h.n_entries ||
      (int64_t)h.n_blocks + h.num_free > num_block)
    return RATSDF_ERR_BAD_ARGUMENT;
  out->voxel_offset = sizeof(h) + (size_t)h.n_entries * sizeof(MapEntry) + (size_t)h.num_free * 4;
  const uint64_t voxel_bytes = (uint64_t)h.n_blocks * kMapRecordBytes + (uint64_t)(h.num_free - h.free_low) * kMapRgbBytes;
  if (fsize != (uint64_t)out->voxel_offset + voxel_bytes + 8) return RATSDF_ERR_BAD_ARGUMENT;
  MapHash hash;
  hash.update(&h, sizeof(h));
  out->entries.resize(h.n_entries);
  out->heap.resize((size_t)h.num_free);
  if (!read_all(f, out->entries.data(), out->entries.size() * sizeof(MapEntry)) ||
      !read_all(f, out->heap.data(), out->heap.size() * 4))
    return RATSDF_ERR_BAD_ARGUMENT;
  hash.update(out->entries.data(), out->entries.size() * sizeof(MapEntry));
  hash.update(out->heap.data(), out->heap.size() * 4);
  // entries: ascending, in range; a block's pool index in range, unused by any other block and at or above free_low
  // (indices below it have never been handed out); every other stored entry is a dead chain node (-1, offset != 0)
  std::vector<uint8_t> used((size_t)num_block, 0);
  out->pool_idx.clear();
  out->pool_idx.reserve(h.n_blocks);
  for (size_t i = 0; i < out->entries.size(); ++i) {
    const MapEntry& m = out->entries[i];
    if (m.entry >= num_entry || (i && m.entry <= out->entries[i - 1].entry)) return RATSDF_ERR_BAD_ARGUMENT;
    if (m.e.idx >= 0) {
      if (m.e.idx >= num_block || m.e.idx < h.free_low || used[(size_t)m.e.idx]) return RATSDF_ERR_BAD_ARGUMENT;
      used[(size_t)m.e.idx] = 1;
      out->pool_idx.push_back(m.e.idx);
    } else if (m.e.idx != -1 || m.e.offset == 0) {
      return RATSDF_ERR_BAD_ARGUMENT;
    }
  }
  if (out->pool_idx.size() != h.n_blocks) return RATSDF_ERR_BAD_ARGUMENT;
  // heap: free pool indices, each once, none of them a live block's; below free_low the never-used ones, in order
  for (size_t i = 0; i < out->heap.size(); ++i) {
    const int32_t v = out->heap[i];
    if (v < 0 || v >= num_block || used[(size_t)v] || ((int64_t)i < h.free_low && v != (int32_t)i))
      return RATSDF_ERR_BAD_ARGUMENT;
    used[(size_t)v] = 2;
  }
  out->pool_idx.insert(out->pool_idx.end(), out->heap.begin() + h.free_low, out->heap.end());
  // the header names a configuration an engine can have, and the entries are a directory that lookups can walk
  if (!map_header_ok(h) || !map_directory_ok(out->entries, h.bucket_bits)) return RATSDF_ERR_BAD_ARGUMENT;
  // voxels: hashed in passing (the load reads them again from here, after the checksum has been checked)
  {
    std::vector<uint8_t> buf((size_t)kMapChunk * kMapRecordBytes);
    uint64_t left = voxel_bytes;
    while (left) {
      const size_t n = (size_t)std::min<uint64_t>(left, buf.size());
      if (!read_all(f, buf.data(), n)) return RATSDF_ERR_BAD_ARGUMENT;
      hash.update(buf.data(), n);
      left -= n;
    }
  }
  uint64_t trailer = 0;
  if (!read_all(f, &trailer, 8) || trailer != hash.final()) return RATSDF_ERR_BAD_ARGUMENT;
  if (keep_open) {
    *keep_open = f;
    fc.f = nullptr;
  }
  return RATSDF_OK;
}

static MapHeader engine_header(const ratsdf_engine* e) {
  MapHeader h;
  memset(&h, 0, sizeof(h));
  memcpy(h.magic, kMapMagic, 8);
  h.version = kMapVersion;
  h.header_size = sizeof(MapHeader);
  h.voxel_size = e->vs;
  h.truncation = e->trunc;
  h.block_bits = e->block_bits;
  h.bucket_bits = e->bucket_bits;
  h.shard_rank = e->shard_rank;
  h.shard_count = e->shard_count;
  h.shard_slab_bits = e->shard_slab_bits;
  return h;
}

// Back to an empty map (creation state) after a load that failed half-way: never a mixture of two maps.
static int map_reset_empty(ratsdf_engine* e) {
  Table& t = e->tab;
  hipLaunchKernelGGL(k_init_table, dim3((t.num_entry + 255) / 256), dim3(256), 0, e->stream, t.entries, t.claim, t.occ,
                     t.num_entry, t.num_bucket);
  hipLaunchKernelGGL(k_init_heap, dim3((t.num_block + 255) / 256), dim3(256), 0, e->stream, e->pool.heap, t.num_block);
  const int32_t nf[4] = {t.num_block, 0, 0, t.num_block};  // num_free | error | n_sel | free_low
  HIPCHK(hipMemcpyAsync(&e->ctl->num_free, nf, sizeof(nf), hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipMemsetAsync(e->pool.rgbw, 0, (size_t)t.num_block * kMapRgbBytes, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  e->ever_sem = false;
  return rebuild_derived(e, true);
}

}  // namespace

extern "C" {

int ratsdf_map_file_info(const char* path, ratsdf_config* cfg, int64_t* n_blocks) {
  MapContents m;
  STCHK(map_read_validate(path, nullptr, &m, nullptr));
  if (cfg) {
    memset(cfg, 0, sizeof(*cfg));
    cfg->voxel_size = m.h.voxel_size;
    cfg->truncation = m.h.truncation;
    cfg->block_bits = m.h.block_bits;
    cfg->bucket_bits = m.h.bucket_bits;
    cfg->shard_rank = m.h.shard_rank;
    cfg->shard_count = m.h.shard_count;
    cfg->shard_slab_bits = m.h.shard_slab_bits;
  }
  if (n_blocks) *n_blocks = (int64_t)m.h.n_blocks;
  return RATSDF_OK;
}

int ratsdf_save_map(ratsdf_engine* e, const char* path) {
  ENTRY(e, path && *path);
  STCHK(e->settle());
  STCHK(e->sticky());  // (waits for the stream)
  // the stored entries in entry order, the free list and its two counters
  STCHK(e->select(kSelStored, GridBounds{}, &e->ctl->n_sel));
  int32_t c[4] = {0, 0, 0, 0};  // num_free | error | n_sel | free_low
  STCHK(e->read_small(c, &e->ctl->num_free, sizeof(c)));
  const uint32_t n_sel = (uint32_t)c[2];
  if (n_sel > e->vis_cap) return RATSDF_ERR_CAPACITY;
  std::vector<VisItem> items(n_sel);
  MapHeader h = engine_header(e);
  h.segm_live = e->ever_sem ? 1 : 0;
  h.num_free = c[0];
  h.free_low = c[3];
  if (h.num_free < 0 || h.num_free > e->tab.num_block) return RATSDF_ERR_DEVICE;
  std::vector<int32_t> heap((size_t)h.num_free);
  if (n_sel) HIPCHK(hipMemcpyAsync(items.data(), e->vis, (size_t)n_sel * sizeof(VisItem), hipMemcpyDeviceToHost, e->stream));
  if (h.num_free) HIPCHK(hipMemcpyAsync(heap.data(), e->pool.heap, heap.size() * 4, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  std::vector<MapEntry> entries(n_sel);
  std::vector<int32_t> pool_idx;
  pool_idx.reserve(n_sel);
  for (uint32_t i = 0; i < n_sel; ++i) {
    const VisItem& v = items[i];
    entries[i].entry = v.entry;
    entries[i].e = Entry{v.x, v.y, v.z, v.offset, v.idx};
    if (v.idx >= 0) {
      if (v.idx >= e->tab.num_block) return RATSDF_ERR_DEVICE;  // (a pool index still pending: never after a settled frame)
      pool_idx.push_back(v.idx);
    }
  }
  h.n_entries = n_sel;
  h.n_blocks = (uint32_t)pool_idx.size();
  {  // a directory that names a pool block twice cannot be resumed (a load refuses it): no file is written
    std::vector<uint8_t> seen((size_t)e->tab.num_block, 0);
    for (int32_t v : pool_idx) {
      if (seen[(size_t)v]) {
        fprintf(stderr, "[ratsdf] save_map: the directory names pool block %d twice; the map is not saved\n", v);
        return RATSDF_ERR_DEVICE;
      }
      seen[(size_t)v] = 1;
    }
  }
  if (h.free_low < 0 || h.free_low > h.num_free) return RATSDF_ERR_DEVICE;
  pool_idx.insert(pool_idx.end(), heap.begin() + h.free_low, heap.end());  // the free blocks that have been in use

  const std::string tmp_path = std::string(path) + ".tmp";
  FILE* f = fopen(tmp_path.c_str(), "wb");
  if (!f) return RATSDF_ERR_BAD_ARGUMENT;
  FileCloser fc{f};
  bool ok = true;
  MapHash hash;
  auto put = [&](const void* p, size_t n) {
    if (!ok || n == 0) return;
    hash.update(p, n);
    ok = fwrite(p, 1, n, f) == n;
  };
  put(&h, sizeof(h));
  put(entries.data(), entries.size() * sizeof(MapEntry));
  put(heap.data(), heap.size() * 4);
  // voxels: chunk k is packed into device staging k % 2 and copied into page-locked buffer k % 2 while the host
  // writes chunk k - 1 to the file
  int dev_st = RATSDF_OK;
  const std::vector<MapChunk> chunks = map_chunks(h.n_blocks, (uint32_t)(pool_idx.size() - h.n_blocks));
  if (ok && !chunks.empty()) {
    MapStaging sg;
    if (sg.init(pool_idx, e->stream) != RATSDF_OK) {
      dev_st = RATSDF_ERR_DEVICE;
    } else {
      auto enqueue = [&](size_t k) -> bool {
        const MapChunk& c = chunks[k];
        const int b = (int)(k & 1u);
        const dim3 grid(std::min<uint32_t>((c.n + 1) / 2, 2048u));
        if (c.full)
          hipLaunchKernelGGL(k_map_pack<true>, grid, dim3(256), 0, e->stream, e->pool, sg.d_idx + c.first, c.n,
                             reinterpret_cast<uint4*>(sg.dev[b]));
        else
          hipLaunchKernelGGL(k_map_pack<false>, grid, dim3(256), 0, e->stream, e->pool, sg.d_idx + c.first, c.n,
                             reinterpret_cast<uint4*>(sg.dev[b]));
        return hipGetLastError() == hipSuccess &&
               hipMemcpyAsync(sg.host[b], sg.dev[b], c.bytes(), hipMemcpyDeviceToHost, e->stream) == hipSuccess &&
               hipEventRecord(sg.ev[b], e->stream) == hipSuccess;
      };
      bool dev_ok = enqueue(0) && (chunks.size() < 2 || enqueue(1));
      for (size_t k = 0; k < chunks.size() && dev_ok && ok; ++k) {
        const int b = (int)(k & 1u);
        dev_ok = hipEventSynchronize(sg.ev[b]) == hipSuccess;
        if (!dev_ok) break;
        put(sg.host[b], chunks[k].bytes());
        if (k + 2 < chunks.size()) dev_ok = enqueue(k + 2);
      }
      if (!dev_ok) dev_st = RATSDF_ERR_DEVICE;
    }
  }
  if (dev_st == RATSDF_OK && ok) {
    const uint64_t sum = hash.final();
    ok = fwrite(&sum, 1, 8, f) == 8;
  }
  ok = (fflush(f) == 0) && ok;
  fc.f = nullptr;
  ok = (fclose(f) == 0) && ok;
  if (dev_st != RATSDF_OK || !ok) {
    (void)remove(tmp_path.c_str());
    return dev_st != RATSDF_OK ? dev_st : RATSDF_ERR_BAD_ARGUMENT;
  }
  if (rename(tmp_path.c_str(), path) != 0) {
    (void)remove(tmp_path.c_str());
    return RATSDF_ERR_BAD_ARGUMENT;
  }
  return RATSDF_OK;
}

int ratsdf_load_map(ratsdf_engine* e, const char* path) {
  ENTRY(e, path);
  MapContents m;
  FILE* f = nullptr;
  const MapHeader want = engine_header(e);
  STCHK(map_read_validate(path, &want, &m, &f));
  FileCloser fc{f};
  // the file is good: everything the engine has enqueued finishes, then the map is replaced
  HIPCHK(hipStreamSynchronize(e->stream));
  STCHK(e->ring.drain());
  const MapHeader& h = m.h;
  Table& t = e->tab;
  int st = RATSDF_OK;
  MapStaging sg;
  DevMem entries_mem;
  StreamDrain drain{e->stream};
  do {
    if (sg.init(m.pool_idx, e->stream) != RATSDF_OK) { st = RATSDF_ERR_DEVICE; break; }
    hipLaunchKernelGGL(k_init_table, dim3((t.num_entry + 255) / 256), dim3(256), 0, e->stream, t.entries, t.claim,
                       t.occ, t.num_entry, t.num_bucket);
    if (!m.entries.empty()) {
      if (entries_mem.alloc(m.entries.size() * sizeof(MapEntry)) != RATSDF_OK) { st = RATSDF_ERR_DEVICE; break; }
      uint4* d_entries = entries_mem.as<uint4>();
      if (hipMemcpyAsync(d_entries, m.entries.data(), m.entries.size() * sizeof(MapEntry), hipMemcpyHostToDevice,
                         e->stream) != hipSuccess) { st = RATSDF_ERR_DEVICE; break; }
      hipLaunchKernelGGL(k_map_scatter_entries, dim3((unsigned)((m.entries.size() + 255) / 256)), dim3(256), 0,
                         e->stream, t, d_entries, (uint32_t)m.entries.size());
    }
    if (!m.heap.empty() && hipMemcpyAsync(e->pool.heap, m.heap.data(), m.heap.size() * 4, hipMemcpyHostToDevice,
                                          e->stream) != hipSuccess) { st = RATSDF_ERR_DEVICE; break; }
    const int32_t c[4] = {h.num_free, 0, 0, h.free_low};  // num_free | error | n_sel | free_low
    if (hipMemcpyAsync(&e->ctl->num_free, c, sizeof(c), hipMemcpyHostToDevice, e->stream) != hipSuccess ||
        hipStreamSynchronize(e->stream) != hipSuccess) { st = RATSDF_ERR_DEVICE; break; }
    // voxels: the host reads chunk k into page-locked buffer k % 2 while chunk k - 1 goes up and is unpacked
    if (fseek(f, (long)m.voxel_offset, SEEK_SET) != 0) { st = RATSDF_ERR_BAD_ARGUMENT; break; }
    // (the never-used blocks below free_low hold colour 0, as after creation)
    if (h.free_low > 0 && hipMemsetAsync(e->pool.rgbw, 0, (size_t)h.free_low * kMapRgbBytes, e->stream) != hipSuccess) {
      st = RATSDF_ERR_DEVICE;
      break;
    }
    const std::vector<MapChunk> chunks = map_chunks(h.n_blocks, (uint32_t)(h.num_free - h.free_low));
    for (size_t k = 0; k < chunks.size(); ++k) {
      const MapChunk& c = chunks[k];
      const int b = (int)(k & 1u);
      if (k >= 2 && hipEventSynchronize(sg.ev[b]) != hipSuccess) { st = RATSDF_ERR_DEVICE; break; }
      if (!read_all(f, sg.host[b], c.bytes())) { st = RATSDF_ERR_BAD_ARGUMENT; break; }
      if (hipMemcpyAsync(sg.dev[b], sg.host[b], c.bytes(), hipMemcpyHostToDevice, e->stream) != hipSuccess) {
        st = RATSDF_ERR_DEVICE;
        break;
      }
      const dim3 grid(std::min<uint32_t>((c.n + 1) / 2, 2048u));
      if (c.full)
        hipLaunchKernelGGL(k_map_unpack<true>, grid, dim3(256), 0, e->stream, e->pool, sg.d_idx + c.first, c.n,
                           reinterpret_cast<const uint4*>(sg.dev[b]));
      else
        hipLaunchKernelGGL(k_map_unpack<false>, grid, dim3(256), 0, e->stream, e->pool, sg.d_idx + c.first, c.n,
                           reinterpret_cast<const uint4*>(sg.dev[b]));
      if (hipGetLastError() != hipSuccess || hipEventRecord(sg.ev[b], e->stream) != hipSuccess) {
        st = RATSDF_ERR_DEVICE;
        break;
      }
    }
    if (st != RATSDF_OK) break;
    if (hipStreamSynchronize(e->stream) != hipSuccess) { st = RATSDF_ERR_DEVICE; break; }
    // occupancy bits, Table::active, claims, counters, the delta log's overflow mark, the error: as ratsdf_recover
    st = rebuild_derived(e, true);
  } while (false);
  if (st != RATSDF_OK) {
    (void)map_reset_empty(e);
    return st;
  }
  e->ever_sem = h.segm_live != 0;
  return RATSDF_OK;
}

}  // extern "C"
