// ratsdf_engine.hip -- host side of the MI355X-native TSDF engine: device memory, the per-frame
// launch sequence on one HIP stream, and the C ABI of include/ratsdf.h.
//
// Replaces TSDFGrid (utils/tsdf/voxel_tsdf.cu:376-559,847-883), VoxelHashTable / VoxelMemPool host
// parts (voxel_hash.cu:25-44,225; voxel_mem.cu:13-35,63-67).  gfx950 only; there is no CPU path.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>

#include "kernels_frame.h"
#include "kernels_mesh.h"
#include "kernels_sample.h"
#include "kernels_esdf.h"
#include "kernels_surface.h"
#include "kernels_surface_mesh.h"
#include "kernels_cluster_mesh.h"
#include "kernels_regions.h"
#include "kernels_cost.h"
#include "kernels_exposure.h"
#include "kernels_score.h"
#include "kernels_score_mesh.h"
#include "kernels_fuse.h"
#include "kernels_resample.h"
#include "kernels_coarsen.h"
#include "hip_mem.h"
#include "hip_handles.h"
#include "stage_plan.h"
#include "workspace.h"
#include "cand_shares.h"
#include "../../include/ratsdf_sample.h"
#include "../../include/ratsdf_esdf.h"
#include "../../include/ratsdf_surface.h"
#include "../../include/ratsdf_surface_mesh.h"
#include "../../include/ratsdf_cluster_mesh.h"
#include "../../include/ratsdf_regions.h"
#include "../../include/ratsdf_cost.h"
#include "../../include/ratsdf_score.h"
#include "../../include/ratsdf_score_mesh.h"

static_assert(sizeof(ratsdf_sample) == 32 && offsetof(ratsdf_sample, flags) == 25, "ratsdf_sample layout");
static_assert(ratsdf::kWsScanTile == (size_t)ratsdf::kScanTile, "scan_tiles() counts the tiles of kernels_mesh.h's scan");

using namespace ratsdf;

#define HIPCHK(expr)                                                                      \
  do {                                                                                    \
    hipError_t err__ = (expr);                                                            \
    if (err__ != hipSuccess) {                                                            \
      fprintf(stderr, "[ratsdf] HIP error %s at %s:%d: %s\n", hipGetErrorName(err__),     \
              __FILE__, __LINE__, #expr);                                                 \
      return RATSDF_ERR_DEVICE;                                                           \
    }                                                                                     \
  } while (0)
// ... and a call that reports a RATSDF_* status of its own (an allocation through hip_mem.h's owners above all)
#define STCHK(expr) do { const int st__ = (expr); if (st__ != RATSDF_OK) return st__; } while (0)

// Scoped "current device" of the calling thread: HIP's current device is per thread and defaults to
// 0, so every entry point that allocates or launches selects the engine's device first and restores
// the caller's on the way out.
struct DeviceGuard {
  int prev = -1;
  bool changed = false;
  bool selected = true;  // false: the engine's device could not be made current -- every entry point
                         // then returns RATSDF_ERR_DEVICE instead of working on the caller's device
                         // with another device's pointers
  explicit DeviceGuard(int device) {
    if (device < 0) return;  // (no engine: the entry point reports the bad argument itself)
    if (hipGetDevice(&prev) != hipSuccess) {
      selected = false;
      return;
    }
    if (prev != device) {
      changed = hipSetDevice(device) == hipSuccess;
      selected = changed;
    }
  }
  bool ok() const { return selected; }
  ~DeviceGuard() {
    if (changed) (void)hipSetDevice(prev);
  }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};

namespace {

__global__ void k_init_table(Entry* entries, uint32_t* claim, unsigned long long* occ,
                             uint32_t num_entry, uint32_t num_bucket) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < num_entry) entries[i] = Entry{0, 0, 0, 0, -1};  // init_hash_table_kernel, voxel_hash.cu:14-17
  if (i < num_bucket) claim[i] = kInf;
  if (i < (num_entry + 63) / 64) occ[i] = 0ull;
}
// block_threads() (device_types.h) reads the workgroup size from a fixed place in the implicit kernel arguments:
// checked once per engine against blockDim.x, with an odd size, so that a toolchain that lays them out
// differently fails ratsdf_create instead of computing garbage.
__global__ void k_check_block_threads(uint32_t* out) {
  if (threadIdx.x == 0) out[0] = block_threads() == blockDim.x ? blockDim.x : 0u;
}

// ratsdf_recover: what the directory says, into the structures derived from it.  One lane per hash entry: a live
// entry sets its occupancy bit, fills its slot of Table::active and marks its pool block as in use; an entry the
// chained-bucket resolver placed but whose commit never ran (pool index pending) is emptied -- its chain links stay,
// a dead node in a chain is walked over.
__global__ void k_recover_scan(Table tab, uint32_t* unused) {
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= tab.num_entry) return;
  uint32_t* pe = reinterpret_cast<uint32_t*>(tab.entries + e);
  const int32_t idx = (int32_t)pe[2];
  if (idx == kPlaceholderIdx || idx >= tab.num_block) {
    pe[2] = (uint32_t)-1;
    return;
  }
  if (idx < 0) return;
  atomicOr(&tab.occ[e >> 6], 1ull << (e & 63));
  reinterpret_cast<uint4*>(tab.active)[idx] = make_uint4(pe[0], pe[1] & 0xFFFFu, (uint32_t)idx, e);
  unused[idx] = 0u;
}
// ... and the free list: the pool blocks no entry names, in ascending order (the lowest positions of the heap hold
// the lowest indices, as after creation: AquireBlock pops from the top)
__global__ void k_recover_heap(const uint32_t* unused, const uint32_t* pos, int32_t* heap, int32_t n) {
  const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && unused[i]) heap[pos[i]] = i;
}
__global__ void k_fill_u32(uint32_t* p, uint32_t v, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

__global__ void k_init_heap(int32_t* heap, int32_t n) {   // heap_init_kernel, voxel_mem.cu:6-11
  const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) heap[i] = i;
}

constexpr uint32_t kSlowCap = kSlowSortCap;
constexpr int kDefaultVPL = 2;  // voxels per lane in k_integrate (RATSDF_VPL=2|4|8 overrides: tuning)
constexpr uint32_t kSlowDelCap = 1u << 16;

}  // namespace

// The head of an entry point, in the order that is contract: the engine's (or group's) device made current for the
// call, RATSDF_ERR_DEVICE if it cannot be; then RATSDF_ERR_BAD_ARGUMENT for a null handle or when `args_ok` -- read
// only with a handle -- does not hold.  An entry point that needs the last frame's carve pass completed says
// STCHK(e->settle()) next.
#define ENTRY(h, args_ok)                             \
  DeviceGuard guard((h) ? (h)->device : -1);          \
  if (!guard.ok()) return RATSDF_ERR_DEVICE;          \
  if (!(h) || !(args_ok)) return RATSDF_ERR_BAD_ARGUMENT

// Nothing queued may outlive a function's local buffers (hip_mem.h: the owner never synchronises).  Declared AFTER
// them, it drains the stream before they are freed, on every way out.
struct StreamDrain {
  hipStream_t stream;
  ~StreamDrain() { (void)hipStreamSynchronize(stream); }
};

#include "stage_ring.inc"

// The workspace of a box read-out: grown and carved by ratsdf_engine::workspace, with a layout of workspace.h.
struct Workspace {
  DevMem mem;
  size_t cap = 0;  // items (voxels, cells of the block grid) it was laid out for
};

// What the engine owns of device and page-locked host memory: every buffer has ONE owner (hip_mem.h), and
// ~ratsdf_engine drops them all by assigning an empty EngineMem.  `fixed` owns what is allocated once, at creation, pix_mem / rank_mem
// the image-sized buffers (ensure_image): the typed pointers in Table, Pool and the engine's fields are views of them
// (those structures go to the kernels by value).  A buffer that grows on demand is its own owner; a capacity counted
// in other units than bytes (pixels, voxels, a Workspace's items) is zero while its buffers are replaced, so a failed
// grow is retried.
struct EngineMem {
  std::vector<DevMem> fixed, pix_mem, rank_mem;
  HostMem h_err_page;  // (ratsdf_engine::h_err)
  DevMem d_out;        // results on their way to the caller's host memory, and the page-locked buffer they pass
  HostMem h_out;       // through: ONE pair for every host-result entry point (ratsdf_engine::staging / download)
  // the workspaces of the box read-outs, one buffer each (calls of two read-outs queued back to back share nothing)
  Workspace ws_esdf;          // ratsdf_esdf*: esdf_layout, per voxel
  Workspace ws_surface;       // ratsdf_surface_points*: surface_layout, per cell of the block grid
  Workspace ws_surface_mesh;  // ratsdf_surface_mesh*: surface_mesh_layout, per cell of the block grid
  DevMem d_surface_mesh_tab;  // ... and its case tables, built on first use
  Workspace ws_cluster_mesh;  // ratsdf_cluster_mesh*: cluster_mesh_layout, per cell of the block grid
  Workspace ws_regions;       // ratsdf_regions*: regions_layout, per voxel
  Workspace ws_cost;          // ratsdf_cost_to_go*: cost_layout, per voxel (an ESDF workspace of its own inside)
  Workspace ws_exposure;      // ratsdf_exposure*: exposure_layout, per voxel
  Workspace ws_score;         // ratsdf_score_labels and ratsdf_score_mesh: score_layout, one item
  DevMem d_fuse;       // map fusion (fuse.inc): positions | source pool indices | done bits | counters of one chunk
  DevMem d_occ;        // ray casting: hashed occupancy of the blocks (kernels_raycast.h), built per rendering
  DevMem d_mc;         // marching-cubes tables, built on first use

  template <class T>
  static int own(std::vector<DevMem>& set, T** view, size_t bytes) {
    set.emplace_back();
    const int st = set.back().alloc(bytes);
    *view = set.back().as<T>();  // (null after a failure)
    return st;
  }
};

// Timing of the dominant kernel (k_integrate / k_integrate_g) with HIP events attached to the dispatch itself; an
// engine and a group each hold one (declared behind the stream it times: its events go before the stream does).
struct KernelTimer {
  bool on = false;
  int mode = 1;  // 1: every 4th frame, sums only; 2 (engines): every frame, per-frame records
  std::vector<std::pair<HipEvent, HipEvent>> prof_events;
  size_t used = 0;
  uint64_t frame = 0;
  double ms = 0;
  int64_t n = 0;
  std::vector<float> k_us, period_us;  // mode 2: kernel time of a frame / start-to-start period

  // pairs for the next `k` timed frames exist afterwards (what may fail, apart from the launches)
  int reserve(size_t k) {
    while (prof_events.size() < used + k) {
      HipEvent a, b;
      STCHK(a.create(hipEventDefault));
      STCHK(b.create(hipEventDefault));
      prof_events.emplace_back(std::move(a), std::move(b));
    }
    return RATSDF_OK;
  }
  // the events of the next frame's launch: a pair when the frame is one of the timed ones, nulls (= a plain launch)
  // otherwise (sampled: events perturb the stream; mode 2 times every frame, for latency distributions)
  std::pair<hipEvent_t, hipEvent_t> take() {
    if (!on || (mode != 2 && frame++ % 4 != 0) || used == prof_events.size()) return {nullptr, nullptr};
    const auto& ev = prof_events[used++];
    return {ev.first, ev.second};
  }
  bool full() const { return on && used >= (mode == 2 ? 60000u : 4096u); }
  // `final`: nothing follows the timed frames (a read-out).  An intermediate drain in mode 2 (the event pool is
  // full) keeps the LAST pair for the next drain: its period ends at the start of a frame that has not been
  // launched yet, and k_us / period_us must stay index-aligned (ratsdf_profile_read_frames).
  int drain(hipStream_t stream, bool final = true) {
    if (!used) return RATSDF_OK;
    HIPCHK(hipStreamSynchronize(stream));
    const bool keep_last = mode == 2 && !final && used > 1;
    const size_t cnt = keep_last ? used - 1 : used;
    for (size_t i = 0; i < cnt; ++i) {
      float t = 0;
      HIPCHK(hipEventElapsedTime(&t, prof_events[i].first, prof_events[i].second));
      ms += t;
      ++n;
      if (mode == 2) {
        k_us.push_back(t * 1e3f);
        float gap = 0;  // consecutive frames: start of this frame's k_integrate to the next one's (last frame: 0)
        if (i + 1 < used) HIPCHK(hipEventElapsedTime(&gap, prof_events[i].first, prof_events[i + 1].first));
        period_us.push_back(gap * 1e3f);
      }
    }
    if (keep_last) std::swap(prof_events[0], prof_events[used - 1]);
    used = keep_last ? 1 : 0;
    return RATSDF_OK;
  }
  // the sums since the last read-out
  int read(hipStream_t stream, double* ms_out, int64_t* launches) {
    const int st = drain(stream);
    if (ms_out) *ms_out = ms;
    if (launches) *launches = n;
    ms = 0;
    n = 0;
    return st;
  }
};

struct ratsdf_engine : EngineMem {
  int device = 0;
  // The handles (hip_handles.h) leave in the reverse of their declaration: `ring`, then `timer`'s events, then
  // `stream` -- behind the drain, the graphs and the memory, which are ~ratsdf_engine's.
  HipStream stream;
  KernelTimer timer;         // profiling of the dominant kernel
  StageRing ring;            // staging of the host-image entry points (stage_ring.inc)
  float vs = 0, trunc = 0;
  int block_bits = 0, bucket_bits = 0;
  int shard_rank = 0, shard_count = 1, shard_slab_bits = 2;
  int S = 3;
  int vpl = kDefaultVPL;
  int debug = 0;
  unsigned integrate_grid = 4096;
  bool grid_from_env = false;

  Table tab{};
  Pool pool{};
  Ctl* ctl = nullptr;
  ratsdf_frame_stats* d_stats = nullptr;
  int staging(size_t dev_bytes, size_t host_bytes);
  int download(void* dst, const void* d_src, size_t bytes);
  template <class Work>
  int workspace(Workspace& ws, size_t n, void (*layout)(WsCursor&, size_t, Work*), Work* w);
  uint32_t* h_err = nullptr;  // page-locked landing place of the sticky error word (sticky())
  EngineDev* d_eng = nullptr;  // device copy of the engine record (device_types.h)

  // image-sized scratch
  size_t pix_cap = 0, rank_cap = 0, cur_nranks = 0;
  float4* texA[2] = {nullptr, nullptr};  // packed per-pixel texels, double-buffered: the candidate
  uint32_t* texB[2] = {nullptr, nullptr};  // pass of frame f+1 writes while k_integrate(f) reads
  CandSet cand[2] = {};                  // candidate sets, used alternately (kernels_cand.h)
  uint32_t* cand_count = nullptr;        // both sets' list counters
  unsigned parity = 0;                   // which texel buffer / candidate set the NEXT frame uses
  bool cand_ready = false;               // that frame's candidate pass has already been enqueued
  bool cand_split_env = false;
// (compile-time defaults that tools/ build variants of for same-box sweeps)
#ifndef RATSDF_GRID_VGA
#define RATSDF_GRID_VGA 4096
#endif
#ifndef RATSDF_GRID_HD
#define RATSDF_GRID_HD 8192
#endif
#ifndef RATSDF_CAND_SPLIT_HD
#define RATSDF_CAND_SPLIT_HD 100
#endif
#ifndef RATSDF_CAND_SPLIT_DEFAULT
#define RATSDF_CAND_SPLIT_DEFAULT 10  // (round 5, with the cheaper visible-list role: 5 - 15 % measure the same, 0 and 20 % are 1.5 % slower)
#endif
  unsigned cand_split = RATSDF_CAND_SPLIT_DEFAULT;  // percent of the look-ahead pass placed in k_front,
  unsigned cand_split_b = 0;             // in k_alloc_rank; the rest rides in k_integrate
  bool fused_serial = true;              // the frame's serial role rides in k_integrate (no k_alloc_rank)
  // ... or, in ordinary frames, at the tail of k_front (front_tail_role, RATSDF_FRONT_TAIL=1).  Off by default:
  // measured (profiles/r04_front_tail.txt) it shortens k_integrate to the pure voxel update (16.8 -> 12.1 us
  // at 640x480 with the whole look-ahead pass in k_front) but lengthens k_front by more (8.6 -> 15.8 us): the
  // role is ~7 us of dependent round trips wherever it runs, and inside k_integrate it hides behind the update.
  bool front_tail = false;
  uint32_t front_prio = 0u;              // 2: k_front's directory workgroups run at raised wave priority (+1 %)
  bool sort_lists = false;               // diagnostic build, RATSDF_SORT_LISTS=1: work lists sorted by image tile on the host (experiment)
  bool inline_off = false;               // diagnostic build, RATSDF_INLINE_CAND=0: k_cand + k_front for frames without look-ahead
  int commit_rot_env = -1;               // RATSDF_COMMIT_ROT: first committing workgroup (measurements)
  // With the serial role in the launch: which update workgroups take the frame's commits.  A grid of
  // at most two rounds of resident workgroups (256 CUs x 8): the first ones, which wait for the role
  // after their first block (anything later is the tail).  More rounds: the second round.
  // (`launch_wgs`: update workgroups of the whole launch -- S slices of `grid` for a group, whose
  // later slices start on a full machine whatever their size.)
  uint32_t commit_rotation(unsigned grid, unsigned launch_wgs) const {
    if (commit_rot_env >= 0) return (uint32_t)commit_rot_env < grid ? (uint32_t)commit_rot_env : 0u;
    if (launch_wgs < 8192u) return 0u;
    return grid > 4096u ? 3072u : grid / 4u * 3u;  // profiles/r02_commit_rot_sweep.txt
  }
  uint32_t* serial_scratch = nullptr;    // its scratch for the general paths (kSerialLdsBytes)
  unsigned cand_parts_env = 0;           // RATSDF_CAND_PARTS: consumer workgroups per candidate list
  unsigned cand_wgs = 248;               // look-ahead workgroups per host kernel (about one per CU)
  // dynamic LDS of k_alloc_rank: the serial role needs kSerialLdsBytes; asking for more than half a
  // CU's LDS keeps the look-ahead workgroups of the launch off the serial workgroup's CU (sharing it
  // stretched the frame's critical path by a quarter)
  unsigned serial_lds = 100 * 1024;
  Request* req = nullptr;
  uint32_t req_cap = 0;
  uint32_t* abitmap = nullptr;   // rank bitmap, many-request path only (whole 32-word groups)
  uint32_t* asummary = nullptr;  // one bit per group
  uint32_t* req_k = nullptr;     // rank among the winners, per request
  uint32_t* win_ranks = nullptr; // raster ranks of the winners (few-winners path)
  uint32_t* aprefix = nullptr;       // per-word prefix of the rank bitmap (set groups only)
  uint32_t awords_cap = 0, asum_words = 0;

  SlowRequest* slow = nullptr;
  XLock* xlocks = nullptr;
  unsigned long long* sort_scratch = nullptr;  // resolver's sort keys beyond the LDS capacity

  // directory-sized scratch
  unsigned long long* masks = nullptr;  // selection / visibility mask, one bit per directory entry
  uint32_t* wg_count = nullptr;         // selected entries per kVisWG-word workgroup
  uint32_t nwg = 0;
  VisItem* vis = nullptr;
  // per frame parity (frame f appends while the end of frame f-1's carve pass still reads its own):
  DelItem* del_list[2] = {nullptr, nullptr};  // slot-0 deletes of a pass (pool release pending)
  uint32_t* upd_wg[2] = {nullptr, nullptr};   // voxels updated, per k_integrate workgroup (mod 1024)
  bool pending = false;            // the last pass still owes its carve_finalize (kernels_carve.h)
  uint32_t* dbitmap = nullptr;   // delete bitmap indexed by hash entry (self-cleaning)
  uint32_t* dsummary = nullptr;
  uint32_t* dprefix = nullptr;
  uint32_t vis_cap = 0;   // total items of `vis`
  uint32_t seg_cap = 0;   // items per work list (vis holds kNumLists + 1 segments)
  uint32_t dwords = 0;
  SlowDelete* slowdel[2] = {nullptr, nullptr};


  // a frame with ht / lt has been integrated, or blocks were imported with their probabilities (FrameParams::segm_live)
  mutable bool ever_sem = false;
  bool sync_integrate = false;         // RATSDF_SYNC_INTEGRATE=1: wait for every frame (the round-3 behaviour)

  // HIP graphs of the batch entry point (ratsdf_integrate_device_batch): the launches of an n-frame batch are
  // captured once per (image size, n) -- the kernels of the group path with one member, which take every
  // per-frame operand (pose, intrinsics, image pointers, counter-set parity) from a FrameJob table in device
  // memory -- and replayed with a fresh table.  Host cost per frame: a table row instead of two launches.
  // (destruction, the reverse of the declarations: the executable and the graph, then the tables' events and memory;
  // the engine's stream has been drained before a BatchGraph goes)
  struct BatchGraph {
    int H = 0, W = 0, n = 0;
    uint64_t last_use = 0;
    DevMem d_jobs;   // FrameJob[n]
    TwinTable jobs;  // ... and its page-locked sides
    HipGraph graph;
  };
  std::vector<BatchGraph> graphs;
  bool use_graphs = true;                // RATSDF_GRAPH=0: every frame launched by itself
  uint64_t graph_clock = 0;
  int batch_graph(int n, int H, int W, BatchGraph** out);
  struct GraphShape {
    int H, W, n;
  };
  std::vector<GraphShape> graph_failed;  // shapes whose capture failed once: launched frame by frame from then on

  uint64_t prof_batch = 0;   // (mode 1: every fourth batch carries the events, ratsdf_integrate_device_batch)

  ~ratsdf_engine();
  int ensure_image(size_t npix, size_t nranks);
  EngineDev record() const;
  int upload_record();
  RankBufs rank_bufs(uint32_t nranks) const;
  int alloc_rank(uint32_t nranks, unsigned par, const CandJob* next = nullptr, bool frame = false);
  int commit_pass(uint32_t nranks, unsigned par);
  int settle();
  void abandon_pipeline(int frames_launched = 0, bool clear_next = false);
  CarveBufs carve_bufs(unsigned par) const;
  int select(int mode, const GridBounds& gb, uint32_t* count_slot);
  struct FrameIn {
    const void *rgb, *depth, *ht, *lt;
    const ratsdf_intrinsics* K;
    const ratsdf_pose* T;
    // ht and lt count only together (modules/tsdf_module.cc:27-31)
    static FrameIn of(const void* rgb, const void* depth, const void* ht, const void* lt, const ratsdf_intrinsics* K,
                      const ratsdf_pose* T) {
      if (!ht || !lt) ht = lt = nullptr;
      return FrameIn{rgb, depth, ht, lt, K, T};
    }
    // ... element i of a batch's arrays (`ht` / `lt`: the arrays themselves may be missing)
    static FrameIn at(size_t i, const void* const* rgb, const void* const* depth, const void* const* ht,
                      const void* const* lt, const ratsdf_intrinsics* K, const ratsdf_pose* T) {
      return of(rgb[i], depth[i], ht ? ht[i] : nullptr, lt ? lt[i] : nullptr, &K[i], &T[i]);
    }
  };
  FrameParams frame_params(const FrameIn& in, int H, int W, float md) const;
  void fill_job(FrameJob& j, const FrameIn& in, int H, int W, float md, unsigned par) const;
  CandJob cand_job(const FrameIn& in, const FrameParams& P, unsigned par) const;
  int frame(const FrameIn& cur, const FrameIn* next, int H, int W, float md);
  int sticky();
  int read_small(void* dst, const void* dev_src, size_t bytes);
  FrameParams base_params() const;
  struct Geom {
    unsigned n_vis_wg, parts, n_front_wg, n_cand_wg, grid;
    AheadGeom a, b, c;  // look-ahead shares of k_front, k_alloc_rank, k_integrate
  };
  Geom geometry(int H, int W, bool has_next, int split_a, int split_b, bool b_launched) const;
  int lookahead_split(size_t npix) const;
  bool graph_eligible(int n, int H, int W) const;
  // the frame in slot i of the staging ring, as the frame path takes it
  FrameIn ring_input(int i, size_t npix, const ratsdf_intrinsics* K, const ratsdf_pose* T, bool sem) const {
    const uint8_t* d = ring.slot(i, npix).d;
    return FrameIn{d + npix * 12, d, sem ? d + npix * 4 : nullptr, sem ? d + npix * 8 : nullptr, K, T};
  }
  int host_image_fail(int status);
};

FrameParams ratsdf_engine::base_params() const {
  FrameParams P;
  memset(&P, 0, sizeof(P));
  P.T = Se3{Quat{0, 0, 0, 1}, V3{0, 0, 0}};
  P.Ti = P.T;
  P.K = Intr{1, 1, 0, 0};
  P.Ki = P.K;
  P.vs = vs;
  P.trunc = trunc;
  P.md = 0;
  P.W = P.H = 0;
  P.S = 1;
  P.has_sem = 0;
  P.segm_live = 1;
  P.shard_rank = shard_rank;
  P.shard_count = shard_count;
  P.shard_slab_bits = shard_slab_bits;
  P.shard_bias = (32768 + shard_count - 1) / shard_count * shard_count;
  P.shard_magic = shard_count > 1 ? 0xFFFFFFFFu / (uint32_t)shard_count + 1u : 0u;
  P.debug = debug;
  return P;
}

// What is not ownership: the streams are drained, and the order -- the graphs, then the memory (the base class would
// go last), then the members' handles: the ring's, the timer's, the stream (see their declarations).
ratsdf_engine::~ratsdf_engine() {
  if (stream) (void)hipStreamSynchronize(stream);
  (void)ring.drain();
  if (stream) (void)hipStreamSynchronize(stream);
  graphs.clear();
  static_cast<EngineMem&>(*this) = EngineMem();
}

RankBufs ratsdf_engine::rank_bufs(uint32_t nranks) const {
  RankBufs rb;
  rb.req = req;
  rb.req_cap = req_cap;
  rb.req_k = req_k;
  rb.win_ranks = win_ranks;
  rb.slow = slow;
  rb.slow_cap = kSlowCap;
  rb.xlocks = xlocks;
  rb.bitmap = abitmap;
  rb.summary = asummary;
  rb.prefix = aprefix;
  rb.nwords = (nranks + 31) / 32;
  rb.sort_scratch = sort_scratch;
  return rb;
}

EngineDev ratsdf_engine::record() const {
  EngineDev r;
  memset(&r, 0, sizeof(r));
  r.tab = tab;
  r.pool = pool;
  r.cb[0] = carve_bufs(0);
  r.cb[1] = carve_bufs(1);
  r.rb = rank_bufs((uint32_t)cur_nranks);
  r.ctl = ctl;
  r.stats = d_stats;
  r.slow = slow;
  r.serial_scratch = serial_scratch;
  r.slow_cap = kSlowCap;
  r.seg_cap = seg_cap;
  r.vis = vis + kFreshCap;  // (the frame kernels' view: device_types.h, kFreshCap)
  for (int i = 0; i < 2; ++i) {
    r.texA[i] = texA[i];
    r.texB[i] = texB[i];
    r.cand[i] = cand[i];
  }
  return r;
}

// the device copy follows every (re)allocation; in stream order, so launches already enqueued keep
// reading the record they were enqueued with
int ratsdf_engine::upload_record() {
  const EngineDev r = record();
  HIPCHK(hipMemcpyAsync(d_eng, &r, sizeof(r), hipMemcpyHostToDevice, stream));
  HIPCHK(hipStreamSynchronize(stream));  // `r` is a stack object
  return RATSDF_OK;
}

int ratsdf_engine::ensure_image(size_t npix, size_t nranks) {
  if (npix <= pix_cap && nranks == cur_nranks) return RATSDF_OK;
  HIPCHK(hipStreamSynchronize(stream));
  // What describes a set of buffers (capacity, the sizes the kernels are given, the views) is cleared before the set is
  // replaced and written once ALL of it exists: after a failure the next call comes through here again.
  if (npix > pix_cap) {
    pix_cap = 0;
    pix_mem.clear();
    texA[0] = texA[1] = nullptr;
    texB[0] = texB[1] = nullptr;
    for (int i = 0; i < 2; ++i) {
      STCHK(own(pix_mem, &texA[i], npix * sizeof(float4)));
      STCHK(own(pix_mem, &texB[i], npix * sizeof(uint32_t)));
    }
    pix_cap = npix;
  }
  if (nranks > rank_cap) {
    rank_cap = cur_nranks = 0;
    req_cap = awords_cap = asum_words = cand[0].seg_cap = cand[1].seg_cap = 0;
    rank_mem.clear();
    req = nullptr;
    req_k = abitmap = asummary = aprefix = nullptr;
    cand[0].list = cand[1].list = nullptr;
    // candidate lists: every sample of the image could in principle ask for a different block
    const uint32_t seg = (uint32_t)((nranks + kCandSegs - 1) / kCandSegs) + 1024;
    const uint32_t words = ((uint32_t)((nranks + 31) / 32) + kGroupWords - 1) / kGroupWords * kGroupWords;
    const uint32_t sum_words = (words / kGroupWords + 31) / 32;
    for (int i = 0; i < 2; ++i) STCHK(own(rank_mem, &cand[i].list, (size_t)seg * kCandSegs * sizeof(uint4)));
    STCHK(own(rank_mem, &req, (size_t)(uint32_t)nranks * sizeof(Request)));
    STCHK(own(rank_mem, &req_k, (size_t)(uint32_t)nranks * 4));
    STCHK(own(rank_mem, &abitmap, (size_t)words * 4));
    STCHK(own(rank_mem, &asummary, (size_t)sum_words * 4));
    STCHK(own(rank_mem, &aprefix, (size_t)words * 4));
    cand[0].seg_cap = cand[1].seg_cap = seg;
    req_cap = (uint32_t)nranks;
    awords_cap = words;
    asum_words = sum_words;
    rank_cap = nranks;
  }
  // the rank bitmap cleans itself after every use; start from a clean one when (re)allocated
  if (nranks != cur_nranks) {
    HIPCHK(hipMemsetAsync(abitmap, 0, (size_t)awords_cap * 4, stream));
    HIPCHK(hipMemsetAsync(asummary, 0, (size_t)asum_words * 4, stream));
    cur_nranks = nranks;
  }
  return upload_record();
}

// A failed host-image call: whatever happened, nothing stays queued that reads a half-prepared slot or the caller's
// buffers.
int ratsdf_engine::host_image_fail(int status) {
  (void)ring.drain();
  abandon_pipeline();
  return status;
}

constexpr size_t kHostChunk = (size_t)32 << 20;  // bytes of h_out that a result of any size passes through

// The staging pair of the host-result entry points: d_out holds at least `dev_bytes` and h_out at least `host_bytes`
// afterwards.  Such an entry point returns only after its result has been copied out and the stream has drained, and
// the entry points of a handle are serialised, so one pair serves them all; what an earlier call left in it is dead.
// Grow-only, each side on its own; the stream is drained before a side is replaced (what it has queued may still use
// the old one), and a side that failed to grow is empty (hip_mem.h).
int ratsdf_engine::staging(size_t dev_bytes, size_t host_bytes) {
  if (dev_bytes > d_out.size()) {
    HIPCHK(hipStreamSynchronize(stream));
    STCHK(d_out.alloc(dev_bytes));
  }
  if (host_bytes > h_out.size()) {
    HIPCHK(hipStreamSynchronize(stream));
    STCHK(h_out.alloc(host_bytes));
  }
  return RATSDF_OK;
}

// `bytes` of device memory into the caller's pageable `dst`, after everything enqueued so far: through h_out, in
// pieces of what it holds (staging() in front sizes it; kHostChunk is enough for any result), each piece waited for
// before it is copied on -- not straight into pageable memory, which is the runtime's staging path (read_small).
// Returns with the stream drained; after a HIP error nothing further has been copied.
int ratsdf_engine::download(void* dst, const void* d_src, size_t bytes) {
  const size_t step = h_out.size();
  if (bytes && !step) return RATSDF_ERR_DEVICE;
  for (size_t o = 0; o < bytes; o += step) {
    const size_t m = std::min(step, bytes - o);
    HIPCHK(hipMemcpyAsync(h_out.as<void>(), (const uint8_t*)d_src + o, m, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    memcpy((uint8_t*)dst + o, h_out.as<void>(), m);
  }
  if (!bytes) HIPCHK(hipStreamSynchronize(stream));
  return RATSDF_OK;
}

// The workspace of a box read-out for n items, carved into *w.  Grow-only: the stream is drained before the buffer is
// replaced (an earlier call may still be using the old one), and the layout is that of the number of items the buffer
// was allocated for, not of this call's n.
template <class Work>
int ratsdf_engine::workspace(Workspace& ws, size_t n, void (*layout)(WsCursor&, size_t, Work*), Work* w) {
  if (ws.cap < n) {
    HIPCHK(hipStreamSynchronize(stream));
    ws.cap = 0;
    STCHK(ws.mem.alloc(ws_bytes(layout, n)));
    ws.cap = n;
  }
  WsCursor c{ws.mem.as<uint8_t>()};
  layout(c, ws.cap, w);
  return RATSDF_OK;
}

CarveBufs ratsdf_engine::carve_bufs(unsigned par) const {
  CarveBufs cb;
  cb.del = del_list[par & 1u];
  cb.del_cap = (uint32_t)tab.num_block;
  cb.slow = slowdel[par & 1u];
  cb.slow_cap = kSlowDelCap;
  cb.upd_wg = upd_wg[par & 1u];
  cb.bitmap = dbitmap;
  cb.summary = dsummary;
  cb.prefix = dprefix;
  return cb;
}

// rank kernel (resolve + mark + scan) on a rank space of `nranks`; the commit itself happens inside
// k_integrate for frames and in commit_pass's k_commit_only otherwise
int ratsdf_engine::alloc_rank(uint32_t nranks, unsigned par, const CandJob* next, bool frame) {
  CandJob none;
  memset(&none, 0, sizeof(none));
  const CandJob& job = next ? *next : none;
  const unsigned extra = job.n_tiles ? (job.n_tiles + job.tiles_per_wg - 1) / job.tiles_per_wg : 0;
  const RankBufs rb = rank_bufs(nranks);
  hipLaunchKernelGGL(k_alloc_rank, dim3(1 + extra), dim3(1024),
                     serial_lds, stream, tab, pool, rb, carve_bufs(par ^ 1u), ctl,
                     (uint32_t)par, d_stats, frame ? cand[par].count : (uint32_t*)nullptr, job);
  HIPCHK(hipGetLastError());
  return RATSDF_OK;
}

// An allocation pass of its own, outside a frame, over the request list a kernel has just filled in the counters of
// parity `par`: the rank kernel, the commits, and k_settle -- no deletes in such a pass, it just zeroes the counters
// again.  After a refused rank launch nothing further is launched.
int ratsdf_engine::commit_pass(uint32_t nranks, unsigned par) {
  STCHK(alloc_rank(nranks, par));
  hipLaunchKernelGGL(k_commit_only, dim3(256), dim3(256), 0, stream, tab, pool, req, req_cap, req_k, win_ranks, ctl,
                     (uint32_t)par);
  hipLaunchKernelGGL(k_settle, dim3(1), dim3(1024), 0, stream, tab, pool, carve_bufs(par), ctl, (uint32_t)par,
                     (ratsdf_frame_stats*)nullptr);
  return RATSDF_OK;
}

// After a failed launch or copy in the middle of a batch: nothing may stay queued that reads the
// caller's buffers, and the look-ahead state must not leak into the next call (a frame that skipped
// k_cand because "its candidate pass already ran" would consume the stale lists of a frame that
// never came).  A group, whose launches were queued on its own stream on behalf of members that do not know about
// them, says how many frames it launched (the last of them owes its carve tail) and has the next candidate counters
// cleared whatever cand_ready says: its look-ahead passes are not in the members' books.
void ratsdf_engine::abandon_pipeline(int frames_launched, bool clear_next) {
  if (stream) (void)hipStreamSynchronize(stream);
  if (frames_launched > 0) {
    parity = (parity + (unsigned)frames_launched) & 1u;
    pending = true;
  }
  if ((cand_ready || clear_next) && cand[parity].count)  // lists filled for a frame that will not be integrated
    (void)hipMemsetAsync(cand[parity].count, 0, (size_t)kCandSegs * kCandCountStride * 4, stream);
  cand_ready = false;
  (void)settle();
  if (stream) (void)hipStreamSynchronize(stream);
}

// Everything but a following frame needs the last frame's carve pass completed first.
int ratsdf_engine::settle() {
  if (!pending) return RATSDF_OK;
  hipLaunchKernelGGL(k_settle, dim3(1), dim3(1024), 0, stream, tab, pool, carve_bufs(parity ^ 1u), ctl,
                     (uint32_t)(parity ^ 1u), d_stats);
  HIPCHK(hipGetLastError());
  pending = false;
  return RATSDF_OK;
}

// ordered compaction of the directory into `vis`; the count lands in *count_slot (device)
int ratsdf_engine::select(int mode, const GridBounds& gb, uint32_t* count_slot) {
  FrameParams P = base_params();
  if (mode == kSelValid)
    hipLaunchKernelGGL(k_select_flags<kSelValid>, dim3(nwg), dim3(kVisWG), 0, stream, tab, P, gb,
                       masks, wg_count);
  else if (mode == kSelOwned)
    hipLaunchKernelGGL(k_select_flags<kSelOwned>, dim3(nwg), dim3(kVisWG), 0, stream, tab, P, gb,
                       masks, wg_count);
  else if (mode == kSelStored)
    hipLaunchKernelGGL(k_select_flags<kSelStored>, dim3(nwg), dim3(kVisWG), 0, stream, tab, P, gb,
                       masks, wg_count);
  else
    hipLaunchKernelGGL(k_select_flags<kSelBounds>, dim3(nwg), dim3(kVisWG), 0, stream, tab, P, gb,
                       masks, wg_count);
  hipLaunchKernelGGL(k_select_scatter, dim3(nwg), dim3(kVisWG), 0, stream, tab, masks, wg_count, vis,
                     vis_cap, count_slot);
  HIPCHK(hipGetLastError());
  return RATSDF_OK;
}

FrameParams ratsdf_engine::frame_params(const FrameIn& in, int H, int W, float md) const {
  FrameParams P = base_params();
  const ratsdf_pose* T = in.T;
  const ratsdf_intrinsics* K = in.K;
  P.T = Se3{Quat{T->qx, T->qy, T->qz, T->qw}, V3{T->tx, T->ty, T->tz}};
  P.Ti = se3_inverse(P.T);                       // voxel_tsdf.cu:459
  P.K = Intr{K->fx, K->fy, K->cx, K->cy};
  P.Ki = intr_inverse(P.K);                      // camera.cuh:67
  P.md = md;
  P.W = W;
  P.H = H;
  P.S = S;
  P.has_sem = (in.ht && in.lt) ? 1 : 0;
  if (P.has_sem) ever_sem = true;  // (frames are prepared in the order they are integrated)
  P.segm_live = ever_sem ? 1 : 0;
  return P;
}

// the frame's row of a job table (kernels_frame.h); `par`: the counter-set parity the frame will run with
void ratsdf_engine::fill_job(FrameJob& j, const FrameIn& in, int H, int W, float md, unsigned par) const {
  j.P = frame_params(in, H, W, md);
  j.depth = (const float*)in.depth;
  j.rgb = (const uint8_t*)in.rgb;
  j.ht = (const float*)in.ht;
  j.lt = (const float*)in.lt;
  j.par = par & 1u;
  j.pad = 0;
}

CandJob ratsdf_engine::cand_job(const FrameIn& in, const FrameParams& P, unsigned par) const {
  CandJob j;
  memset(&j, 0, sizeof(j));
  j.P = P;
  j.depth = (const float*)in.depth;
  j.rgb = (const uint8_t*)in.rgb;
  j.ht = (const float*)in.ht;
  j.lt = (const float*)in.lt;
  j.texA = texA[par];
  j.texB = texB[par];
  j.set = cand[par];
  j.tiles_x = (uint32_t)((P.W + 15) / 16);
  j.tiles_x_magic = cand_tiles_magic(j.tiles_x);
  j.first_tile = 0;
  j.n_tiles = j.tiles_x * (uint32_t)((P.H + 15) / 16) * 4u;
  j.tiles_per_wg = 4;
  return j;
}

// Launch geometry of a frame: workgroup counts and the split of the NEXT frame's candidate pass over
// this frame's three launches (percent in k_front and in k_alloc_rank; the rest rides in k_integrate).
// `b_launched`: the frame has a k_alloc_rank launch -- a share without a launch gets no tiles.
ratsdf_engine::Geom ratsdf_engine::geometry(int H, int W, bool has_next, int split_a, int split_b,
                                            bool b_launched) const {
  Geom g;
  memset(&g, 0, sizeof(g));
  const size_t npix = (size_t)H * W;
  const uint32_t tiles_x = (uint32_t)((W + 15) / 16);
  const uint32_t tiles = tiles_x * (uint32_t)((H + 15) / 16) * 4u;
  g.n_cand_wg = (tiles + 3) / 4;
  g.a.tiles_x = g.b.tiles_x = g.c.tiles_x = tiles_x;
  g.a.tiles_x_magic = g.b.tiles_x_magic = g.c.tiles_x_magic = cand_tiles_magic(tiles_x);
  g.a.tiles_per_wg = g.b.tiles_per_wg = g.c.tiles_per_wg = 4;
  if (has_next) {
    // (the arithmetic and what the kernels rely on: cand_shares.h)
    const CandShares sh = cand_shares(H, W, split_a, split_b, cand_wgs, b_launched);
    auto set = [](AheadGeom& ag, const CandShare& s) {
      ag.first_tile = s.first_tile;
      ag.n_tiles = s.n_tiles;
      ag.tiles_per_wg = s.tiles_per_wg;
    };
    set(g.a, sh.a);
    set(g.b, sh.b);
    set(g.c, sh.c);
  }
  // visible-list workgroups: one lane per pool slot, from the top of the pool down (kernels_visible.h); 128 of them
  // cover a map of 65 536 blocks in one round of two loads per lane, larger maps take more rounds
  g.n_vis_wg = std::min<unsigned>(128u, std::max<unsigned>(1u, ((unsigned)tab.num_block + 2 * 256 - 1) / (2 * 256)));
  // consumer workgroups per candidate list: every 16x16 super-tile reserves kCandReserve entries
  // (one pass of 256 lanes per consumer when nothing overflows); finer voxels need more
  const unsigned supers = ((unsigned)W + 15) / 16 * (((unsigned)H + 15) / 16);
  unsigned parts = (supers * kCandReserve / kCandSegs + 255) / 256;
  if (vs < 0.004f) parts *= 2;
  parts = std::min(std::max(parts, 1u), 32u);
  if (cand_parts_env) parts = cand_parts_env;
  g.parts = parts;
  g.n_front_wg = g.n_vis_wg + kCandSegs * parts + kReleaseWGs + (g.a.n_tiles + 3) / 4;
  // more workgroups for images with several times more visible blocks than 640x480 (1280x720 / 2 mm: 13 k - 22 k
  // visible blocks).  Round 2 measured 16 384 as best (profiles/r02_grid_sweep.txt); with round 4's kernels 8 192
  // is: 60.3 vs 62.4 us per frame on the 20-frame ping-pong (6 144: 61.9, 12 288: 61.5), 11 316 vs 10 838
  // frames/s on the 416 MB map -- a workgroup takes 1.5 - 2.6 blocks, fewer workgroups to dispatch
  g.grid = grid_from_env ? integrate_grid : (npix >= 600000 ? (unsigned)RATSDF_GRID_HD : (unsigned)RATSDF_GRID_VGA);
  return g;
}

// Where the NEXT frame's candidate pass rides, percent in k_front (interleaved A/B, profiles/r02_split_ab.txt): at
// 640x480 10 % in k_front (20 % until round 5) and the rest at the head of k_integrate's grid (10-30 % measured the same,
// 0 and 40 % are ~2.5 % slower: k_front is a chain of dependent round trips that a few riders do not
// lengthen, the voxel update hides the rest); at 1280x720 all of it in k_front (best by 1-3 %, and
// k_integrate stays the pure voxel update its roofline figure is about)
// (k_integrate<1> runs 512-thread workgroups and hosts no look-ahead: everything in k_front then)
int ratsdf_engine::lookahead_split(size_t npix) const {
  if (vpl == 1) return 100;
  return (int)(!cand_split_env && npix >= 600000 ? (unsigned)RATSDF_CAND_SPLIT_HD : cand_split);
}

// May an n-frame batch at H x W replay a captured graph (batch_graph)?  Not for the 512-thread voxel-per-lane
// variant, not with the serial role as a launch of its own, not when a look-ahead pass is already out.
bool ratsdf_engine::graph_eligible(int n, int H, int W) const {
  return use_graphs && n >= 2 && !cand_ready && fused_serial && vpl != 1 && (size_t)H * W * (size_t)S < 0xFFFFFFFFull;
}

// One frame.  `next` (same image size) is the frame the caller will integrate right after this one,
// if it already knows it: its candidate pass then rides in this frame's single-workgroup kernels.
int ratsdf_engine::frame(const FrameIn& cur, const FrameIn* next, int H, int W, float md) {
  const size_t npix = (size_t)H * W;
  if (npix * (size_t)S >= 0xFFFFFFFFull) return RATSDF_ERR_BAD_ARGUMENT;
  int st = ensure_image(npix, npix * (size_t)S);
  if (st != RATSDF_OK) return st;
  const FrameParams P = frame_params(cur, H, W, md);
  const unsigned par = parity;

  // nobody looked ahead (a single frame, the first of a batch): this frame's candidate pass rides in k_front, every
  // pixel workgroup its own consumer (k_front_inline)
  const bool inline_cand = !cand_ready;
#ifdef RATSDF_STAMPS
  const bool inline_kernel = inline_cand && !tab.tail_on && !inline_off;  // (RATSDF_INLINE_CAND=0: k_cand + k_front, for A/B)
  if (inline_cand && !inline_kernel) {
    const CandJob job = cand_job(cur, P, par);
    hipLaunchKernelGGL(k_cand, dim3((job.n_tiles + 3) / 4), dim3(256), 0, stream, job, ctl);
  }
#else
  const bool inline_kernel = inline_cand;
#endif
  const bool fused = fused_serial && vpl != 1;
  const int split_b = fused ? 0 : (int)(cand_split_env ? cand_split_b : 0u);
  const Geom g = geometry(H, W, next != nullptr, lookahead_split(npix), split_b, !fused);
  // shares of the next frame's candidate pass: k_front, k_alloc_rank, k_integrate
  CandJob ahead_a, ahead_b, ahead_c;
  memset(&ahead_a, 0, sizeof(ahead_a));
  memset(&ahead_b, 0, sizeof(ahead_b));
  memset(&ahead_c, 0, sizeof(ahead_c));
  if (next) {
    const FrameParams Pn = frame_params(*next, H, W, md);
    ahead_a = cand_job(*next, Pn, par ^ 1u);
    ahead_b = ahead_a;
    ahead_c = ahead_a;
    auto set = [](CandJob& j, const AheadGeom& ag) {
      j.first_tile = ag.first_tile;
      j.n_tiles = ag.n_tiles;
      j.tiles_per_wg = ag.tiles_per_wg;
    };
    set(ahead_a, g.a);
    set(ahead_b, g.b);
    set(ahead_c, g.c);
  }
  parity = par ^ 1u;
  cand_ready = next != nullptr;

  // fr[par] was zeroed when the frame before last was finalised (or at creation)
  if (inline_kernel) {
    const CandJob now = cand_job(cur, P, par);
    const unsigned n_now_wg = (now.n_tiles + 3) / 4;
    hipLaunchKernelGGL(k_front_inline, dim3(g.n_vis_wg + n_now_wg + kReleaseWGs + (g.a.n_tiles + 3) / 4), dim3(256), 0,
                       stream, tab, (uint32_t)g.n_vis_wg, (uint32_t)n_now_wg, req, req_cap, slow, kSlowCap,
                       vis + kFreshCap, seg_cap, pool, carve_bufs(par ^ 1u), ctl, (uint32_t)par, now, ahead_a);
  } else
#ifdef RATSDF_STAMPS
  if (tab.tail_on)
    hipLaunchKernelGGL(k_front<true>, dim3(g.n_front_wg), dim3(256), 0, stream, tab, P, g.n_vis_wg, cand[par],
                       (uint32_t)g.parts, req, req_cap, slow, kSlowCap, vis + kFreshCap, seg_cap, pool,
                       carve_bufs(par ^ 1u), ctl, (uint32_t)par, d_stats, 1u | front_prio, ahead_a);
  else
#endif
    hipLaunchKernelGGL(k_front<false>, dim3(g.n_front_wg), dim3(256), 0, stream, tab, P, g.n_vis_wg, cand[par],
                       (uint32_t)g.parts, req, req_cap, slow, kSlowCap, vis + kFreshCap, seg_cap, pool,
                       carve_bufs(par ^ 1u), ctl, (uint32_t)par, d_stats, 0u, ahead_a);
#ifdef RATSDF_STAMPS
  // (experiment, RATSDF_SORT_LISTS=1: every work list put into image-tile order on the HOST between the two launches --
  // an upper bound for what tile-ordered lists would buy the update; the engine waits for k_front here, so only the
  // update's own time means anything in such a run)
  if (sort_lists) {
    HIPCHK(hipStreamSynchronize(stream));
    std::vector<uint32_t> fc(sizeof(FrameCtl) / 4);
    HIPCHK(hipMemcpy(fc.data(), &ctl->fr[par], sizeof(FrameCtl), hipMemcpyDeviceToHost));
    const FrameCtl* hf = reinterpret_cast<const FrameCtl*>(fc.data());
    const double qx = P.T.q.x, qy = P.T.q.y, qz = P.T.q.z, qw = P.T.q.w;
    for (int l = 0; l < kNumLists; ++l) {
      uint32_t n = hf->n_list[l * kListStride];
      if (n > seg_cap - kFreshCap) n = seg_cap - kFreshCap;
      if (n < 2) continue;
      std::vector<VisItem> items(n);
      VisItem* dl = vis + kFreshCap + (size_t)l * seg_cap;
      HIPCHK(hipMemcpy(items.data(), dl, (size_t)n * sizeof(VisItem), hipMemcpyDeviceToHost));
      auto key = [&](const VisItem& it) {
        const double x = (it.x * 8 + 4) * (double)P.vs, y = (it.y * 8 + 4) * (double)P.vs, z = (it.z * 8 + 4) * (double)P.vs;
        // rotate by the quaternion, translate, project
        const double ux = 2 * (qy * z - qz * y), uy = 2 * (qz * x - qx * z), uz = 2 * (qx * y - qy * x);
        const double cx = x + qw * ux + (qy * uz - qz * uy) + P.T.t.x, cy = y + qw * uy + (qz * ux - qx * uz) + P.T.t.y,
                     cz = z + qw * uz + (qx * uy - qy * ux) + P.T.t.z;
        double u = (P.K.fx * cx + P.K.cx * cz) / cz, v = (P.K.fy * cy + P.K.cy * cz) / cz;
        u = std::min(std::max(u, 0.0), (double)(P.W - 1));
        v = std::min(std::max(v, 0.0), (double)(P.H - 1));
        // finer than the 8x8 tiles: 32x32 cells in raster order of cells
        return (int)(v * 32.0 / P.H) * 32 + (int)(u * 32.0 / P.W);
      };
      std::stable_sort(items.begin(), items.end(), [&](const VisItem& a, const VisItem& b) { return key(a) < key(b); });
      HIPCHK(hipMemcpy(dl, items.data(), (size_t)n * sizeof(VisItem), hipMemcpyHostToDevice));
    }
  }
  if (!fused) {  // (the serial role as a launch of its own: the round-1 layout, kept for A/B in the diagnostic build)
    st = alloc_rank((uint32_t)(npix * (size_t)S), par, next ? &ahead_b : nullptr, true);
    if (st != RATSDF_OK) return st;
  }
#endif

  if (timer.on) STCHK(timer.reserve(1));
  const auto [ev0, ev1] = timer.take();
  const unsigned integrate_grid = g.grid;
  // hipExtLaunchKernelGGL attaches the two events to the dispatch itself: their difference is the
  // kernel's own start-to-end time (what rocprofv3 reports), without the barrier packets that
  // hipEventRecord before / after a launch would add (~3 us here).  Null events = a plain launch.
  const unsigned extra_c = ((ahead_c.n_tiles + 3) / 4 + 7u) & ~7u;  // whole groups of 8 (XCD mapping)
  const uint32_t n_serial_wg = fused ? 8u : 0u;  // the first of them works
  const uint32_t commit_rot = fused ? commit_rotation(integrate_grid, integrate_grid) : 0u;
  IntegArgs ia;
  ia.rgbw = pool.rgbw;
  ia.tsdf = pool.tsdf;
  ia.segm = pool.segm;
  ia.texA = texA[par];
  ia.texB = texB[par];
  ia.vis = vis + kFreshCap;
  ia.seg_cap = seg_cap;
  ia.F = &ctl->fr[par];
  ia.upd_wg = upd_wg[par];
  ia.par = par;
#define RATSDF_LAUNCH_INTEGRATE(V, T, NT)                                                              \
  hipExtLaunchKernelGGL((k_integrate<V, T>), dim3(integrate_grid + n_serial_wg + extra_c), dim3(NT), 0, \
                        stream, ev0, ev1, 0, ia, P, (EnginePtr)d_eng, (uint32_t)integrate_grid,         \
                        n_serial_wg, (uint32_t)extra_c, commit_rot, ahead_c)
  // (the voxels-per-lane variants 1 / 4 / 8 are tuning options: without the front-tail path)
#ifdef RATSDF_STAMPS
  switch (vpl) {
    case 1: RATSDF_LAUNCH_INTEGRATE(1, false, 512); break;
    case 8: RATSDF_LAUNCH_INTEGRATE(8, false, RATSDF_INTEG_NT); break;
    case 4: RATSDF_LAUNCH_INTEGRATE(4, false, RATSDF_INTEG_NT); break;
    default:
      if (tab.tail_on) RATSDF_LAUNCH_INTEGRATE(2, true, RATSDF_INTEG_NT);
      else RATSDF_LAUNCH_INTEGRATE(2, false, RATSDF_INTEG_NT);
  }
#else
  RATSDF_LAUNCH_INTEGRATE(2, false, RATSDF_INTEG_NT);  // the one form the product ships
#endif
#undef RATSDF_LAUNCH_INTEGRATE

  HIPCHK(hipGetLastError());
  pending = true;
  if (timer.full()) return timer.drain(stream, false);
  return RATSDF_OK;
}

// The sticky error word, after everything enqueued so far.  No device-to-host copy in the ordinary call: set_error
// (kernels_alloc.h) also raises a flag in page-locked host memory (h_err[0], through Ctl::err_flag), which is read
// once the stream has drained; only when it is set is the device word -- the FIRST error -- fetched (into h_err[1]:
// page-locked as well; a copy into pageable memory goes through the runtime's staging path).  A synchronising call on
// an idle engine went from 20 - 25 us to a stream synchronisation; the per-frame convention of TSDFGrid::Integrate
// (ratsdf_integrate_device + ratsdf_synchronize) from 59 - 61 us per frame to the figure in profiles/r05_sync_path.txt.
int ratsdf_engine::sticky() {
  HIPCHK(hipStreamSynchronize(stream));
  if (*(volatile uint32_t*)h_err == 0u) return RATSDF_OK;
  HIPCHK(hipMemcpyAsync(h_err + 1, &ctl->error, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  return (int)((volatile uint32_t*)h_err)[1];
}

// A few words of device memory for the host, after everything enqueued so far: through the page-locked landing buffer
// (h_err + 16 words on), not straight into the caller's pageable memory (the runtime's staging path: ~20 us per call,
// and these are the calls a per-frame logger makes -- NumActiveBlock, the frame statistics).
int ratsdf_engine::read_small(void* dst, const void* dev_src, size_t bytes) {
  if (bytes > 384) return RATSDF_ERR_BAD_ARGUMENT;
  HIPCHK(hipMemcpyAsync(h_err + 16, dev_src, bytes, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  memcpy(dst, h_err + 16, bytes);
  return RATSDF_OK;
}

// Non-finite camera parameters are refused at the boundary (RATSDF_ERR_BAD_ARGUMENT).  The reference
// would integrate garbage (a NaN pose projects every voxel to pixel (0, 0): float -> int of NaN is 0 in
// CUDA); the engine's short pixel pick (kernels_integrate.h) reproduces the reference for
// every finite pose -- including voxels in the camera plane, z == 0 -- and relies on this check for the
// rest.
static bool finite_frame(const ratsdf_intrinsics& K, const ratsdf_pose& T, float max_depth) {
  const float v[] = {K.fx, K.fy, K.cx, K.cy, T.qx, T.qy, T.qz, T.qw, T.tx, T.ty, T.tz, max_depth};
  for (float x : v)
    if (!std::isfinite(x)) return false;
  return true;
}

// The launches of a batch whose operands lie in device tables: n frames of S members each (blockIdx.y), engine
// records in `engs`, frame f of member s in d_jobs[f * S + s].  k_cand_g for the first frame (nobody looked ahead
// for it: its candidate pass runs in line), then per frame k_front_g, k_alloc_rank_g when the serial role is a launch
// of its own (n_serial_wg == 0, diagnostic build) and k_integrate_g; `g1` is the geometry of a frame that hosts the
// next one's look-ahead pass, `g0` of the last.  With a `timer` the k_integrate_g launches are direct ones that carry
// its events (hipExtLaunchKernelGGL attaches them to the dispatch itself, see frame()); without, plain launches: what
// a stream capture records.  Returns the frames enqueued completely and the status: after a refused launch the
// caller has that many frames queued on behalf of its engines.
struct Enqueued {
  int frames, status;
};
static Enqueued enqueue_jobs(hipStream_t stream, EnginePtr engs, const FrameJob* d_jobs, int n, int S,
                             const ratsdf_engine::Geom& g0, const ratsdf_engine::Geom& g1, uint32_t commit_rot,
                             uint32_t n_serial_wg, [[maybe_unused]] uint32_t tail, [[maybe_unused]] int vpl,
                             KernelTimer* timer) {
  {
    AheadGeom all = g0.a;
    all.first_tile = 0;
    all.n_tiles = g0.n_cand_wg * 4;
    hipLaunchKernelGGL(k_cand_g, dim3(g0.n_cand_wg, S), dim3(256), 0, stream, engs, (JobPtr)d_jobs, all);
  }
  if (hipGetLastError() != hipSuccess) return {0, RATSDF_ERR_DEVICE};
  for (int f = 0; f < n; ++f) {
    const bool has_next = f + 1 < n;
    const ratsdf_engine::Geom& gg = has_next ? g1 : g0;
    JobPtr cur = (JobPtr)(d_jobs + (size_t)f * S);
    JobPtr nxt = (JobPtr)(d_jobs + (size_t)(has_next ? f + 1 : f) * S);
#ifdef RATSDF_STAMPS
    if (tail & 1u)
      hipLaunchKernelGGL(k_front_g<true>, dim3(gg.n_front_wg, S), dim3(256), 0, stream, engs, cur, nxt,
                         (uint32_t)gg.n_vis_wg, (uint32_t)gg.parts, tail, gg.a);
    else
#endif
      hipLaunchKernelGGL(k_front_g<false>, dim3(gg.n_front_wg, S), dim3(256), 0, stream, engs, cur, nxt,
                         (uint32_t)gg.n_vis_wg, (uint32_t)gg.parts, 0u, gg.a);
#ifdef RATSDF_STAMPS
    if (!n_serial_wg) {
      const unsigned extra_b = gg.b.n_tiles ? (gg.b.n_tiles + gg.b.tiles_per_wg - 1) / gg.b.tiles_per_wg : 0;
      hipLaunchKernelGGL(k_alloc_rank_g, dim3(1 + extra_b, S), dim3(1024), kSerialLdsBytes, stream, engs, cur, nxt,
                         gg.b);
    }
#endif
    const unsigned extra_c = ((gg.c.n_tiles + 3) / 4 + 7u) & ~7u;  // whole groups of 8 (XCD mapping)
    const dim3 grid(gg.grid + n_serial_wg + extra_c, S);
    std::pair<hipEvent_t, hipEvent_t> ev{nullptr, nullptr};
    if (timer) ev = timer->take();
#define RATSDF_LAUNCH_INTEGRATE_G(V, T, NT)                                                                    \
  do {                                                                                                         \
    const auto kernel = k_integrate_g<V, T>;                                                                   \
    if (timer)                                                                                                 \
      hipExtLaunchKernelGGL(kernel, grid, dim3(NT), 0, stream, ev.first, ev.second, 0, engs, cur, nxt,         \
                            (uint32_t)gg.grid, n_serial_wg, (uint32_t)extra_c, commit_rot, gg.c);              \
    else                                                                                                       \
      hipLaunchKernelGGL(kernel, grid, dim3(NT), 0, stream, engs, cur, nxt, (uint32_t)gg.grid, n_serial_wg,    \
                         (uint32_t)extra_c, commit_rot, gg.c);                                                 \
  } while (0)
    // (the voxels-per-lane variants 1 / 4 / 8 are tuning options: without the front-tail path)
#ifdef RATSDF_STAMPS
    switch (vpl) {
      case 1: RATSDF_LAUNCH_INTEGRATE_G(1, false, 512); break;
      case 8: RATSDF_LAUNCH_INTEGRATE_G(8, false, RATSDF_INTEG_NT); break;
      case 4: RATSDF_LAUNCH_INTEGRATE_G(4, false, RATSDF_INTEG_NT); break;
      default:
        if (tail & 1u) RATSDF_LAUNCH_INTEGRATE_G(2, true, RATSDF_INTEG_NT);
        else RATSDF_LAUNCH_INTEGRATE_G(2, false, RATSDF_INTEG_NT);
    }
#else
    RATSDF_LAUNCH_INTEGRATE_G(2, false, RATSDF_INTEG_NT);  // the one form the product ships
#endif
#undef RATSDF_LAUNCH_INTEGRATE_G
    if (hipGetLastError() != hipSuccess) return {f, RATSDF_ERR_DEVICE};  // a launch of this frame was refused
    if (timer && timer->full()) {
      const int st = timer->drain(stream);
      if (st != RATSDF_OK) return {f + 1, st};
    }
  }
  return {n, RATSDF_OK};
}

// The graph of an n-frame batch at H x W (built on first use, a few kept): the launches of enqueue_jobs with the
// look-ahead shares frame() would choose, one member (blockIdx.y = 0), operands from d_eng and the graph's own job
// table.
int ratsdf_engine::batch_graph(int n, int H, int W, BatchGraph** out) {
  *out = nullptr;
  for (auto& g : graphs)
    if (g.H == H && g.W == W && g.n == n) {
      g.last_use = ++graph_clock;
      *out = &g;
      return RATSDF_OK;
    }
  for (const auto& f : graph_failed)
    if (f.H == H && f.W == W && f.n == n) return RATSDF_ERR_DEVICE;  // (reported when it happened)
  // A graph per batch LENGTH: a caller that drains a queue (ratsdf::TSDFSystem hands over 1 .. 32 frames) meets
  // every length sooner or later, so the cache holds all of them for a couple of image sizes before anything is
  // evicted (a graph is ~0.2 KiB of job table per frame plus the executable graph).
  if (graphs.size() >= 72) {  // least recently used out
    size_t victim = 0;
    for (size_t i = 1; i < graphs.size(); ++i)
      if (graphs[i].last_use < graphs[victim].last_use) victim = i;
    HIPCHK(hipStreamSynchronize(stream));  // (nothing queued replays the graph that goes)
    graphs.erase(graphs.begin() + (long)victim);
  }
  BatchGraph g;
  g.H = H;
  g.W = W;
  g.n = n;
  auto fail = [&](const char* what) {
    fprintf(stderr, "[ratsdf] batch graph %dx%d x %d: %s failed; batches of this shape are launched frame by frame\n",
            W, H, n, what);
    graph_failed.push_back(GraphShape{H, W, n});
    return RATSDF_ERR_DEVICE;
  };
  if (g.d_jobs.alloc((size_t)n * sizeof(FrameJob)) != RATSDF_OK) return fail("hipMalloc");
  FrameJob* const d_jobs = g.d_jobs.as<FrameJob>();
  if (g.jobs.grow((size_t)n * sizeof(FrameJob)) != RATSDF_OK) return fail("staging allocation");
  // (graph_eligible: the serial role rides in k_integrate_g, whose first 8 extra workgroups are its own)
  const Geom g1 = geometry(H, W, true, lookahead_split((size_t)H * W), 0, false);
  const Geom g0 = geometry(H, W, false, 0, 0, false);
  if (hipStreamBeginCapture(stream, hipStreamCaptureModeRelaxed) != hipSuccess) return fail("hipStreamBeginCapture");
  const Enqueued q = enqueue_jobs(stream, (EnginePtr)d_eng, d_jobs, n, 1, g0, g1, commit_rotation(g0.grid, g0.grid), 8u,
                                  (tab.tail_on ? 1u : 0u) | front_prio, vpl, nullptr);
  if (g.graph.end_capture(stream) != RATSDF_OK || q.status != RATSDF_OK) return fail("capture");
  if (g.graph.instantiate() != RATSDF_OK) return fail("hipGraphInstantiate");
  g.last_use = ++graph_clock;
  graphs.push_back(std::move(g));
  *out = &graphs.back();
  return RATSDF_OK;
}

// a sticky error some finished launch has already raised, without waiting for the stream (ratsdf_engine::sticky): the
// check of the asynchronous entry points of sample.inc, esdf.inc and surface.inc
static int sticky_raised(ratsdf_engine* e) {
  return *(volatile uint32_t*)e->h_err != 0u ? e->sticky() : RATSDF_OK;
}

// ... behind the settled carve pass: what every entry point of a box read-out does after ENTRY
static int box_entry(ratsdf_engine* e) {
  STCHK(e->settle());
  return sticky_raised(e);
}

// The exclusive scan of kernels_mesh.h, queued on the engine's stream: pos[i] = cnt[0] + .. + cnt[i - 1] and *d_total
// their sum, for n counts (device arrays); `tiles` holds scan_tiles(n) words and is dead afterwards.  pos == cnt scans
// in place (a thread of k_mask_positions reads its four counts before it writes their positions).  Does not wait.
static int scan_counts(ratsdf_engine* e, const uint32_t* cnt, size_t n, uint32_t* tiles, uint32_t* d_total,
                       uint32_t* pos) {
  const uint32_t ntiles = (uint32_t)scan_tiles(n);
  hipLaunchKernelGGL(k_mask_tile_sums, dim3(ntiles), dim3(1024), 0, e->stream, cnt, n, tiles);
  hipLaunchKernelGGL(k_scan_tile_sums, dim3(1), dim3(1024), 0, e->stream, tiles, ntiles, d_total);
  hipLaunchKernelGGL(k_mask_positions, dim3(ntiles), dim3(1024), 0, e->stream, cnt, n, tiles, pos);
  HIPCHK(hipGetLastError());
  return RATSDF_OK;
}

// exclusive positions of the set items of a 0/1 mask (device arrays), and in *h_total their number; waits for the stream
// (rebuild_derived's free list, the mesh gather of query.inc)
static int mask_positions(ratsdf_engine* e, const uint32_t* mask, size_t n, uint32_t* pos,
                          uint32_t* scratch_tiles, uint32_t* d_total, uint32_t* h_total) {
  STCHK(scan_counts(e, mask, n, scratch_tiles, d_total, pos));
  HIPCHK(hipMemcpyAsync(h_total, d_total, 4, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return RATSDF_OK;
}

// A counted result leaves through the staging pair into fresh malloc memory, which the caller of the entry point owns:
// up to two parts, laid side by side in d_out in their order, the first at offset 0.
struct HostPart {
  size_t count, record;  // records the count pass found, and the bytes of one
  void** out;            // the entry point's outputs: null and zero unless everything has arrived
  size_t* n_out;
};
// `emit(d)` queues the pass that writes part i at d[i].  Nulls the outputs first; with every count zero that is all
// (the status is sticky()).  An empty part beside a filled one still gets an allocation of its own.  A failed malloc is
// RATSDF_ERR_DEVICE with nothing queued (the caller's read of the counts drained the stream); after any failure every
// part has been freed.
template <class Emit>
static int hand_over(ratsdf_engine* e, const HostPart* parts, int nparts, Emit emit) {
  size_t bytes[2] = {0, 0}, sum = 0;
  for (int i = 0; i < nparts; ++i) {
    *parts[i].out = nullptr, *parts[i].n_out = 0;
    bytes[i] = parts[i].count * parts[i].record;
    sum += bytes[i];
  }
  if (sum == 0) return e->sticky();
  STCHK(e->staging(sum, kHostChunk));
  void* host[2] = {nullptr, nullptr};
  uint8_t* dev[2] = {e->d_out.as<uint8_t>(), e->d_out.as<uint8_t>() + bytes[0]};
  int st = RATSDF_OK;
  for (int i = 0; i < nparts; ++i)
    if (!(host[i] = malloc(bytes[i] ? bytes[i] : 1))) st = RATSDF_ERR_DEVICE;
  if (st == RATSDF_OK) st = emit(dev);
  for (int i = 0; i < nparts && st == RATSDF_OK; ++i) st = e->download(host[i], dev[i], bytes[i]);
  if (st == RATSDF_OK) st = e->sticky();
  for (int i = 0; i < nparts; ++i) {
    if (st != RATSDF_OK)
      free(host[i]);
    else
      *parts[i].out = host[i], *parts[i].n_out = parts[i].count;
  }
  return st;
}

// ================================== C ABI =====================================================
extern "C" {

int ratsdf_create_ex(const ratsdf_config* cfg, ratsdf_engine** out) {
  if (!cfg || !out) return RATSDF_ERR_BAD_ARGUMENT;
  if (!(cfg->voxel_size > 0) || !(cfg->truncation > 0) || !std::isfinite(cfg->voxel_size) ||
      !std::isfinite(cfg->truncation))
    return RATSDF_ERR_BAD_ARGUMENT;
  const int bb = cfg->block_bits ? cfg->block_bits : RATSDF_DEFAULT_BLOCK_BITS;
  const int kb = cfg->bucket_bits ? cfg->bucket_bits : RATSDF_DEFAULT_BUCKET_BITS;
  if (bb < 1 || bb > 24 || kb < 9 || kb > 26) return RATSDF_ERR_BAD_ARGUMENT;
  if (cfg->shard_count > 1 && (cfg->shard_rank < 0 || cfg->shard_rank >= cfg->shard_count))
    return RATSDF_ERR_BAD_ARGUMENT;
  if (cfg->shard_slab_bits > RATSDF_MAX_SHARD_SLAB_BITS) return RATSDF_ERR_BAD_ARGUMENT;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return RATSDF_ERR_NO_DEVICE;
  if (cfg->device < 0 || cfg->device >= ndev) return RATSDF_ERR_BAD_ARGUMENT;
  DeviceGuard guard(cfg->device);  // (not ENTRY: there is no engine yet, the device comes from the configuration)
  if (!guard.ok()) return RATSDF_ERR_DEVICE;
  ratsdf_engine* e = new (std::nothrow) ratsdf_engine();
  if (!e) return RATSDF_ERR_DEVICE;
  e->device = cfg->device;
  e->vs = cfg->voxel_size;
  e->trunc = cfg->truncation;
  e->block_bits = bb;
  e->bucket_bits = kb;
  e->shard_rank = cfg->shard_rank;
  e->shard_count = cfg->shard_count > 1 ? cfg->shard_count : 1;
  e->shard_slab_bits = cfg->shard_slab_bits > 0 ? cfg->shard_slab_bits : 2;
  e->S = (int)ceilf(2.f * e->trunc / e->vs / RATSDF_BLOCK_LEN) + 2;
  // What the environment may change in the shipped library: the three documented behaviours below.  Every tuning and ablation switch of the measurements in
  // DESIGN.md / profiles/ -- voxels per lane, look-ahead split, grid, the serial role as a launch of its own or at
  // the tail of k_front, fault injection -- exists in the diagnostic build only (make stamps, -DRATSDF_STAMPS),
  // together with the kernel variants it selects.
  if (const char* v = getenv("RATSDF_SYNC_INTEGRATE")) e->sync_integrate = atoi(v) != 0;
  if (const char* v = getenv("RATSDF_GRAPH")) e->use_graphs = atoi(v) != 0;
  if (const char* v = getenv("RATSDF_COPY_STREAMS")) e->ring.two_streams = atoi(v) != 1;
#ifdef RATSDF_STAMPS
  if (const char* v = getenv("RATSDF_VPL")) {
    const int x = atoi(v);
    if (x == 1 || x == 2 || x == 4 || x == 8) e->vpl = x;
  }
  if (const char* v = getenv("RATSDF_DEBUG")) e->debug = atoi(v);
  if (const char* v = getenv("RATSDF_CAND_SPLIT")) {  // "a" or "a,b": percent in k_front[, k_alloc_rank]
    const int x = atoi(v);
    if (x >= 0 && x <= 100) {
      e->cand_split = (unsigned)x;
      e->cand_split_b = 100u - (unsigned)x;
      e->cand_split_env = true;
      if (const char* c = strchr(v, ',')) {
        const int y = atoi(c + 1);
        if (y >= 0 && x + y <= 100) e->cand_split_b = (unsigned)y;
      }
    }
  }
  if (const char* v = getenv("RATSDF_CAND_PARTS")) {
    const int x = atoi(v);
    if (x >= 1 && x <= 64) e->cand_parts_env = (unsigned)x;
  }
  if (const char* v = getenv("RATSDF_COMMIT_ROT")) e->commit_rot_env = atoi(v);
  if (const char* v = getenv("RATSDF_FUSED_SERIAL")) e->fused_serial = atoi(v) != 0;  // 0: k_alloc_rank launch
  if (const char* v = getenv("RATSDF_FRONT_TAIL")) e->front_tail = atoi(v) != 0;  // 0: the role always in k_integrate
  if (const char* v = getenv("RATSDF_FRONT_PRIO")) e->front_prio = atoi(v) ? 2u : 0u;
  if (const char* v = getenv("RATSDF_INLINE_CAND")) e->inline_off = atoi(v) == 0;
  if (const char* v = getenv("RATSDF_SORT_LISTS")) e->sort_lists = atoi(v) != 0;
  if (const char* v = getenv("RATSDF_SERIAL_LDS")) {
    const int x = atoi(v);
    if (x >= kSerialLdsBytes && x <= 160 * 1024) e->serial_lds = (unsigned)x;
  }
  if (const char* v = getenv("RATSDF_CAND_WGS")) {
    const int x = atoi(v);
    if (x >= 1 && x <= 4096) e->cand_wgs = (unsigned)x;
  }
  if (const char* v = getenv("RATSDF_GRID")) {
    const int x = atoi(v);
    if (x >= 64 && x <= 65536) {
      e->integrate_grid = (unsigned)x;
      e->grid_from_env = true;
    }
  }
#endif
  Table& t = e->tab;
  t.tail_on = (e->front_tail && e->fused_serial && e->vpl == 2) ? 1u : 0u;
  t.delta_on = 0;
  t.num_block = 1 << bb;
  t.num_bucket = 1u << kb;
  t.num_entry = t.num_bucket << 1;
  t.bucket_mask = t.num_bucket - 1;
  t.entry_mask = t.num_entry - 1;
  const uint32_t occ_words = (t.num_entry + 63) / 64;
  e->nwg = (occ_words + kVisWG - 1) / kVisWG;
  e->dwords = (t.num_entry + 31) / 32;  // delete bitmap is indexed by hash entry
  const size_t nvox = (size_t)t.num_block << 9;

#define CREATE_CHK(expr)                 \
  do {                                   \
    if ((expr) != hipSuccess) {          \
      fprintf(stderr, "[ratsdf] create failed: %s\n", #expr); \
      delete e;                          \
      return RATSDF_ERR_DEVICE;          \
    }                                    \
  } while (0)

  CREATE_CHK(e->stream.create(hipStreamNonBlocking));
  CREATE_CHK(e->own(e->fixed, &t.entries, (size_t)t.num_entry * sizeof(Entry)));
  CREATE_CHK(e->own(e->fixed, &t.claim, (size_t)t.num_bucket * 4));
  // occupancy bitmap, and behind it the dirty bitmap of the directory delta (device_types.h: Table)
  CREATE_CHK(e->own(e->fixed, &t.occ, (size_t)occ_words * 8 * 2));
  CREATE_CHK(hipMemsetAsync(t.occ + occ_words, 0, (size_t)occ_words * 8, e->stream));
  // the live blocks by pool index (device_types.h: Table::active): every slot empty (idx = -1)
  CREATE_CHK(e->own(e->fixed, &t.active, (size_t)t.num_block * sizeof(VisItem)));
  CREATE_CHK(hipMemsetAsync(t.active, 0xFF, (size_t)t.num_block * sizeof(VisItem), e->stream));
  t.del_cap = (uint32_t)t.num_block;
  CREATE_CHK(e->own(e->fixed, &t.del_log, (size_t)t.del_cap * sizeof(uint2)));
  CREATE_CHK(e->own(e->fixed, &t.del_count, 128));
  CREATE_CHK(hipMemsetAsync(t.del_count, 0, 128, e->stream));
  CREATE_CHK(e->own(e->fixed, &e->pool.rgbw, nvox * 4));
  CREATE_CHK(e->own(e->fixed, &e->pool.tsdf, nvox * 4));
  CREATE_CHK(e->own(e->fixed, &e->pool.segm, nvox * 4));
  CREATE_CHK(e->own(e->fixed, &e->pool.heap, (size_t)t.num_block * 4));
  CREATE_CHK(e->own(e->fixed, &e->ctl, sizeof(Ctl)));
  CREATE_CHK(e->own(e->fixed, &e->d_stats, sizeof(ratsdf_frame_stats)));
  CREATE_CHK(e->h_err_page.alloc(512));
  e->h_err = e->h_err_page.as<uint32_t>();
  CREATE_CHK(e->own(e->fixed, &e->d_eng, sizeof(EngineDev)));
  CREATE_CHK(e->own(e->fixed, &e->slow, (size_t)kSlowCap * sizeof(SlowRequest)));
  CREATE_CHK(e->own(e->fixed, &e->xlocks, (size_t)kXLockCap * sizeof(XLock)));
  CREATE_CHK(e->own(e->fixed, &e->sort_scratch, (size_t)kSlowSortCap * sizeof(unsigned long long) +
                                               (size_t)kSlowPlanCap * sizeof(SlowPlan)));  // sort keys | plans
  CREATE_CHK(e->own(e->fixed, &e->serial_scratch, (size_t)kSerialLdsBytes));
  CREATE_CHK(e->own(e->fixed, &e->masks, (size_t)e->nwg * kVisWG * 8));
  CREATE_CHK(e->own(e->fixed, &e->wg_count, (size_t)e->nwg * 4));
  // 8 per-XCD work lists; a segment = kFreshCap items for the list's new blocks (front_tail_role) in front of
  // room for every block of the pool (device_types.h: kFreshCap); queries use the buffer as one flat list
  e->seg_cap = (uint32_t)t.num_block + kFreshCap;
  e->vis_cap = kFreshCap + kNumLists * e->seg_cap;
  CREATE_CHK(e->own(e->fixed, &e->vis, (size_t)e->vis_cap * sizeof(VisItem)));
  for (int i = 0; i < 2; ++i) {
    CREATE_CHK(e->own(e->fixed, &e->del_list[i], (size_t)t.num_block * sizeof(DelItem)));
    CREATE_CHK(e->own(e->fixed, &e->upd_wg[i], kUpdCounters * 4));
    CREATE_CHK(hipMemsetAsync(e->upd_wg[i], 0, kUpdCounters * 4, e->stream));
    CREATE_CHK(e->own(e->fixed, &e->slowdel[i], (size_t)kSlowDelCap * sizeof(SlowDelete)));
  }
  CREATE_CHK(e->own(e->fixed, &e->win_ranks, (size_t)kFusedRank * 4));
  CREATE_CHK(e->own(e->fixed, &t.dclaim, (size_t)t.num_bucket * 4));
  CREATE_CHK(hipMemsetAsync(t.dclaim, 0xFF, (size_t)t.num_bucket * 4, e->stream));
  e->dwords = (e->dwords + kGroupWords - 1) / kGroupWords * kGroupWords;
  const uint32_t dsum_words = (e->dwords / kGroupWords + 31) / 32;
  CREATE_CHK(e->own(e->fixed, &e->dbitmap, (size_t)e->dwords * 4));
  CREATE_CHK(e->own(e->fixed, &e->dsummary, (size_t)dsum_words * 4));
  CREATE_CHK(e->own(e->fixed, &e->dprefix, (size_t)e->dwords * 4));
  CREATE_CHK(e->own(e->fixed, &e->cand_count, 2 * kCandSegs * kCandCountStride * 4));
  CREATE_CHK(hipMemsetAsync(e->cand_count, 0, 2 * kCandSegs * kCandCountStride * 4, e->stream));
  for (int i = 0; i < 2; ++i) e->cand[i].count = e->cand_count + i * kCandSegs * kCandCountStride;
  // voxel memory starts zeroed (defined value for the reference's uninitialised rgb)
  CREATE_CHK(hipMemsetAsync(e->pool.rgbw, 0, nvox * 4, e->stream));
  CREATE_CHK(hipMemsetAsync(e->pool.tsdf, 0, nvox * 4, e->stream));
  CREATE_CHK(hipMemsetAsync(e->pool.segm, 0, nvox * 4, e->stream));
  CREATE_CHK(hipMemsetAsync(e->ctl, 0, sizeof(Ctl), e->stream));
  CREATE_CHK(hipMemsetAsync(e->d_stats, 0, sizeof(ratsdf_frame_stats), e->stream));
  CREATE_CHK(hipMemsetAsync(e->dbitmap, 0, (size_t)e->dwords * 4, e->stream));
  CREATE_CHK(hipMemsetAsync(e->dsummary, 0, (size_t)dsum_words * 4, e->stream));
  hipLaunchKernelGGL(k_init_table, dim3((t.num_entry + 255) / 256), dim3(256), 0, e->stream,
                     t.entries, t.claim, t.occ, t.num_entry, t.num_bucket);
  hipLaunchKernelGGL(k_init_heap, dim3((t.num_block + 255) / 256), dim3(256), 0, e->stream,
                     e->pool.heap, t.num_block);
  const int32_t nf = t.num_block;
  CREATE_CHK(hipMemcpyAsync(&e->ctl->num_free, &nf, 4, hipMemcpyHostToDevice, e->stream));
  CREATE_CHK(hipMemcpyAsync(&e->ctl->free_low, &nf, 4, hipMemcpyHostToDevice, e->stream));
  {  // the error flag's home in page-locked host memory, as the device addresses it (sticky())
    e->h_err[0] = e->h_err[1] = 0u;
    void* flag_dev = nullptr;
    CREATE_CHK(hipHostGetDevicePointer(&flag_dev, e->h_err, 0));
    CREATE_CHK(hipMemcpyAsync(&e->ctl->err_flag, &flag_dev, sizeof(flag_dev), hipMemcpyHostToDevice, e->stream));
  }
  CREATE_CHK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_alloc_rank),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 8 * 1024));
  hipLaunchKernelGGL(k_check_block_threads, dim3(3), dim3(192), 0, e->stream, &e->ctl->n_sel);
  uint32_t bt = 0;
  CREATE_CHK(hipMemcpyAsync(&bt, &e->ctl->n_sel, 4, hipMemcpyDeviceToHost, e->stream));
  CREATE_CHK(hipStreamSynchronize(e->stream));
  CREATE_CHK(hipGetLastError());
  if (bt != 192u) {
    fprintf(stderr, "[ratsdf] create failed: the workgroup size is not where block_threads() reads it (code object ABI?)\n");
    delete e;
    return RATSDF_ERR_DEVICE;
  }
  CREATE_CHK(e->upload_record());
#undef CREATE_CHK
  *out = e;
  return RATSDF_OK;
}

int ratsdf_create(float voxel_size, float truncation, int device, ratsdf_engine** out) {
  ratsdf_config c;
  memset(&c, 0, sizeof(c));
  c.voxel_size = voxel_size;
  c.truncation = truncation;
  c.device = device;
  return ratsdf_create_ex(&c, out);
}

int ratsdf_destroy(ratsdf_engine* e) {
  ENTRY(e, true);
  delete e;
  return RATSDF_OK;
}

int ratsdf_integrate_device(ratsdf_engine* e, const void* d_rgb, const void* d_depth,
                            const void* d_ht, const void* d_lt, int height, int width,
                            float max_depth, const ratsdf_intrinsics* K, const ratsdf_pose* T) {
  ENTRY(e, d_rgb && d_depth && K && T && height > 0 && width > 0);
  if (!finite_frame(*K, *T, max_depth)) return RATSDF_ERR_BAD_ARGUMENT;
  return e->frame(ratsdf_engine::FrameIn::of(d_rgb, d_depth, d_ht, d_lt, K, T), nullptr, height, width, max_depth);
}

int ratsdf_integrate_device_batch(ratsdf_engine* e, int n, const void* const* d_rgb,
                                  const void* const* d_depth, const void* const* d_ht,
                                  const void* const* d_lt, int height, int width, float max_depth,
                                  const ratsdf_intrinsics* K, const ratsdf_pose* T) {
  ENTRY(e, n >= 0 && (n == 0 || (d_rgb && d_depth && K && T)) && height > 0 && width > 0);
  for (int i = 0; i < n; ++i)
    if (!d_rgb[i] || !d_depth[i] || !finite_frame(K[i], T[i], max_depth)) return RATSDF_ERR_BAD_ARGUMENT;
  auto input = [&](int i) { return ratsdf_engine::FrameIn::at((size_t)i, d_rgb, d_depth, d_ht, d_lt, K, T); };
  // The captured form: one graph launch for the whole batch (not while individual launches carry profiling
  // events, nor for the shapes graph_eligible refuses).
  // (profiling, mode 1: every fourth batch is launched frame by frame and carries the events -- a sample of the
  // same stream inside the same timed region; mode 2 times every frame: no graphs)
  const bool sampled = e->timer.on && (e->timer.mode == 2 || (e->prof_batch++ & 3u) == 0);
  if (!sampled && e->graph_eligible(n, height, width)) {
    const size_t npix = (size_t)height * width;
    STCHK(e->ensure_image(npix, npix * (size_t)e->S));
    ratsdf_engine::BatchGraph* g = nullptr;
    if (e->batch_graph(n, height, width, &g) == RATSDF_OK && g) {
      void* side = nullptr;
      STCHK(g->jobs.acquire(&side));  // (the copy that last used this side of the table is done)
      FrameJob* hj = static_cast<FrameJob*>(side);
      for (int i = 0; i < n; ++i) e->fill_job(hj[i], input(i), height, width, max_depth, e->parity + (unsigned)i);
      STCHK(g->jobs.commit(g->d_jobs.as<FrameJob>(), 0, (size_t)n * sizeof(FrameJob), e->stream));
      if (hipGraphLaunch(g->graph.exec(), e->stream) != hipSuccess) {
        e->abandon_pipeline();
        return RATSDF_ERR_DEVICE;
      }
      e->parity = (e->parity + (unsigned)n) & 1u;
      e->cand_ready = false;
      e->pending = true;
      return RATSDF_OK;
    }
  }
  // (mode 1 samples frames 2, 6, 10, ... of the batch, never its first: the start stamp of a dispatch that finds
  // the queue idle is taken early -- events showed 100+ us for such a frame where rocprofv3's trace of the same
  // launch shows an ordinary one, tools/event_probe.py)
  if (e->timer.on && e->timer.mode != 2 && n > 2) e->timer.frame = 2;
  for (int i = 0; i < n; ++i) {
    const ratsdf_engine::FrameIn cur = input(i);
    ratsdf_engine::FrameIn nxt{};
    if (i + 1 < n) nxt = input(i + 1);
    const int st = e->frame(cur, i + 1 < n ? &nxt : nullptr, height, width, max_depth);
    if (st != RATSDF_OK) {
      e->abandon_pipeline();
      return st;
    }
  }
  return RATSDF_OK;
}

// Builds what the first ratsdf_integrate_device_batch of this shape would build on the spot -- image-sized scratch
// and the HIP graph of an n-frame batch -- so that a caller with a deadline does not pay for allocation, capture
// and instantiation inside its first batch.  Nothing is launched; a shape the engine launches frame by frame
// anyway (n < 2, graphs off) only gets its scratch.
int ratsdf_prepare_device_batch(ratsdf_engine* e, int n, int height, int width) {
  ENTRY(e, n >= 0 && height > 0 && width > 0);
  const size_t npix = (size_t)height * width;
  if (npix * (size_t)e->S >= 0xFFFFFFFFull) return RATSDF_ERR_BAD_ARGUMENT;
  STCHK(e->ensure_image(npix, npix * (size_t)e->S));
  if (e->graph_eligible(n, height, width)) {
    ratsdf_engine::BatchGraph* g = nullptr;
    (void)e->batch_graph(n, height, width, &g);  // (a failed capture is remembered: such batches go frame by frame)
  }
  return RATSDF_OK;
}

int ratsdf_integrate(ratsdf_engine* e, const uint8_t* rgb, const float* depth, const float* ht,
                     const float* lt, int height, int width, float max_depth,
                     const ratsdf_intrinsics* K, const ratsdf_pose* T) {
  ENTRY(e, rgb && depth && K && T && height > 0 && width > 0);
  if (!finite_frame(*K, *T, max_depth)) return RATSDF_ERR_BAD_ARGUMENT;
  if (!ht || !lt) ht = lt = nullptr;  // modules/tsdf_module.cc:27-31
  const size_t npix = (size_t)height * width;
  StageRing& ring = e->ring;
  STCHK(ring.grow(npix, e->stream));
  // The slots of the staging ring, one per call in turn.  The call returns when the caller's images sit in the
  // slot's page-locked memory: the upload runs on a copy stream (it overlaps the previous frame's kernels), the
  // frame's launches follow it on the engine's stream, and nothing here waits for the GPU unless the ring is full --
  // the slot's previous upload (kStageSlots calls ago) must have left its host memory before it is overwritten.
  // (Until round 4 every call ended with a stream synchronisation: 2 700 frames/s at 640x480, a third of it the
  // single-threaded staging copy.)
  const int slot = stage_slot_of(ring.no++, 0);
  auto fail = [&](int status) { return e->host_image_fail(status); };
  // (a TSDF-only frame's two images in halves: four pieces either way)
  int st = ring.upload(slot, npix, StageImages{rgb, depth, ht, lt}, StageFrom::kPageable, ring.copy[slot & 1], 1,
                       ht ? 1 : 2);
  if (st != RATSDF_OK) return fail(st);
  if (hipStreamWaitEvent(e->stream, ring.up_ev[slot], 0) != hipSuccess) return fail(RATSDF_ERR_DEVICE);
  st = e->frame(e->ring_input(slot, npix, K, T, ht != nullptr), nullptr, height, width, max_depth);
  if (st != RATSDF_OK) return fail(st);
  // the slot's device memory is next written kStageSlots frames on (of either host-image entry point), behind this
  // event.  Nothing else on the engine's stream reads the staging slots.
  if (hipEventRecord(ring.use_ev[slot], e->stream) != hipSuccess) return fail(RATSDF_ERR_DEVICE);
  if (!e->sync_integrate) return RATSDF_OK;
  return e->sticky();  // cudaStreamSynchronize(stream_), voxel_tsdf.cu:450
}

int ratsdf_integrate_batch(ratsdf_engine* e, int n, const uint8_t* const* rgb,
                           const float* const* depth, const float* const* ht,
                           const float* const* lt, int height, int width, float max_depth,
                           const ratsdf_intrinsics* K, const ratsdf_pose* T, int pinned) {
  ENTRY(e, n >= 0 && (n == 0 || (rgb && depth && K && T)) && height > 0 && width > 0);
  for (int i = 0; i < n; ++i)
    if (!rgb[i] || !depth[i] || !finite_frame(K[i], T[i], max_depth)) return RATSDF_ERR_BAD_ARGUMENT;
  if (n == 0) return e->sticky();
  const size_t npix = (size_t)height * width;
  StageRing& ring = e->ring;
  STCHK(ring.grow(npix, e->stream));
  const uint64_t base = ring.no;  // frame i of this call takes slot stage_slot_of(base, i)
  ring.no += (uint64_t)n;
  auto sem = [&](int i) { return ht && lt && ht[i] && lt[i]; };  // tsdf_module.cc:27-31
  auto bytes_of = [](const void* p) { return reinterpret_cast<const uint8_t*>(p); };
  // a frame whose four images lie side by side in one page-locked block in the slot's own order (ratsdf::TSDFSystem's
  // queue keeps them so): one copy instead of four -- each costs ~10 us of launch overhead on the copy engine
  auto packed = [&](int i) {
    const uint8_t* h0 = bytes_of(depth[i]);
    return pinned && sem(i) && bytes_of(ht[i]) == h0 + npix * 4 && bytes_of(lt[i]) == h0 + npix * 8 &&
           bytes_of(rgb[i]) == h0 + npix * 12;
  };
  // ... and frame i + k a block k ring strides behind it (the blocks of one arena of ratsdf::HostBlockPool)
  auto adjacent = [&](int i, int k) {
    return npix == ring.pix && bytes_of(depth[i + k]) == bytes_of(depth[i]) + (size_t)k * ring.stride();
  };
  // Uploads run on their own streams, ahead of the frames that use them (stage_plan.h), so the PCIe copy of later
  // frames overlaps the integration of earlier ones (one stream would serialise them).
  // (No fence against earlier calls: frames of earlier host-image calls that are still in flight are what the
  // slots' events stand for, and nothing else on the engine's stream touches the staging slots.  Until round 5
  // every call began by making both copy streams wait for ALL earlier work of the engine's stream and ended with
  // a synchronisation: the link idled ~0.4 ms per 32-frame call, 13 % of it -- tools/copy_gaps.py.)
  unsigned copy_no = 0;
  auto upload = [&](int i, int max_run) {
    const int slot = stage_slot_of(base, i);
    const int run = stage_run_length(i, n, slot, max_run, packed, adjacent);
    const StageImages im{rgb[i], depth[i], sem(i) ? ht[i] : nullptr, sem(i) ? lt[i] : nullptr};
    const StageFrom from = packed(i) ? StageFrom::kPacked : pinned ? StageFrom::kPinned : StageFrom::kPageable;
    return StageTook{run, ring.upload(slot, npix, im, from, ring.copy[(copy_no++ & 1u) && ring.two_streams], run)};
  };
  auto input = [&](int i) { return e->ring_input(stage_slot_of(base, i), npix, &K[i], &T[i], sem(i)); };
  auto launch = [&](int i) -> int {
    if (hipStreamWaitEvent(e->stream, ring.up_ev[stage_slot_of(base, i)], 0) != hipSuccess ||
        (i + 1 < n && hipStreamWaitEvent(e->stream, ring.up_ev[stage_slot_of(base, i + 1)], 0) != hipSuccess))
      return RATSDF_ERR_DEVICE;
    const ratsdf_engine::FrameIn cur = input(i);
    ratsdf_engine::FrameIn nxt{};
    if (i + 1 < n) nxt = input(i + 1);
    STCHK(e->frame(cur, i + 1 < n ? &nxt : nullptr, height, width, max_depth));
    // frame i's images were last read by its candidate pass, which ran in frame i-1's launches or
    // before; recording after frame i is the simple, safe point
    return hipEventRecord(ring.use_ev[stage_slot_of(base, i)], e->stream) == hipSuccess ? RATSDF_OK : RATSDF_ERR_DEVICE;
  };
  // whatever happens, the caller's buffers (and the staging slots) are no longer in use on return
  auto fail = [&](int status) { return e->host_image_fail(status); };
  int st = stage_schedule(n, upload, launch);
  if (st != RATSDF_OK) return fail(st);
  // The call returns when the caller's buffers are no longer in use: at once for pageable images (they were copied
  // into the staging ring), after the last upload for page-locked ones.  It does not wait for the frames'
  // kernels -- the next call's uploads overlap them -- so a device error of these frames is reported by the next
  // entry point that synchronises, as for ratsdf_integrate.
  if (pinned && ring.drain() != RATSDF_OK) return fail(RATSDF_ERR_DEVICE);
  if (!e->sync_integrate) return RATSDF_OK;
  st = e->sticky();
  if (st == RATSDF_ERR_DEVICE) return fail(st);
  return st;
}

int ratsdf_host_alloc(size_t bytes, void** out) {
  if (!out) return RATSDF_ERR_BAD_ARGUMENT;
  *out = nullptr;
  if (bytes == 0) return RATSDF_OK;
  HIPCHK(hipHostMalloc(out, bytes, hipHostMallocDefault));  // (the caller's from here on: ratsdf_host_free)
  return RATSDF_OK;
}

int ratsdf_host_free(void* p) {
  if (p) HIPCHK(hipHostFree(p));
  return RATSDF_OK;
}

int ratsdf_synchronize(ratsdf_engine* e) {
  ENTRY(e, true);
  // (no k_settle here: what the last frame's carve pass still owes -- pool releases, its statistics -- is done by the
  // next frame's launches, or by the entry point that reads the map, the free list or the statistics: each of them
  // settles first.  A caller that synchronises after every frame, TSDFGrid::Integrate's convention, paid a fourth
  // launch per frame for it.)
  return e->sticky();
}


// After a sticky error (RATSDF_ERR_TIMEOUT above all: a workgroup gave up waiting and skipped its share of a frame) the
// map is what the frames before left plus a part of the failed one, and the structures DERIVED from the directory no
// longer agree with it: pool indices reserved by a serial role whose commits were skipped, claims never reset, counters
// of a frame that nobody finalised.  The directory itself is whole -- the workgroups that EDIT it (the resolvers, the
// serial role) are the ones that were waited for, they never give up and have finished by the time the stream is idle.
// So: everything is rebuilt from the directory -- occupancy bits, Table::active, the free list (the pool blocks no
// entry names, ascending), the free count and its low-water mark -- the claim tables, both frames' counters, the
// candidate counters and the delete bitmaps go back to their initial state, a consumer of directory deltas is told to
// take a whole directory next, and the error is cleared.  The voxels keep what reached them.  No reference counterpart.
// keep_heap: the free list, the free count and its low-water mark are left as they are (ratsdf_load_map has just
// written them); otherwise they are rebuilt from the directory, ascending.
static int rebuild_derived(ratsdf_engine* e, bool keep_heap) {
  HIPCHK(hipStreamSynchronize(e->stream));
  STCHK(e->ring.drain());
  Table& t = e->tab;
  const uint32_t occ_words = (t.num_entry + 63) / 64;
  const size_t nb = (size_t)t.num_block;
  const uint32_t ntiles = (uint32_t)scan_tiles(nb);
  DevMem tmp;  // unused flags | positions | tile sums | total
  STCHK(tmp.alloc((2 * nb + ntiles + 2) * 4));
  uint32_t *unused = tmp.as<uint32_t>(), *pos = unused + nb, *tiles = pos + nb, *d_total = tiles + ntiles + 1;
  StreamDrain drain{e->stream};
  HIPCHK(hipMemsetAsync(t.occ, 0, (size_t)occ_words * 8, e->stream));
  HIPCHK(hipMemsetAsync(t.active, 0xFF, nb * sizeof(VisItem), e->stream));
  HIPCHK(hipMemsetAsync(t.claim, 0xFF, (size_t)t.num_bucket * 4, e->stream));
  HIPCHK(hipMemsetAsync(t.dclaim, 0xFF, (size_t)t.num_bucket * 4, e->stream));
  HIPCHK(hipMemsetAsync(e->dbitmap, 0, (size_t)e->dwords * 4, e->stream));
  HIPCHK(hipMemsetAsync(e->dsummary, 0, (size_t)((e->dwords / kGroupWords + 31) / 32) * 4, e->stream));
  if (e->abitmap) {
    HIPCHK(hipMemsetAsync(e->abitmap, 0, (size_t)e->awords_cap * 4, e->stream));
    HIPCHK(hipMemsetAsync(e->asummary, 0, (size_t)e->asum_words * 4, e->stream));
  }
  HIPCHK(hipMemsetAsync(e->cand_count, 0, 2 * kCandSegs * kCandCountStride * 4, e->stream));
  for (int i = 0; i < 2; ++i) HIPCHK(hipMemsetAsync(e->upd_wg[i], 0, kUpdCounters * 4, e->stream));
  HIPCHK(hipMemsetAsync(&e->ctl->fr[0], 0, 2 * sizeof(FrameCtl), e->stream));
  hipLaunchKernelGGL(k_fill_u32, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, e->stream, unused, 1u, nb);
  hipLaunchKernelGGL(k_recover_scan, dim3((t.num_entry + 255) / 256), dim3(256), 0, e->stream, t, unused);
  if (!keep_heap) {
    uint32_t n_free = 0;
    STCHK(mask_positions(e, unused, nb, pos, tiles, d_total, &n_free));
    hipLaunchKernelGGL(k_recover_heap, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, e->stream, unused, pos,
                       e->pool.heap, (int32_t)nb);
    const int32_t nf = (int32_t)n_free;
    HIPCHK(hipMemcpyAsync(&e->ctl->num_free, &nf, 4, hipMemcpyHostToDevice, e->stream));
    // (the low-water mark only ever goes down: slots at or above it may have been in use; the rebuilt heap keeps the
    // never-used indices -- the lowest ones -- at its bottom, so the mark stays true.  A free count below it moves it.)
    int32_t low = 0;
    HIPCHK(hipMemcpyAsync(&low, &e->ctl->free_low, 4, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (nf < low) HIPCHK(hipMemcpyAsync(&e->ctl->free_low, &nf, 4, hipMemcpyHostToDevice, e->stream));
  }
  if (t.delta_on) {  // the delta log no longer describes what changed: the next export reports an overflow
    const uint32_t over = 0x80000000u;
    HIPCHK(hipMemcpyAsync(t.del_count, &over, 4, hipMemcpyHostToDevice, e->stream));
  }
  const uint32_t zero = 0;
  HIPCHK(hipMemcpyAsync(&e->ctl->error, &zero, 4, hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(e->stream));
  e->h_err[0] = e->h_err[1] = 0u;
  e->pending = false;
  e->cand_ready = false;
  return RATSDF_OK;
}

int ratsdf_recover(ratsdf_engine* e) {
  ENTRY(e, true);
  return rebuild_derived(e, false);
}

int ratsdf_stream(ratsdf_engine* e, void** out) {
  ENTRY(e, out);
  *out = (void*)e->stream;
  return RATSDF_OK;
}

int ratsdf_profile_enable(ratsdf_engine* e, int enable) {
  ENTRY(e, true);
  KernelTimer& t = e->timer;
  const int st = t.drain(e->stream);
  t.on = enable != 0;
  t.mode = enable == 2 ? 2 : 1;
  t.k_us.clear();
  t.period_us.clear();
  return st;
}

int ratsdf_profile_read_frames(ratsdf_engine* e, float* k_us, float* period_us, int capacity, int* n) {
  ENTRY(e, n && capacity >= 0);
  KernelTimer& t = e->timer;
  const int st = t.read(e->stream, nullptr, nullptr);
  const int have = (int)t.k_us.size();
  *n = have;
  for (int i = 0; i < have && i < capacity; ++i) {
    if (k_us) k_us[i] = t.k_us[(size_t)i];
    if (period_us) period_us[i] = (size_t)i < t.period_us.size() ? t.period_us[(size_t)i] : 0.f;
  }
  t.k_us.clear();
  t.period_us.clear();
  return st;
}

int ratsdf_profile_read(ratsdf_engine* e, double* ms, int64_t* launches) {
  ENTRY(e, true);
  return e->timer.read(e->stream, ms, launches);
}

int ratsdf_num_active_blocks(ratsdf_engine* e, int32_t* out) {
  ENTRY(e, out);
  STCHK(e->settle());
  int32_t nf = 0;
  STCHK(e->read_small(&nf, &e->ctl->num_free, 4));
  *out = e->tab.num_block - nf;
  return RATSDF_OK;
}

int ratsdf_last_frame_stats(ratsdf_engine* e, ratsdf_frame_stats* out) {
  ENTRY(e, out);
  STCHK(e->settle());
  STCHK(e->read_small(out, e->d_stats, sizeof(*out)));
  return RATSDF_OK;
}

int ratsdf_totals(ratsdf_engine* e, int64_t* out5, int reset) {
  ENTRY(e, true);
  STCHK(e->settle());
  unsigned long long t[5] = {0, 0, 0, 0, 0};
  STCHK(e->read_small(t, e->ctl->totals, sizeof(t)));
  if (reset) HIPCHK(hipMemsetAsync(e->ctl->totals, 0, sizeof(t), e->stream));
  if (out5)
    for (int i = 0; i < 5; ++i) out5[i] = (int64_t)t[i];
  return RATSDF_OK;
}

int ratsdf_pipeline_counters(ratsdf_engine* e, int64_t* out4, int reset) {
  ENTRY(e, true);
  unsigned long long t[4] = {0, 0, 0, 0};
  STCHK(e->read_small(t, e->ctl->paths, sizeof(t)));
  if (reset) HIPCHK(hipMemsetAsync(e->ctl->paths, 0, sizeof(t), e->stream));
  if (out4)
    for (int i = 0; i < 4; ++i) out4[i] = (int64_t)t[i];
  return RATSDF_OK;
}

const char* ratsdf_status_string(int s) {
  switch (s) {
    case RATSDF_OK: return "ok";
    case RATSDF_ERR_BAD_ARGUMENT: return "bad argument";
    case RATSDF_ERR_DEVICE: return "device / allocation error";
    case RATSDF_ERR_POOL_EXHAUSTED: return "voxel block pool exhausted";
    case RATSDF_ERR_CAPACITY: return "internal work list overflow";
    case RATSDF_ERR_NO_DEVICE: return "no HIP device";
    case RATSDF_ERR_NOT_IMPLEMENTED: return "not implemented";
    case RATSDF_ERR_TIMEOUT: return "in-launch wait between workgroups timed out";
    default: return "unknown status";
  }
}
const char* ratsdf_backend(void) { return "hip-gfx950"; }

}  // extern "C"

// Above: creation, the integrate family, synchronise, recover, profile and the counters.  The other entry-point
// families, one file each (this stays ONE translation unit: the files need the engine record, the
// macros and the helpers above, and the order of the kernels is the order of the headers and of mapfile.inc).
#include "debug.inc"    // ratsdf_debug_*: readers of the diagnostic build's stamps and counters
#include "query.inc"    // ratsdf_query / ratsdf_gather_valid* / ratsdf_download_all* / ratsdf_raycast*
#include "sample.inc"   // ratsdf_sample_points[_device] (include/ratsdf_sample.h)
#include "esdf.inc"     // ratsdf_esdf[_device] (include/ratsdf_esdf.h)
#include "surface.inc"  // ratsdf_surface_points[_device] (include/ratsdf_surface.h)
#include "blocks.inc"   // directory export and delta, block import / export, ratsdf_test_*, ratsdf_dump_*
#include "group.inc"    // ratsdf_group_*: several engines of one device stepped together
#include "mapfile.inc"  // ratsdf_save_map / ratsdf_load_map / ratsdf_map_file_info (include/ratsdf_map.h)
#include "fuse.inc"     // ratsdf_fuse_map / ratsdf_fuse_blocks[_device] / ratsdf_fuse_map_file (include/ratsdf_fuse.h)
#include "resample.inc" // ratsdf_resample_blocks_device / ratsdf_fuse_map_transformed (include/ratsdf_resample.h)
#include "coarsen.inc"  // ratsdf_coarsen_blocks_device / ratsdf_fuse_map_coarsened (include/ratsdf_coarsen.h)
#include "surface_mesh.inc"  // ratsdf_surface_mesh[_device] (include/ratsdf_surface_mesh.h)
#include "cluster_mesh.inc"  // ratsdf_cluster_mesh[_device] (include/ratsdf_cluster_mesh.h)
#include "regions.inc"  // ratsdf_regions[_device] (include/ratsdf_regions.h)
#include "cost.inc"     // ratsdf_cost_to_go[_device] (include/ratsdf_cost.h)
#include "score.inc"    // ratsdf_labelset_* / ratsdf_score_labels[_device] (include/ratsdf_score.h)
#include "score_mesh.inc"  // ratsdf_labelmesh_* / ratsdf_score_mesh[_device] (include/ratsdf_score_mesh.h)
#include "exposure.inc"  // ratsdf_exposure[_device] (include/ratsdf_surface.h)
