// hip_handles.h -- the owners of what the runtime hands out besides memory (hip_mem.h): an event, a stream, a
// captured graph with its executable; and the twin page-locked table built from them.  As for HipMem: an owner is
// empty by default, move-only, create() leaves it empty after a failure, and the handle is destroyed exactly once, in
// reset() or the destructor.  An owner never synchronises: whether queued work still uses a handle is what the call
// site knows, and its hipStreamSynchronize / hipEventSynchronize stands in front of the reset() or the end of the
// owner's life.  Where several owners are members of one struct, the members' declaration order (reversed) is the
// order of destruction; the structs that depend on it say so.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <utility>

#include "hip_mem.h"

namespace ratsdf {

namespace detail {
struct EventKind {
  using Handle = hipEvent_t;
  static constexpr const char* kCreate = "hipEventCreateWithFlags";
  static hipError_t create(Handle* h, unsigned flags) { return hipEventCreateWithFlags(h, flags); }
  static hipError_t destroy(Handle h) { return hipEventDestroy(h); }
};
struct StreamKind {
  using Handle = hipStream_t;
  static constexpr const char* kCreate = "hipStreamCreateWithFlags";
  static hipError_t create(Handle* h, unsigned flags) { return hipStreamCreateWithFlags(h, flags); }
  static hipError_t destroy(Handle h) { return hipStreamDestroy(h); }
};
// RATSDF_OK, or the failed call named on stderr and RATSDF_ERR_DEVICE
inline int checked(hipError_t err, const char* call) {
  if (err == hipSuccess) return RATSDF_OK;
  fprintf(stderr, "[ratsdf] HIP error %s at %s: %s\n", hipGetErrorName(err), __FILE__, call);
  return RATSDF_ERR_DEVICE;
}
}  // namespace detail

template <class Kind>
class HipHandle {
 public:
  using Handle = typename Kind::Handle;
  HipHandle() = default;
  HipHandle(HipHandle&& o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
  HipHandle& operator=(HipHandle&& o) noexcept {  // (destroys what THIS held; what moves in is not touched)
    if (this != &o) {
      reset();
      h_ = std::exchange(o.h_, nullptr);
    }
    return *this;
  }
  HipHandle(const HipHandle&) = delete;
  HipHandle& operator=(const HipHandle&) = delete;
  ~HipHandle() { reset(); }

  void reset() {
    if (h_) (void)Kind::destroy(h_);
    h_ = nullptr;
  }
  // destroys what it held, then creates: RATSDF_OK, or RATSDF_ERR_DEVICE with the owner left empty
  int create(unsigned flags) {
    reset();
    Handle h = nullptr;
    const int st = detail::checked(Kind::create(&h, flags), Kind::kCreate);
    if (st == RATSDF_OK) h_ = h;
    return st;
  }
  // the raw handle (null while empty): what every call of the runtime takes
  operator Handle() const { return h_; }

 private:
  Handle h_ = nullptr;
};
using HipEvent = HipHandle<detail::EventKind>;    // create(hipEventDisableTiming), create(hipEventDefault)
using HipStream = HipHandle<detail::StreamKind>;  // create(hipStreamNonBlocking)

// A captured graph and the executable graph made of it; the executable goes first.
class HipGraph {
 public:
  HipGraph() = default;
  HipGraph(HipGraph&& o) noexcept : graph_(std::exchange(o.graph_, nullptr)), exec_(std::exchange(o.exec_, nullptr)) {}
  HipGraph& operator=(HipGraph&& o) noexcept {
    if (this != &o) {
      reset();
      graph_ = std::exchange(o.graph_, nullptr);
      exec_ = std::exchange(o.exec_, nullptr);
    }
    return *this;
  }
  HipGraph(const HipGraph&) = delete;
  HipGraph& operator=(const HipGraph&) = delete;
  ~HipGraph() { reset(); }

  void reset() {
    if (exec_) (void)hipGraphExecDestroy(exec_);
    if (graph_) (void)hipGraphDestroy(graph_);
    exec_ = nullptr;
    graph_ = nullptr;
  }
  // ends the capture that hipStreamBeginCapture began on `s` and takes the graph; a capture that yields none is a
  // failure (the owner is empty then).  A call that fails hands nothing out: what it may have written into the handle
  // is not the owner's and is not destroyed (the runtime does write one when no capture was under way).
  int end_capture(hipStream_t s) {
    reset();
    hipGraph_t g = nullptr;
    if (hipStreamEndCapture(s, &g) != hipSuccess || !g) return RATSDF_ERR_DEVICE;
    graph_ = g;
    return RATSDF_OK;
  }
  // the executable of the captured graph (which it keeps); after a failure the owner is empty
  int instantiate() {
    hipGraphExec_t x = nullptr;
    if (!graph_ || hipGraphInstantiate(&x, graph_, nullptr, nullptr, 0) != hipSuccess || !x) {
      reset();
      return RATSDF_ERR_DEVICE;
    }
    if (exec_) (void)hipGraphExecDestroy(exec_);
    exec_ = x;
    return RATSDF_OK;
  }
  hipGraphExec_t exec() const { return exec_; }
  explicit operator bool() const { return exec_ != nullptr; }

 private:
  hipGraph_t graph_ = nullptr;
  hipGraphExec_t exec_ = nullptr;
};

// Two page-locked sides used alternately, each guarded by the event of the last copy out of it: the host fills one
// side while the copy out of the other may still be pending.  acquire() picks the next side, waits for its event (one
// never recorded counts as complete) and hands out its memory; copy() queues a copy of a part of that side to device
// memory; commit() does the same and then records the side's event on the stream -- the last copy of a turn is a
// commit().  Destruction: the events, then the memory (declaration order); the stream's drain is the holder's.
class TwinTable {
 public:
  // both sides hold at least `bytes` and their events exist; the contents are NOT carried over.  After a failure
  // size() is 0 and the next grow() goes through the allocations again.  (What is queued may still use the old
  // sides: the call site drains its stream first.)
  int grow(size_t bytes) {
    if (bytes <= size()) return RATSDF_OK;
    for (int i = 0; i < 2; ++i) {
      int st = side_[i].alloc(bytes);
      if (st == RATSDF_OK && !ev_[i]) st = ev_[i].create(hipEventDisableTiming);
      if (st != RATSDF_OK) {
        side_[0].reset();
        side_[1].reset();
        return st;
      }
    }
    return RATSDF_OK;
  }
  size_t size() const { return side_[0].size() < side_[1].size() ? side_[0].size() : side_[1].size(); }
  // the next side's memory in *host, once the last copy out of it has been executed
  int acquire(void** host) {
    *host = nullptr;
    if (!size()) return RATSDF_ERR_DEVICE;
    const unsigned s = turn_ & 1u;
    const int st = detail::checked(hipEventSynchronize(ev_[s]), "hipEventSynchronize");
    if (st != RATSDF_OK) return st;
    cur_ = s;
    ++turn_;
    *host = side_[s].as<void>();
    return RATSDF_OK;
  }
  // bytes [off, off + bytes) of the acquired side to `dst`, asynchronously on `stream`
  int copy(void* dst, size_t off, size_t bytes, hipStream_t stream) {
    if (off + bytes > side_[cur_].size()) return RATSDF_ERR_DEVICE;
    return detail::checked(
        hipMemcpyAsync(dst, side_[cur_].as<unsigned char>() + off, bytes, hipMemcpyHostToDevice, stream),
        "hipMemcpyAsync");
  }
  // ... and the side's event behind it
  int commit(void* dst, size_t off, size_t bytes, hipStream_t stream) {
    const int st = copy(dst, off, bytes, stream);
    if (st != RATSDF_OK) return st;
    return detail::checked(hipEventRecord(ev_[cur_], stream), "hipEventRecord");
  }

 private:
  HostMem side_[2];  // (declared before the events: freed after them)
  HipEvent ev_[2];
  unsigned turn_ = 0, cur_ = 0;
};

}  // namespace ratsdf
