// stage_ring.inc -- what the host-image entry points (ratsdf_integrate, ratsdf_integrate_batch) own: the ring of
// staging slots, its events and copy streams, and the helper threads of its host copies.  Included by
// ratsdf_engine.hip in front of ratsdf_engine, which holds ONE StageRing; the schedule of a batch is stage_plan.h's.

// Staging copies of the host-image entry points (caller's pageable images -> the engine's page-locked slot):
// a 640x480 frame is 4.6 MB, which one core copies at ~10 GB/s -- 2 200 frames/s before anything else
// happens.  The images of a frame are copied side by side by a few helper threads (started on first use,
// parked on a condition variable in between); the caller takes the last piece itself.
class HostCopyPool {
 public:
  struct Piece {
    void* dst;
    const void* src;
    size_t bytes;
  };
  // (thread creation can fail -- RLIMIT_NPROC, a cgroup's pids limit -- and nothing may be thrown through the C
  // ABI: the pool carries on with the helpers that did start; with none, copy() is a plain memcpy loop)
  explicit HostCopyPool(unsigned helpers) {
    for (unsigned i = 0; i < helpers; ++i) {
      try {
        threads_.emplace_back([this] { run(); });
      } catch (...) {
        break;
      }
    }
  }
  ~HostCopyPool() {
    {
      std::lock_guard<std::mutex> lk(m_);
      stop_ = true;
    }
    cv_.notify_all();
    for (auto& t : threads_) t.join();
  }
  // copies every piece; returns when all are done (one caller at a time: the engine's entry points are
  // serialised per handle, SURVEY 8b "Threading")
  void copy(const Piece* pieces, int n) {
    if (n <= 0) return;
    {
      std::lock_guard<std::mutex> lk(m_);
      pieces_ = pieces;
      next_ = 0;
      count_ = n - 1;  // the caller keeps the last one
      pending_.store(n - 1, std::memory_order_relaxed);
    }
    if (n > 1) cv_.notify_all();
    memcpy(pieces[n - 1].dst, pieces[n - 1].src, pieces[n - 1].bytes);
    take_pieces();  // whatever the helpers have not picked up yet
    while (pending_.load(std::memory_order_acquire) != 0) std::this_thread::yield();
  }

 private:
  void take_pieces() {
    for (;;) {
      const Piece* p = nullptr;
      {
        std::lock_guard<std::mutex> lk(m_);
        if (next_ < count_) p = &pieces_[next_++];
      }
      if (!p) return;
      memcpy(p->dst, p->src, p->bytes);
      pending_.fetch_sub(1, std::memory_order_release);
    }
  }
  void run() {
    for (;;) {
      {
        std::unique_lock<std::mutex> lk(m_);
        cv_.wait(lk, [this] { return stop_ || next_ < count_; });
        if (stop_) return;
      }
      take_pieces();
    }
  }
  std::vector<std::thread> threads_;
  std::mutex m_;
  std::condition_variable cv_;
  const Piece* pieces_ = nullptr;
  int next_ = 0, count_ = 0;
  std::atomic<int> pending_{0};
  bool stop_ = false;
};

// A slot of the ring (depth | ht | lt | rgb, 16 bytes per pixel of the ring's largest image): its page-locked and
// its device memory, for an image of npix pixels.
struct StageSlot {
  uint8_t *h, *d;
  size_t npix;
};
// The caller's four images of a frame (ht == lt == nullptr: a TSDF-only frame), and where they lie.
struct StageImages {
  const void *rgb, *depth, *ht, *lt;
};
enum class StageFrom {
  kPageable,  // anywhere: copied into the slot's page-locked memory by the helper threads, and up from there
  kPinned,    // four page-locked images: straight from the caller's buffers
  kPacked     // page-locked, semantic, in the slot's own order in one block: one copy, for a run of frames that lie
              // side by side at the ring's stride too (stage_plan.h: stage_run_length)
};

// Both host-image entry points use the slots as ONE ring (slot = no % kStageSlots, counted over every frame either of
// them has taken) and neither waits for its frames: what a slot's next user has to wait for is in the slot's two
// events, whichever call recorded them -- no fence between calls.
// The members' declaration order is the reverse of their destruction: the memory goes first, then the events, then
// the streams (drain() stands in front of it: ~ratsdf_engine).
struct StageRing {
  HipStream copy[2];             // uploads: ratsdf_integrate by slot parity, a batch's copies alternately (two copy
                                 // engines: one sustains ~31 GB/s)
  HipEvent up_ev[kStageSlots];   // upload of the slot's last user has been executed
  HipEvent use_ev[kStageSlots];  // the frame that read the slot has been executed
  DevMem d_mem;
  HostMem h_mem;
  size_t pix = 0;            // pixels of a slot: the ring's stride is pix * 16 bytes
  uint64_t no = 0;           // frames taken so far
  bool two_streams = true;   // RATSDF_COPY_STREAMS=1: a batch's copies all on copy[0]
  std::unique_ptr<HostCopyPool> pool;  // started on first use: copy_pool()
  HostCopyPool* copy_pool() {          // (nullptr when it cannot be had: the callers copy by themselves then)
    if (!pool) pool.reset(new (std::nothrow) HostCopyPool(3));
    return pool.get();
  }

  // both copy streams idle: nothing queued reads a slot's page-locked memory or the caller's buffers any more
  int drain() {
    for (HipStream& s : copy)
      if (s) HIPCHK(hipStreamSynchronize(s));
    return RATSDF_OK;
  }
  // slots of at least npix pixels; `reader` is the stream whose frames read the slots (drained before they go)
  int grow(size_t npix, hipStream_t reader) {
    if (npix <= pix) return RATSDF_OK;
    STCHK(drain());
    HIPCHK(hipStreamSynchronize(reader));
    pix = 0;  // (a failure below leaves no capacity: the next call comes through here again)
    const size_t bytes = npix * 16 * kStageSlots;  // per slot: depth 4 + ht 4 + lt 4 + rgb 3 (padded to 4)
    h_mem.reset();
    d_mem.reset();
    STCHK(h_mem.alloc(bytes));
    STCHK(d_mem.alloc(bytes));
    for (HipEvent& ev : up_ev)
      if (!ev) STCHK(ev.create(hipEventDisableTiming));
    for (HipEvent& ev : use_ev)
      if (!ev) STCHK(ev.create(hipEventDisableTiming));
    for (HipStream& s : copy)
      if (!s) STCHK(s.create(hipStreamNonBlocking));
    pix = npix;
    return RATSDF_OK;
  }
  // (the slot stride is the ring's, not the call's: a smaller image after a larger one must land in the SAME slot
  // memory the slot's events guard -- with a per-call stride its bytes would fall inside other slots that frames of
  // earlier calls, which are not waited for, may still be reading)
  size_t stride() const { return pix * 16; }
  StageSlot slot(int i, size_t npix) const {
    const size_t off = (size_t)i * stride();
    return StageSlot{h_mem.as<uint8_t>() + off, d_mem.as<uint8_t>() + off, npix};
  }

  // Uploads the frame `im` of npix pixels into slot `first` on copy stream `cs` -- `run` frames into slots
  // [first, first + run) when they are packed and lie side by side (ONE copy: 16 bytes per pixel, the 15 a frame has +
  // the slot's pad).  A pageable frame passes through the slot's page-locked memory, every image in `parts` pieces of
  // about equal size, once the slot's last upload has left it.  The copies wait for the slots' last readers (frames of
  // this call or of an earlier one; an event never recorded counts as complete) and the slots' upload events follow
  // them.
  int upload(int first, size_t npix, const StageImages& im, StageFrom from, hipStream_t cs, int run = 1, int parts = 1) {
    const StageSlot s = slot(first, npix);
    if (from == StageFrom::kPageable) {
      HIPCHK(hipEventSynchronize(up_ev[first]));
      fill(s, im, parts);
    }
    for (int j = 0; j < run; ++j) HIPCHK(hipStreamWaitEvent(cs, use_ev[first + j], 0));
    if (from == StageFrom::kPacked) {
      HIPCHK(hipMemcpyAsync(s.d, im.depth, (size_t)(run - 1) * stride() + npix * 15, hipMemcpyHostToDevice, cs));
    } else if (from == StageFrom::kPageable && im.ht) {
      HIPCHK(hipMemcpyAsync(s.d, s.h, npix * 15, hipMemcpyHostToDevice, cs));
    } else {  // image by image: from the caller's buffers, or depth and rgb of a TSDF-only frame from the slot's
      const bool own = from == StageFrom::kPageable;
      HIPCHK(hipMemcpyAsync(s.d, own ? s.h : im.depth, npix * 4, hipMemcpyHostToDevice, cs));
      if (im.ht) {
        HIPCHK(hipMemcpyAsync(s.d + npix * 4, im.ht, npix * 4, hipMemcpyHostToDevice, cs));
        HIPCHK(hipMemcpyAsync(s.d + npix * 8, im.lt, npix * 4, hipMemcpyHostToDevice, cs));
      }
      HIPCHK(hipMemcpyAsync(s.d + npix * 12, own ? s.h + npix * 12 : im.rgb, npix * 3, hipMemcpyHostToDevice, cs));
    }
    for (int j = 0; j < run; ++j) HIPCHK(hipEventRecord(up_ev[first + j], cs));
    return RATSDF_OK;
  }

 private:
  // The caller's pageable images into the slot's page-locked memory, side by side by the copy helpers.
  void fill(const StageSlot& s, const StageImages& im, int parts) {
    HostCopyPool::Piece pieces[8];
    int np = 0;
    auto add = [&](size_t off, const void* src, size_t bytes) {
      const size_t step = ((bytes + parts - 1) / parts + 63) & ~(size_t)63;
      for (size_t o = 0; o < bytes; o += step)
        pieces[np++] = HostCopyPool::Piece{s.h + off + o, (const uint8_t*)src + o, std::min(step, bytes - o)};
    };
    add(0, im.depth, s.npix * 4);
    if (im.ht) {
      add(s.npix * 4, im.ht, s.npix * 4);
      add(s.npix * 8, im.lt, s.npix * 4);
    }
    add(s.npix * 12, im.rgb, s.npix * 3);
    if (HostCopyPool* cp = copy_pool()) {
      cp->copy(pieces, np);
    } else {
      for (int i = 0; i < np; ++i) memcpy(pieces[i].dst, pieces[i].src, pieces[i].bytes);
    }
  }
};
