// test_hip_handles.cc -- the invariants of ra-slam_amd/csrc/hip_handles.h: the owners of an event, a stream and a
// captured graph with its executable, and the twin page-locked table.
//
// Runs twice (tests/test_hip_handles.py): against the HIP runtime as it is on this machine -- without a GPU every
// create fails (no device) and the failure branch is what is exercised, on an MI355X the success branch -- and against
// a stand-in that hands out handles of its own and can be told to fail, so that both branches are checked on every
// machine.  Every create, destroy, wait, record and copy that the header makes goes through a counter and a log: a
// handle is destroyed exactly once, never twice, none leaks; the table's calls come in the order it promises.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

namespace {
bool g_fake = false;        // the stand-in instead of the runtime
bool g_fake_fails = false;  // ... refusing every create and allocation
int g_fail_after = -1;      // ... or refusing once that many more have succeeded (-1: never)
std::map<void*, char> g_live;  // what an owner has been given and has not given back: handle -> kind
int g_destroys = 0, g_bad_destroys = 0, g_creates = 0;
struct Call {
  char what;  // 'W' event wait, 'R' event record, 'C' copy
  void* handle;
  const void* src;
  size_t bytes;
};
std::vector<Call> g_log;

bool fake_refuses() {
  if (g_fake_fails) return true;
  if (g_fail_after == 0) return true;
  if (g_fail_after > 0) --g_fail_after;
  return false;
}
template <class H>
hipError_t made(hipError_t err, H* h, char kind) {
  if (err == hipSuccess && *h) {
    g_live[(void*)*h] = kind;
    ++g_creates;
  }
  return err;
}
// (a refusal still writes something into the handle, as the runtime's hipStreamEndCapture does when no capture is under
// way: it is not the caller's, and destroying it counts as a bad destroy)
char g_junk[8];
template <class H>
hipError_t fake_create(H* h, char kind) {
  if (fake_refuses()) {
    *h = (H)(void*)g_junk;
    return hipErrorOutOfMemory;
  }
  *h = (H)malloc(8);
  return made(*h ? hipSuccess : hipErrorOutOfMemory, h, kind);
}
// the handle leaves the books; false: never handed out, of another kind, or given back before
bool given_back(void* h, char kind) {
  ++g_destroys;
  const auto it = g_live.find(h);
  if (it == g_live.end() || it->second != kind) {
    ++g_bad_destroys;
    return false;
  }
  g_live.erase(it);
  return true;
}

hipError_t test_event_create(hipEvent_t* e, unsigned flags) {
  return g_fake ? fake_create(e, 'e') : made(hipEventCreateWithFlags(e, flags), e, 'e');
}
hipError_t test_event_destroy(hipEvent_t e) {
  if (!given_back((void*)e, 'e')) return hipErrorInvalidHandle;
  if (g_fake) return free((void*)e), hipSuccess;
  return hipEventDestroy(e);
}
hipError_t test_stream_create(hipStream_t* s, unsigned flags) {
  return g_fake ? fake_create(s, 's') : made(hipStreamCreateWithFlags(s, flags), s, 's');
}
hipError_t test_stream_destroy(hipStream_t s) {
  if (!given_back((void*)s, 's')) return hipErrorInvalidHandle;
  if (g_fake) return free((void*)s), hipSuccess;
  return hipStreamDestroy(s);
}
hipError_t test_end_capture(hipStream_t s, hipGraph_t* g) {
  return g_fake ? fake_create(g, 'g') : made(hipStreamEndCapture(s, g), g, 'g');
}
hipError_t test_graph_destroy(hipGraph_t g) {
  if (!given_back((void*)g, 'g')) return hipErrorInvalidHandle;
  if (g_fake) return free((void*)g), hipSuccess;
  return hipGraphDestroy(g);
}
hipError_t test_instantiate(hipGraphExec_t* x, hipGraph_t g, hipGraphNode_t* n, char* log, size_t bytes) {
  if (g_fake) return g_live.count((void*)g) ? fake_create(x, 'x') : hipErrorInvalidValue;
  return made(hipGraphInstantiate(x, g, n, log, bytes), x, 'x');
}
hipError_t test_exec_destroy(hipGraphExec_t x) {
  if (!given_back((void*)x, 'x')) return hipErrorInvalidHandle;
  if (g_fake) return free((void*)x), hipSuccess;
  return hipGraphExecDestroy(x);
}
hipError_t test_host_malloc(void** p, size_t bytes, unsigned flags) {
  if (g_fake) {
    return fake_refuses() ? hipErrorOutOfMemory : made((*p = malloc(bytes)) ? hipSuccess : hipErrorOutOfMemory, p, 'h');
  }
  return made(hipHostMalloc(p, bytes, flags), p, 'h');
}
hipError_t test_host_free(void* p) {
  if (!given_back(p, 'h')) return hipErrorInvalidValue;
  if (g_fake) return free(p), hipSuccess;
  return hipHostFree(p);
}
hipError_t test_event_wait(hipEvent_t e) {
  g_log.push_back(Call{'W', (void*)e, nullptr, 0});
  if (!g_live.count((void*)e)) return hipErrorInvalidHandle;
  return g_fake ? hipSuccess : hipEventSynchronize(e);
}
hipError_t test_event_record(hipEvent_t e, hipStream_t s) {
  g_log.push_back(Call{'R', (void*)e, nullptr, 0});
  if (!g_live.count((void*)e)) return hipErrorInvalidHandle;
  return g_fake ? hipSuccess : hipEventRecord(e, s);
}
hipError_t test_copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t s) {
  g_log.push_back(Call{'C', nullptr, src, bytes});
  if (g_fake) return memcpy(dst, src, bytes), hipSuccess;
  return hipMemcpyAsync(dst, src, bytes, kind, s);
}
}  // namespace

// the header's calls into the runtime, through the counters above (hipMalloc / hipFree, which hip_mem.h's DevMem
// would make, are not used by anything under test here)
#define hipEventCreateWithFlags test_event_create
#define hipEventDestroy test_event_destroy
#define hipStreamCreateWithFlags test_stream_create
#define hipStreamDestroy test_stream_destroy
#define hipStreamEndCapture test_end_capture
#define hipGraphDestroy test_graph_destroy
#define hipGraphInstantiate test_instantiate
#define hipGraphExecDestroy test_exec_destroy
#define hipHostMalloc test_host_malloc
#define hipHostFree test_host_free
#define hipEventSynchronize test_event_wait
#define hipEventRecord test_event_record
#define hipMemcpyAsync test_copy
#include "../../ra-slam_amd/csrc/hip_handles.h"
#undef hipEventCreateWithFlags
#undef hipEventDestroy
#undef hipStreamCreateWithFlags
#undef hipStreamDestroy
#undef hipStreamEndCapture
#undef hipGraphDestroy
#undef hipGraphInstantiate
#undef hipGraphExecDestroy
#undef hipHostMalloc
#undef hipHostFree
#undef hipEventSynchronize
#undef hipEventRecord
#undef hipMemcpyAsync

static int g_failed = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);           \
      ++g_failed;                                                        \
    }                                                                    \
  } while (0)

using ratsdf::HipEvent;
using ratsdf::HipGraph;
using ratsdf::HipStream;
using ratsdf::TwinTable;

// one round of everything an event or stream owner does, whatever create answers; returns the creates that succeeded
template <class Owner>
static int exercise(const char* kind, unsigned flags) {
  using Handle = typename Owner::Handle;
  const int creates0 = g_creates, destroys0 = g_destroys;
  {
    Owner a;
    CHECK(!a && (Handle)a == nullptr);
    int st = a.create(flags);
    if (st == RATSDF_OK) {
      const Handle h = a;
      CHECK(h != nullptr);
      const int d = g_destroys;
      Owner b(std::move(a));  // moving does not destroy
      CHECK(g_destroys == d && (Handle)a == nullptr && (Handle)b == h);
      Owner c;
      c = std::move(b);
      CHECK(g_destroys == d && (Handle)b == nullptr && (Handle)c == h);
      Owner& same = c;
      c = std::move(same);  // self-assignment keeps the handle
      CHECK(g_destroys == d && (Handle)c == h);
      st = c.create(flags);  // creating over a live owner destroys what it held, once
      CHECK(g_destroys == d + 1);
      CHECK(st == RATSDF_OK ? (Handle)c != nullptr : (Handle)c == nullptr);
      Owner e;
      if (e.create(flags) == RATSDF_OK) {  // move-assigning over a live owner destroys what IT held, not what moves in
        const Handle q = e;
        const int d2 = g_destroys;
        c = std::move(e);
        CHECK(g_destroys == d2 + (st == RATSDF_OK ? 1 : 0) && (Handle)c == q && (Handle)e == nullptr);
      }
      c.reset();
      CHECK((Handle)c == nullptr);
      const int d3 = g_destroys;
      c.reset();  // (nothing left to destroy)
      CHECK(g_destroys == d3);
    } else {
      CHECK(st == RATSDF_ERR_DEVICE && (Handle)a == nullptr);
      Owner b(std::move(a));
      CHECK((Handle)a == nullptr && (Handle)b == nullptr);
    }
  }
  // every handle handed out was destroyed exactly once, by the time the owners are gone
  const int made = g_creates - creates0;
  CHECK(g_destroys - destroys0 == made);
  CHECK(g_live.empty() && g_bad_destroys == 0);
  printf("%s: %d create(s) succeeded, %d destroy(s)\n", kind, made, g_destroys - destroys0);
  return made;
}

// a failed create over a live owner leaves it empty (the stand-in only)
template <class Owner>
static void failure_after_success(unsigned flags) {
  g_fake_fails = false;
  Owner a;
  CHECK(a.create(flags) == RATSDF_OK && a);
  g_fake_fails = true;
  const int d = g_destroys;
  CHECK(a.create(flags) == RATSDF_ERR_DEVICE && !a && g_destroys == d + 1);
  g_fake_fails = false;
}

// the graph owner: against the runtime there is no capture to end, so that run takes the failure branch everywhere
static int exercise_graph(const char* kind) {
  const int creates0 = g_creates, destroys0 = g_destroys;
  {
    HipStream s;
    (void)s.create(hipStreamNonBlocking);
    HipGraph g;
    CHECK(!g && g.exec() == nullptr);
    CHECK(g.instantiate() == RATSDF_ERR_DEVICE && !g);  // (nothing captured)
    if (g.end_capture(s) == RATSDF_OK) {
      CHECK(!g);  // a graph, no executable yet
      if (g.instantiate() == RATSDF_OK) {
        const hipGraphExec_t x = g.exec();
        CHECK(g && x != nullptr);
        const int d = g_destroys;
        HipGraph h(std::move(g));
        CHECK(g_destroys == d && !g && g.exec() == nullptr && h.exec() == x);
        HipGraph& same = h;
        h = std::move(same);
        CHECK(g_destroys == d && h.exec() == x);
        HipGraph k;
        k = std::move(h);
        CHECK(g_destroys == d && k.exec() == x && !h);
        k.reset();  // the executable and the graph, once each
        CHECK(g_destroys == d + 2 && !k);
        k.reset();
        CHECK(g_destroys == d + 2);
      } else {
        CHECK(!g && g.exec() == nullptr);
      }
      if (g.end_capture(s) == RATSDF_OK && g.instantiate() == RATSDF_OK) {
        const int d = g_destroys;
        (void)g.end_capture(s);  // a second capture over a live owner: what it held goes first
        CHECK(g_destroys == d + 2);
      }
    } else {
      CHECK(!g && g.exec() == nullptr);
    }
  }
  const int made = g_creates - creates0;
  CHECK(g_destroys - destroys0 == made);
  CHECK(g_live.empty() && g_bad_destroys == 0);
  printf("%s: %d create(s) succeeded, %d destroy(s)\n", kind, made, g_destroys - destroys0);
  return made;
}

// the twin table: its order of calls, against whatever allocates; returns 1 when it could be grown
static int exercise_twin(const char* kind) {
  const int creates0 = g_creates, destroys0 = g_destroys;
  int grown = 0;
  {
    HipStream s;
    (void)s.create(hipStreamNonBlocking);
    // where the copies go: host memory for the stand-in (which copies at once), device memory for the runtime
    std::vector<unsigned char> host_dst(4096);
    ratsdf::DevMem dev_dst;
    unsigned char* const dst = g_fake || dev_dst.alloc(4096) != RATSDF_OK ? host_dst.data() : dev_dst.as<unsigned char>();
    struct Drain {  // (declared before the table: the stream is idle before the table's memory goes)
      hipStream_t s;
      ~Drain() {
        if (!g_fake && s) (void)hipStreamSynchronize(s);
      }
    } drain{s};
    TwinTable t;
    void* p = nullptr;
    CHECK(t.size() == 0 && t.acquire(&p) == RATSDF_ERR_DEVICE && p == nullptr);  // nothing to hand out
    if (t.grow(1024) == RATSDF_OK) {
      grown = 1;
      CHECK(t.size() >= 1024);
      const int c = g_creates;
      CHECK(t.grow(512) == RATSDF_OK && g_creates == c);  // (fits: nothing is allocated)
      void* side[4] = {};
      for (int turn = 0; turn < 4; ++turn) {
        const size_t at = g_log.size();
        CHECK(t.acquire(&side[turn]) == RATSDF_OK && side[turn] != nullptr);
        // the side's event is waited for, and only then is its memory handed out (acquire() has returned by now)
        CHECK(g_log.size() == at + 1 && g_log[at].what == 'W');
        memset(side[turn], 0x40 + turn, 1024);
        CHECK(t.copy(dst, 0, 256, s) == RATSDF_OK);
        CHECK(t.commit(dst + 256, 256, 768, s) == RATSDF_OK);
        // two copies out of THIS side, then the record of the event that the wait two turns on goes to
        CHECK(g_log.size() == at + 4);
        if (g_log.size() == at + 4) {
          CHECK(g_log[at + 1].what == 'C' && g_log[at + 1].src == side[turn] && g_log[at + 1].bytes == 256);
          CHECK(g_log[at + 2].what == 'C' && g_log[at + 2].src == (unsigned char*)side[turn] + 256 &&
                g_log[at + 2].bytes == 768);
          CHECK(g_log[at + 3].what == 'R' && g_log[at + 3].handle == g_log[at].handle);
        }
        if (g_fake) CHECK(host_dst[0] == 0x40 + turn && host_dst[1023] == 0x40 + turn);
      }
      CHECK(side[0] != side[1] && side[2] == side[0] && side[3] == side[1]);  // the sides alternate
      CHECK(t.copy(dst, 1000, 100, s) == RATSDF_ERR_DEVICE);  // (beyond the side: refused, nothing queued)
      const int st = t.grow(2048);  // a larger one replaces both sides; the events stay
      CHECK(st == RATSDF_OK ? t.size() >= 2048 : t.size() == 0);
    } else {
      CHECK(t.size() == 0 && t.acquire(&p) == RATSDF_ERR_DEVICE && p == nullptr);
    }
  }
  CHECK(g_destroys - destroys0 == g_creates - creates0);
  CHECK(g_live.empty() && g_bad_destroys == 0);
  printf("%s: %s, %d create(s), %d destroy(s)\n", kind, grown ? "grown" : "not grown", g_creates - creates0,
         g_destroys - destroys0);
  return grown;
}

// a grow that fails part of the way -- at every allocation or create it makes -- leaves size 0 and leaks nothing
static void twin_failed_grow() {
  for (int ok_first = 0; ok_first < 4; ++ok_first) {
    g_fail_after = ok_first;  // side 0, event 0, side 1, event 1
    TwinTable t;
    void* p = nullptr;
    CHECK(t.grow(1024) == RATSDF_ERR_DEVICE && t.size() == 0 && t.acquire(&p) == RATSDF_ERR_DEVICE);
    g_fail_after = -1;
    CHECK(t.grow(1024) == RATSDF_OK && t.size() >= 1024);  // ... and the next one goes through the allocations again
    g_fail_after = 0;
    CHECK(t.grow(4096) == RATSDF_ERR_DEVICE && t.size() == 0);  // a failure after a success: the old size is not kept
    g_fail_after = -1;
  }
  CHECK(g_live.empty() && g_bad_destroys == 0);
}

int main() {
  // 1. the runtime of this machine
  g_fake = false;
  const int real = exercise<HipEvent>("runtime, event", hipEventDisableTiming) +
                   exercise<HipStream>("runtime, stream", hipStreamNonBlocking);
  CHECK(exercise_graph("runtime, graph") <= 1);  // (at most the stream: no capture was begun)
  const int real_twin = exercise_twin("runtime, twin table");
  // 2. the stand-in: succeeding, refusing, and refusing after it has succeeded
  g_fake = true;
  g_fake_fails = false;
  CHECK(exercise<HipEvent>("stand-in, event", hipEventDisableTiming) == 3);
  CHECK(exercise<HipStream>("stand-in, stream", hipStreamNonBlocking) == 3);
  CHECK(exercise_graph("stand-in, graph") == 6);  // the stream; a graph and its executable, twice; a third graph
  CHECK(exercise_twin("stand-in, twin table") == 1);
  g_fake_fails = true;
  CHECK(exercise<HipEvent>("stand-in refusing, event", hipEventDisableTiming) == 0);
  CHECK(exercise<HipStream>("stand-in refusing, stream", hipStreamNonBlocking) == 0);
  CHECK(exercise_graph("stand-in refusing, graph") == 0);
  CHECK(exercise_twin("stand-in refusing, twin table") == 0);
  failure_after_success<HipEvent>(hipEventDisableTiming);
  failure_after_success<HipStream>(hipStreamNonBlocking);
  g_fake_fails = false;
  twin_failed_grow();
  CHECK(g_live.empty() && g_bad_destroys == 0);
  printf("runtime creates that succeeded: %d, twin table %s\n", real, real_twin ? "grown" : "not grown");
  printf(g_failed ? "hip_handles FAILED (%d)\n" : "hip_handles OK\n", g_failed);
  return g_failed ? 1 : 0;
}
