// test_hip_mem.cc -- the invariants of ra-slam_amd/csrc/hip_mem.h, for device and for page-locked host memory.
//
// Runs twice (tests/test_hip_mem.py): against the HIP runtime as it is on this machine -- without a GPU every
// allocation fails (no device) and the failure branch is what is exercised, on an MI355X the success branch -- and
// against a stand-in allocator that can be told to fail, so that both branches are checked on every machine.
// Every free that the owners make goes through a counter: a pointer is freed exactly once, never twice, none leaks.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>

namespace {
bool g_fake = false;       // the stand-in allocator instead of the runtime
bool g_fake_fails = false; // ... refusing
std::set<void*> g_live;    // what an owner has been given and has not freed yet
int g_frees = 0, g_bad_frees = 0;

hipError_t test_alloc(void** p, size_t bytes, bool pinned) {
  hipError_t err;
  if (g_fake) {
    *p = g_fake_fails ? nullptr : malloc(bytes);
    err = *p ? hipSuccess : hipErrorOutOfMemory;
  } else {
    err = pinned ? hipHostMalloc(p, bytes, hipHostMallocDefault) : hipMalloc(p, bytes);
  }
  if (err == hipSuccess && *p) g_live.insert(*p);
  return err;
}
hipError_t test_free(void* p, bool pinned) {
  ++g_frees;
  if (!g_live.erase(p)) ++g_bad_frees;  // never handed out, or freed before
  if (g_fake) {
    free(p);
    return hipSuccess;
  }
  return pinned ? hipHostFree(p) : hipFree(p);
}
hipError_t test_malloc(void** p, size_t bytes) { return test_alloc(p, bytes, false); }
hipError_t test_host_malloc(void** p, size_t bytes, unsigned) { return test_alloc(p, bytes, true); }
hipError_t test_dev_free(void* p) { return test_free(p, false); }
hipError_t test_host_free(void* p) { return test_free(p, true); }
}  // namespace

// hip_mem.h's four calls into the runtime, through the counters above
#define hipMalloc test_malloc
#define hipHostMalloc test_host_malloc
#define hipFree test_dev_free
#define hipHostFree test_host_free
#include "../../ra-slam_amd/csrc/hip_mem.h"
#undef hipMalloc
#undef hipHostMalloc
#undef hipFree
#undef hipHostFree

static int g_failed = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);           \
      ++g_failed;                                                        \
    }                                                                    \
  } while (0)

template <class Mem>
static bool empty(const Mem& m) {
  return !m && m.template as<void>() == nullptr && m.size() == 0;
}

// one round of everything, whatever the allocator answers; returns how many allocations succeeded
template <class Mem>
static int exercise(const char* kind) {
  int ok_calls = 0;
  const int frees0 = g_frees;
  {
    Mem a;
    CHECK(empty(a));
    int st = a.alloc(4096);
    if (st == RATSDF_OK) {
      ++ok_calls;
      CHECK(a && a.size() >= 4096);
      void* p = a.template as<void>();
      CHECK(a.grow(1024) == RATSDF_OK && a.template as<void>() == p && a.size() >= 4096);  // a smaller grow keeps it
      CHECK(a.grow(4096) == RATSDF_OK && a.template as<void>() == p);
      const int f = g_frees;
      Mem b(std::move(a));  // moving does not free
      CHECK(g_frees == f && empty(a) && b.template as<void>() == p && b.size() >= 4096);
      Mem c;
      c = std::move(b);
      CHECK(g_frees == f && empty(b) && c.template as<void>() == p);
      st = c.grow(8192);  // a larger one replaces it: the old piece is freed, once
      CHECK(g_frees == f + 1);
      if (st == RATSDF_OK) {
        ++ok_calls;
        CHECK(c && c.size() >= 8192);
      } else {
        CHECK(empty(c));
      }
      Mem d;
      if (d.alloc(2048) == RATSDF_OK) {  // move-assigning over a live owner frees what IT held, not what moves in
        ++ok_calls;
        void* q = d.template as<void>();
        const int f2 = g_frees;
        c = std::move(d);
        CHECK(g_frees == f2 + (st == RATSDF_OK ? 1 : 0) && c.template as<void>() == q && empty(d));
      }
      c.reset();
      CHECK(empty(c));
      const int f3 = g_frees;
      c.reset();  // (nothing left to free)
      CHECK(g_frees == f3);
    } else {
      CHECK(st == RATSDF_ERR_DEVICE);
      CHECK(empty(a));
      CHECK(a.grow(1024) == RATSDF_ERR_DEVICE && empty(a));  // an empty owner grows through the allocation again
      Mem b(std::move(a));
      CHECK(empty(a) && empty(b));
    }
  }
  // every piece handed out was freed exactly once, by the time the owners are gone
  CHECK(g_frees - frees0 == ok_calls);
  CHECK(g_live.empty() && g_bad_frees == 0);
  printf("%s: %d allocation(s) succeeded, %d free(s)\n", kind, ok_calls, g_frees - frees0);
  return ok_calls;
}

// a failure after a success: the owner must not keep the old size (the stand-in allocator only)
template <class Mem>
static void failure_after_success() {
  g_fake_fails = false;
  Mem a;
  CHECK(a.alloc(4096) == RATSDF_OK && a.size() == 4096);
  g_fake_fails = true;
  CHECK(a.grow(1024) == RATSDF_OK && a.size() == 4096);  // (fits: no allocation, so nothing can fail)
  const int f = g_frees;
  CHECK(a.grow(8192) == RATSDF_ERR_DEVICE && empty(a) && g_frees == f + 1);
  CHECK(a.alloc(16) == RATSDF_ERR_DEVICE && empty(a) && g_frees == f + 1);
  g_fake_fails = false;
  CHECK(a.grow(16) == RATSDF_OK && a.size() == 16);
}

int main() {
  using ratsdf::DevMem;
  using ratsdf::HostMem;
  // 1. the runtime of this machine
  g_fake = false;
  const int real = exercise<DevMem>("runtime, device") + exercise<HostMem>("runtime, page-locked");
  // 2. the stand-in allocator: succeeding, refusing, and refusing after it has succeeded
  g_fake = true;
  g_fake_fails = false;
  CHECK(exercise<DevMem>("stand-in, device") == 3);
  CHECK(exercise<HostMem>("stand-in, page-locked") == 3);
  g_fake_fails = true;
  CHECK(exercise<DevMem>("stand-in refusing, device") == 0);
  CHECK(exercise<HostMem>("stand-in refusing, page-locked") == 0);
  failure_after_success<DevMem>();
  failure_after_success<HostMem>();
  CHECK(g_live.empty() && g_bad_frees == 0);
  printf("runtime allocations that succeeded: %d\n", real);
  printf(g_failed ? "hip_mem FAILED (%d)\n" : "hip_mem OK\n", g_failed);
  return g_failed ? 1 : 0;
}
