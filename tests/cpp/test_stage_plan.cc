// The upload-ahead schedule of the host-image batch (ra-slam_amd/csrc/stage_plan.h), on the host alone.
//
// Sweep: every batch length n from 0 to 3 * kStageSlots + 5, every ring position `base` of the call's first frame in
// 0 .. kStageSlots - 1, and four kinds of batch: no frame packed; all packed and side by side; all packed, none
// adjacent; a fixed-seed mix of the three.  stage_schedule runs with callables that record instead of copying and
// launching.  For every case:
//   * every frame is uploaded exactly once, in ascending order
//   * the uploads of frames i and i + 1 both precede launch(i)
//   * when frame u is uploaded, frame u - kStageSlots has been launched (its "used" event exists before a copy stream
//     is told to wait for it)
//   * no run is longer than kUploadRun or than the upload was allowed, none crosses the ring's end, and every frame of
//     a run of more than one is packed and lies the right number of strides behind the first
//   * the trace equals, step for step, that of the loop as it stood inside ratsdf_integrate_batch before it moved into
//     the header, restated below without its lambdas
//   * a refused upload or launch, at every step of the trace in turn, ends the loop with that status and nothing
//     further is called
// ... and once more with an image smaller than the ring's stride, where no two frames go up together.
//
// usage: test_stage_plan        (prints "stage plan OK: ..." and returns 0, or names what failed)
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "stage_plan.h"

using namespace ratsdf;

static long g_failures = 0;
#define CHECK(cond, ...)                    \
  do {                                      \
    if (!(cond)) {                          \
      if (g_failures++ < 40) {              \
        printf("FAILED %s: ", #cond);       \
        printf(__VA_ARGS__);                \
        printf("\n");                       \
      }                                     \
    }                                       \
  } while (0)

// A batch: which frames are packed, and where each frame's block lies in host memory, in ring strides.
struct Batch {
  int n;
  uint64_t base;
  bool full_stride;  // the image has the ring's slot size
  std::vector<char> packed;
  std::vector<long> addr;
  bool is_packed(int i) const { return packed[(size_t)i] != 0; }
  bool adjacent(int i, int k) const { return full_stride && addr[(size_t)(i + k)] == addr[(size_t)i] + k; }
};

struct Step {
  char kind;  // 'U' upload, 'L' launch
  int first, max_run, took;
  bool operator==(const Step& o) const {
    return kind == o.kind && first == o.first && max_run == o.max_run && took == o.took;
  }
};
using Trace = std::vector<Step>;

// ---- the loop of ratsdf_integrate_batch as it stood before stage_plan.h, its lambdas written out ----
static void ref_upload(const Batch& b, int i, int max_run, int* took, Trace* out) {
  const int slot = (int)((b.base + (uint64_t)i) % kStageSlots);
  int run = 1;
  if (b.is_packed(i) && b.full_stride)
    while (run < max_run && i + run < b.n && slot + run < kStageSlots && b.is_packed(i + run) &&
           b.addr[(size_t)(i + run)] == b.addr[(size_t)i] + run)
      ++run;
  *took = run;
  out->push_back(Step{'U', i, max_run, run});
}
static Trace reference(const Batch& b) {
  Trace out;
  const int n = b.n;
  const int ahead = kStageSlots - 1;
  int uploaded = 0;
  for (int i = 0; i < n; ++i) {
    while (uploaded < n && uploaded <= i + 1) {
      int took = 0;
      ref_upload(b, uploaded, std::min(kUploadRun, i + ahead - uploaded + 1), &took, &out);
      uploaded += took;
    }
    out.push_back(Step{'L', i, 0, 0});
    while (uploaded < n) {
      const int want = std::min(kUploadRun, n - uploaded);
      if (uploaded + want - 1 > i + ahead) break;
      int took = 0;
      ref_upload(b, uploaded, want, &took, &out);
      uploaded += took;
    }
  }
  return out;
}

// ---- stage_schedule with recording callables; the call number `refuse_at` (if >= 0) is refused with `status` ----
static int record(const Batch& b, Trace* out, long refuse_at, int status) {
  long calls = 0;
  auto packed = [&](int i) { return b.is_packed(i); };
  auto adjacent = [&](int i, int k) { return b.adjacent(i, k); };
  auto upload = [&](int first, int max_run) {
    const bool refused = calls++ == refuse_at;
    const int run = stage_run_length(first, b.n, stage_slot_of(b.base, first), max_run, packed, adjacent);
    out->push_back(Step{'U', first, max_run, run});
    return refused ? StageTook{0, status} : StageTook{run, 0};
  };
  auto launch = [&](int i) {
    const bool refused = calls++ == refuse_at;
    out->push_back(Step{'L', i, 0, 0});
    return refused ? status : 0;
  };
  return stage_schedule(b.n, upload, launch);
}

#define AT "n %d base %d %s"
#define ARGS b.n, (int)b.base, name

static long check(const Batch& b, const char* name) {
  const long before = g_failures;
  Trace t;
  CHECK(record(b, &t, -1, 0) == 0, AT, ARGS);
  int uploaded = 0, launched = 0;
  for (const Step& s : t) {
    if (s.kind == 'U') {
      CHECK(s.first == uploaded, "frame %d goes up where %d is due; " AT, s.first, uploaded, ARGS);
      CHECK(s.took >= 1 && s.took <= kUploadRun && s.took <= s.max_run && s.first + s.took <= b.n,
            "a run of %d at frame %d (allowed %d); " AT, s.took, s.first, s.max_run, ARGS);
      const int slot = stage_slot_of(b.base, s.first);
      CHECK(slot + s.took <= kStageSlots, "the run of %d at frame %d (slot %d) crosses the ring's end; " AT, s.took,
            s.first, slot, ARGS);
      for (int k = 0; k < s.took; ++k) {
        const int u = s.first + k;
        CHECK(stage_slot_of(b.base, u) == slot + k, "frame %d: slot; " AT, u, ARGS);
        CHECK(u - kStageSlots < launched, "frame %d goes up before frame %d has been launched; " AT, u, u - kStageSlots,
              ARGS);
        if (s.took > 1)
          CHECK(b.is_packed(u) && (k == 0 || b.adjacent(s.first, k)), "frame %d in a run of %d; " AT, u, s.took, ARGS);
      }
      uploaded += s.took;
    } else {
      CHECK(s.first == launched, "launch %d where %d is due; " AT, s.first, launched, ARGS);
      CHECK(uploaded >= std::min(b.n, s.first + 2), "launch %d with %d frames uploaded; " AT, s.first, uploaded, ARGS);
      ++launched;
    }
  }
  CHECK(uploaded == b.n && launched == b.n, "%d uploaded, %d launched; " AT, uploaded, launched, ARGS);
  const Trace ref = reference(b);
  CHECK(t == ref, "the trace (%zu steps) differs from the earlier loop's (%zu steps); " AT, t.size(), ref.size(), ARGS);
  return g_failures - before;
}

// every call of the trace refused in turn: the status comes back and the trace ends with the refused call
static long check_refusals(const Batch& b, const char* name) {
  Trace whole;
  (void)record(b, &whole, -1, 0);
  long refusals = 0;
  for (size_t k = 0; k < whole.size(); ++k, ++refusals) {
    Trace t;
    const int status = 2 + (int)(k % 5);
    const int st = record(b, &t, (long)k, status);
    CHECK(st == status, "refusal at step %zu: status %d came back as %d; " AT, k, status, st, ARGS);
    CHECK(t.size() == k + 1 && std::equal(t.begin(), t.end(), whole.begin()),
          "refusal at step %zu: %zu steps were made; " AT, k, t.size(), ARGS);
  }
  return refusals;
}

static uint32_t g_rng = 0x2545F491u;
static uint32_t rnd() {  // xorshift32, fixed seed
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 17;
  g_rng ^= g_rng << 5;
  return g_rng;
}

static Batch make(int n, int base, int kind, bool full_stride) {
  Batch b{n, (uint64_t)base, full_stride, std::vector<char>((size_t)n), std::vector<long>((size_t)n)};
  long at = 1000;
  int left = 0, cur = 0;  // (the mix: frames left of the current stretch, and its kind)
  for (int i = 0; i < n; ++i) {
    bool packed = false, next_to_last = false;
    switch (kind) {
      case 0: next_to_last = true; break;                 // not packed (wherever the frames lie)
      case 1: packed = next_to_last = true; break;        // packed and side by side
      case 2: packed = true; break;                       // packed, not adjacent
      default: {                                          // a mix, in stretches of 1 .. 8 frames
        if (!left) {
          left = 1 + (int)(rnd() % 8);
          cur = (int)(rnd() % 3);
        }
        --left;
        packed = cur != 0;
        next_to_last = cur != 2;
      }
    }
    at += next_to_last ? 1 : 3;
    b.packed[(size_t)i] = packed;
    b.addr[(size_t)i] = at;
  }
  return b;
}

int main() {
  const char* names[] = {"none packed", "packed side by side", "packed apart", "mixed"};
  long cases = 0, refusals = 0, runs = 0;
  for (int n = 0; n <= 3 * kStageSlots + 5; ++n)
    for (int base = 0; base < kStageSlots; ++base)
      for (int kind = 0; kind < 4; ++kind) {
        const Batch b = make(n, base, kind, true);
        check(b, names[kind]);
        refusals += check_refusals(b, names[kind]);
        ++cases;
        Trace t;
        (void)record(b, &t, -1, 0);
        for (const Step& s : t) runs += s.kind == 'U' && s.took > 1;
      }
  // the sweep has met what it is about: runs of several frames, and runs cut short
  CHECK(runs > 1000, "%ld runs of more than one frame", runs);
  // an image smaller than the ring's slots: packed frames of such a call never lie at the ring's stride
  for (int base = 0; base < kStageSlots; ++base) {
    const Batch b = make(2 * kStageSlots + 3, base, 1, false);
    check(b, "smaller image");
    Trace t;
    (void)record(b, &t, -1, 0);
    for (const Step& s : t) CHECK(s.kind != 'U' || s.took == 1, "a run of %d with a smaller image", s.took);
  }
  if (g_failures) {
    printf("%ld checks failed\n", g_failures);
    return 1;
  }
  printf("stage plan OK: %ld cases, %ld refusals, %ld runs of more than one frame\n", cases, refusals, runs);
  return 0;
}
