// stage_plan.h -- the upload-ahead schedule of the host-image batch (ratsdf_integrate_batch) as plain C++: no HIP
// types, so tests/cpp/test_stage_plan.cc runs it on the host alone, with recording callables in place of the copies
// and the launches.
//
// The staging ring has kStageSlots slots; frame i of a call that starts at ring position `base` (frames counted over
// every host-image call of the engine) takes slot (base + i) % kStageSlots.  Uploads run ahead of the frames that read
// them.  What the schedule guarantees:
//   * every frame is uploaded once, in ascending order;
//   * the uploads of frames i and i + 1 precede the launches of frame i (which host the look-ahead pass of i + 1);
//   * when frame u is uploaded, frame u - kStageSlots -- the last reader of u's slot -- has been launched: its "used"
//     event has been RECORDED before a copy stream is told to wait for it;
//   * an upload takes up to kUploadRun frames with ONE copy when they are packed blocks that lie side by side at the
//     ring's stride, and such a run never crosses the ring's end (its slots are contiguous).
#pragma once
#include <cstdint>

namespace ratsdf {

constexpr int kStageSlots = 16;  // frames of the host-image entry points in flight (uploads run ahead)
constexpr int kUploadRun = 4;    // frames that go up with one copy when they lie side by side in page-locked memory

inline int stage_slot_of(uint64_t base, int i) { return (int)((base + (uint64_t)i) % kStageSlots); }

// Frames that one upload starting at frame i of n takes, i in slot `slot`: 1, or up to max_run when frame i is packed
// (page-locked, semantic, its four images in the slot's own order), and so is every further frame i + k, which must
// also lie k ring strides behind frame i in host memory (`adjacent(i, k)`) and in a slot of the same lap of the ring.
template <class Packed, class Adjacent>
int stage_run_length(int i, int n, int slot, int max_run, Packed&& packed, Adjacent&& adjacent) {
  int run = 1;
  if (packed(i))
    while (run < max_run && i + run < n && slot + run < kStageSlots && packed(i + run) && adjacent(i, run)) ++run;
  return run;
}

struct StageTook {
  int frames, status;  // frames an upload took (>= 1) when status is 0
};

// The batch loop.  `upload(first, max_run)` uploads frames [first, first + frames), frames <= max_run, and returns
// StageTook; `launch(i)` makes the engine's stream wait for the uploads of frames i and i + 1, launches frame i and
// records its "used" event, and returns a status.  The first status that is not 0 ends the loop and is returned.
template <class Upload, class Launch>
int stage_schedule(int n, Upload&& upload, Launch&& launch) {
  // Uploads are enqueued up to `ahead` frames in front of the frame being launched: slot (u % kStageSlots) was last
  // read by frame u - kStageSlots, whose use_ev must have been RECORDED (i.e. that frame launched) before a copy
  // stream is told to wait for it.
  const int ahead = kStageSlots - 1;
  int uploaded = 0;
  for (int i = 0; i < n; ++i) {
    // frame i's launches host the look-ahead of frame i+1: both uploads precede them
    while (uploaded < n && uploaded <= i + 1) {
      const int room = i + ahead - uploaded + 1;
      const StageTook t = upload(uploaded, kUploadRun < room ? kUploadRun : room);
      if (t.status != 0) return t.status;
      uploaded += t.frames;
    }
    const int st = launch(i);
    if (st != 0) return st;
    // run further ahead with the uploads while the queue is busy -- in whole runs (or the batch's tail), so that
    // side-by-side frames keep going up together instead of one by one as slots fall free
    while (uploaded < n) {
      const int want = kUploadRun < n - uploaded ? kUploadRun : n - uploaded;
      if (uploaded + want - 1 > i + ahead) break;
      const StageTook t = upload(uploaded, want);
      if (t.status != 0) return t.status;
      uploaded += t.frames;
    }
  }
  return 0;
}

}  // namespace ratsdf
