// Map coarsening through the C++ host layer (TSDFGrid::FuseMapCoarsened, TSDFSystem::FuseMapCoarsened,
// TSDFSystem::CoarsenInto) against one ABI library.
//   usage: test_host_coarsen <library.so> <symbol prefix> <case file> <output stem>
// The case file is the one of test_host_fuse (tests/test_host_fuse.py: make_case): frames A, frames B, voxel size vs.
//   grid:   A in a TSDFGrid of vs, coarsened into an empty TSDFGrid of 2 vs, saved to <stem>_grid.map
//   system: a TSDFSystem of 2 vs is handed B's frames and, while its worker still has them queued,
//           FuseMapCoarsened(A's grid): the call drains the queue first; saved to <stem>_system.map
//   into:   a TSDFSystem of vs is handed A's frames and, with the queue full, CoarsenInto(an empty TSDFGrid of 2 vs):
//           the same map as `grid`; saved to <stem>_into.map
// A library without the entry point (the CPU oracle) must report RATSDF_ERR_NOT_IMPLEMENTED through both layers and
// write nothing.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ratsdf/tsdf_system.hpp"

using namespace ratsdf;

#define CHECK(cond)                                                       \
  do {                                                                    \
    if (!(cond)) {                                                        \
      fprintf(stderr, "CHECK failed at line %d: %s\n", __LINE__, #cond);  \
      exit(1);                                                            \
    }                                                                     \
  } while (0)

template <class T>
static void read_into(FILE* f, T* p, size_t n) {
  CHECK(fread(p, sizeof(T), n, f) == n);
}

struct FrameData {
  float par[11];
  std::vector<uint8_t> rgb;
  std::vector<float> depth, ht, lt;
};

static void print_stats(const ratsdf_fuse_stats& s) {
  printf("stats %lld %lld %lld %lld %lld\n", (long long)s.blocks_seen, (long long)s.blocks_allocated,
         (long long)s.blocks_skipped, (long long)s.voxels_copied, (long long)s.voxels_averaged);
}

int main(int argc, char** argv) {
  CHECK(argc == 5);
  const Api& api = Api::Load(argv[1], argv[2]);
  const std::string stem = argv[4];
  FILE* f = fopen(argv[3], "rb");
  CHECK(f);
  int32_t hdr[4];
  float cfg[3];
  read_into(f, hdr, 4);
  read_into(f, cfg, 3);
  const int H = hdr[0], W = hdr[1], nA = hdr[2], nB = hdr[3];
  const float vs = cfg[0], trunc = cfg[1], max_depth = cfg[2];
  const float vs2 = 2.0f * vs;
  std::vector<FrameData> frames((size_t)(nA + nB));
  for (FrameData& fr : frames) {
    read_into(f, fr.par, 11);
    fr.rgb.resize((size_t)H * W * 3);
    fr.depth.resize((size_t)H * W);
    fr.ht.resize((size_t)H * W);
    fr.lt.resize((size_t)H * W);
    read_into(f, fr.rgb.data(), fr.rgb.size());
    read_into(f, fr.depth.data(), fr.depth.size());
    read_into(f, fr.ht.data(), fr.ht.size());
    read_into(f, fr.lt.data(), fr.lt.size());
  }
  fclose(f);
  printf("backend %s\n", api.backend());
  auto K_of = [](const FrameData& fr) { return CameraIntrinsics<float>(fr.par[0], fr.par[1], fr.par[2], fr.par[3]); };
  auto pose_of = [](const FrameData& fr) {
    return SE3<float>(Quaternion<float>{fr.par[4], fr.par[5], fr.par[6], fr.par[7]},
                      Vector3<float>{fr.par[8], fr.par[9], fr.par[10]});
  };
  auto queue = [&](TSDFSystem& sys, int lo, int hi) {
    for (int i = lo; i < hi; ++i) {
      const FrameData& fr = frames[(size_t)i];
      sys.Integrate(pose_of(fr), Image{fr.rgb.data(), H, W, kU8C3}, Image{fr.depth.data(), H, W, kF32C1},
                    Image{fr.ht.data(), H, W, kF32C1}, Image{fr.lt.data(), H, W, kF32C1});
    }
  };

  TSDFGrid a(vs, trunc, 0, &api), c(vs2, trunc, 0, &api);
  CHECK(a.last_status() == RATSDF_OK && c.last_status() == RATSDF_OK);
  for (int i = 0; i < nA; ++i) {
    const FrameData& fr = frames[(size_t)i];
    a.Integrate(Image{fr.rgb.data(), H, W, kU8C3}, Image{fr.depth.data(), H, W, kF32C1},
                Image{fr.ht.data(), H, W, kF32C1}, Image{fr.lt.data(), H, W, kF32C1}, max_depth, K_of(fr), pose_of(fr));
    CHECK(a.last_status() == RATSDF_OK);
  }
  ratsdf_fuse_stats s_grid, s_sys, s_into;
  memset(&s_grid, 0xFF, sizeof(s_grid));
  s_sys = s_into = s_grid;
  const int st_grid = c.FuseMapCoarsened(a, &s_grid);
  int st_sys = RATSDF_OK, st_into = RATSDF_OK;
  {
    TSDFSystem sys(vs2, trunc, max_depth, K_of(frames[0]), SE3<float>::Identity(), 0, &api);
    queue(sys, nA, nA + nB);
    st_sys = sys.FuseMapCoarsened(a, &s_sys);  // (no Flush here: the worker still has frames queued)
    if (st_sys == RATSDF_OK) CHECK(sys.SaveMap(stem + "_system.map") == RATSDF_OK);
    sys.terminate();
  }
  {
    TSDFGrid c2(vs2, trunc, 0, &api);
    CHECK(c2.last_status() == RATSDF_OK);
    TSDFSystem sys(vs, trunc, max_depth, K_of(frames[0]), SE3<float>::Identity(), 0, &api);
    queue(sys, 0, nA);
    st_into = sys.CoarsenInto(c2, &s_into);
    if (st_into == RATSDF_OK) CHECK(c2.SaveMap(stem + "_into.map") == RATSDF_OK);
    sys.terminate();
  }
  printf("status %d %d %d\n", st_grid, st_sys, st_into);
  if (!api.fuse_map_coarsened) {  // the oracle: not implemented, reported through both layers, nothing written
    CHECK(st_grid == RATSDF_ERR_NOT_IMPLEMENTED && st_sys == RATSDF_ERR_NOT_IMPLEMENTED &&
          st_into == RATSDF_ERR_NOT_IMPLEMENTED);
    CHECK(c.last_status() == RATSDF_ERR_NOT_IMPLEMENTED);
    for (const ratsdf_fuse_stats* s : {&s_grid, &s_sys, &s_into})
      CHECK(s->blocks_seen == -1 && s->voxels_averaged == -1);  // (the statistics were not written either)
    printf("not implemented OK\n");
    return 0;
  }
  CHECK(st_grid == RATSDF_OK && st_sys == RATSDF_OK && st_into == RATSDF_OK);
  CHECK(c.SaveMap(stem + "_grid.map") == RATSDF_OK);
  print_stats(s_grid);
  print_stats(s_sys);
  print_stats(s_into);
  // refusals reach the caller
  CHECK(c.FuseMapCoarsened(c) == RATSDF_ERR_BAD_ARGUMENT);
  CHECK(a.FuseMapCoarsened(c) == RATSDF_ERR_BAD_ARGUMENT);  // (the wrong way round: a is the finer one)
  CHECK(a.last_status() == RATSDF_ERR_BAD_ARGUMENT);
  printf("coarsened OK\n");
  return 0;
}
