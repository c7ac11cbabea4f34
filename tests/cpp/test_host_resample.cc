// Transformed map fusion through the C++ host layer (TSDFGrid::FuseMapTransformed, TSDFSystem::FuseMapTransformed)
// against one ABI library.
//   usage: test_host_resample <library.so> <symbol prefix> <case file> <output stem> qx qy qz qw tx ty tz
// The case file is the one of test_host_fuse (tests/test_host_fuse.py: make_case); the pose is dst_T_src, map A <- map B.
//   grid:   A and B in two TSDFGrids, A.FuseMapTransformed(B, pose), A saved to <stem>_grid.map
//   system: a TSDFSystem is handed A's frames and, while its worker still has them queued, FuseMapTransformed(B, pose):
//           the call drains the queue first, so the result is the same; saved to <stem>_system.map
// A library without the entry point (the CPU oracle) must report RATSDF_ERR_NOT_IMPLEMENTED through both layers.
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

int main(int argc, char** argv) {
  CHECK(argc == 12);
  const Api& api = Api::Load(argv[1], argv[2]);
  const std::string stem = argv[4];
  ratsdf_pose pose;
  {
    float v[7];
    for (int i = 0; i < 7; ++i) v[i] = strtof(argv[5 + i], nullptr);
    pose = ratsdf_pose{v[0], v[1], v[2], v[3], v[4], v[5], v[6]};
  }
  FILE* f = fopen(argv[3], "rb");
  CHECK(f);
  int32_t hdr[4];
  float cfg[3];
  read_into(f, hdr, 4);
  read_into(f, cfg, 3);
  const int H = hdr[0], W = hdr[1], nA = hdr[2], nB = hdr[3];
  const float vs = cfg[0], trunc = cfg[1], max_depth = cfg[2];
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
  auto integrate = [&](TSDFGrid& g, int lo, int hi) {
    for (int i = lo; i < hi; ++i) {
      const FrameData& fr = frames[(size_t)i];
      g.Integrate(Image{fr.rgb.data(), H, W, kU8C3}, Image{fr.depth.data(), H, W, kF32C1},
                  Image{fr.ht.data(), H, W, kF32C1}, Image{fr.lt.data(), H, W, kF32C1}, max_depth, K_of(fr), pose_of(fr));
      CHECK(g.last_status() == RATSDF_OK);
    }
  };

  TSDFGrid a(vs, trunc, 0, &api), b(vs, trunc, 0, &api);
  CHECK(a.last_status() == RATSDF_OK && b.last_status() == RATSDF_OK);
  integrate(a, 0, nA);
  integrate(b, nA, nA + nB);
  ratsdf_fuse_stats s_grid, s_sys;
  memset(&s_grid, 0, sizeof(s_grid));
  s_sys = s_grid;
  const int st_grid = a.FuseMapTransformed(b, pose, &s_grid);
  int st_sys = RATSDF_OK;
  {
    TSDFSystem sys(vs, trunc, max_depth, K_of(frames[0]), SE3<float>::Identity(), 0, &api);
    for (int i = 0; i < nA; ++i) {
      const FrameData& fr = frames[(size_t)i];
      sys.Integrate(pose_of(fr), Image{fr.rgb.data(), H, W, kU8C3}, Image{fr.depth.data(), H, W, kF32C1},
                    Image{fr.ht.data(), H, W, kF32C1}, Image{fr.lt.data(), H, W, kF32C1});
    }
    st_sys = sys.FuseMapTransformed(b, pose, &s_sys);  // (no Flush here: the worker still has frames queued)
    if (st_sys == RATSDF_OK) CHECK(sys.SaveMap(stem + "_system.map") == RATSDF_OK);
    sys.terminate();
  }
  printf("status %d %d\n", st_grid, st_sys);
  if (!api.fuse_map_transformed) {  // the oracle: not implemented, reported through both layers
    CHECK(st_grid == RATSDF_ERR_NOT_IMPLEMENTED && st_sys == RATSDF_ERR_NOT_IMPLEMENTED);
    CHECK(a.last_status() == RATSDF_ERR_NOT_IMPLEMENTED);
    printf("not implemented OK\n");
    return 0;
  }
  CHECK(st_grid == RATSDF_OK && st_sys == RATSDF_OK);
  CHECK(a.SaveMap(stem + "_grid.map") == RATSDF_OK);
  for (const ratsdf_fuse_stats* s : {&s_grid, &s_sys})
    printf("stats %lld %lld %lld %lld %lld\n", (long long)s->blocks_seen, (long long)s->blocks_allocated,
           (long long)s->blocks_skipped, (long long)s->voxels_copied, (long long)s->voxels_averaged);
  // refusals reach the caller
  CHECK(a.FuseMapTransformed(a, pose) == RATSDF_ERR_BAD_ARGUMENT);
  CHECK(a.FuseMapTransformed(b, ratsdf_pose{0, 0, 0, 0, 0, 0, 0}) == RATSDF_ERR_BAD_ARGUMENT);
  CHECK(a.last_status() == RATSDF_ERR_BAD_ARGUMENT);
  printf("fused OK\n");
  return 0;
}
