// Point sampling through the C++ host layer (TSDFGrid::SamplePoints, TSDFSystem::Sample) against one ABI library.
//   usage: test_host_sample <library.so> <symbol prefix> <case file> <output file>
// The case file (written by tests/test_host_sample.py): int32 H, W, n; float32 fx, fy, cx, cy, qx, qy, qz, qw, tx,
// ty, tz, voxel size, truncation, max depth; then rgb (H*W*3 u8), depth, ht, lt (H*W f32 each), points (n*3 f32).
// One frame goes into a TSDFGrid and into a TSDFSystem (identity extrinsics); both sample the points.  The output file
// gets the grid's n records, then the system's.  A library without the entry points (the CPU oracle) must report
// RATSDF_ERR_NOT_IMPLEMENTED from both calls; nothing is written then.
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

int main(int argc, char** argv) {
  CHECK(argc == 5);
  const Api& api = Api::Load(argv[1], argv[2]);
  FILE* f = fopen(argv[3], "rb");
  CHECK(f);
  int32_t hdr[3];
  float par[14];
  read_into(f, hdr, 3);
  read_into(f, par, 14);
  const int H = hdr[0], W = hdr[1];
  const size_t n = (size_t)hdr[2];
  std::vector<uint8_t> rgb((size_t)H * W * 3);
  std::vector<float> depth((size_t)H * W), ht((size_t)H * W), lt((size_t)H * W), xyz(n * 3);
  read_into(f, rgb.data(), rgb.size());
  read_into(f, depth.data(), depth.size());
  read_into(f, ht.data(), ht.size());
  read_into(f, lt.data(), lt.size());
  read_into(f, xyz.data(), xyz.size());
  fclose(f);
  const CameraIntrinsics<float> K(par[0], par[1], par[2], par[3]);
  const SE3<float> pose(Quaternion<float>{par[4], par[5], par[6], par[7]}, Vector3<float>{par[8], par[9], par[10]});
  const float vs = par[11], trunc = par[12], max_depth = par[13];
  const Image i_rgb{rgb.data(), H, W, kU8C3}, i_depth{depth.data(), H, W, kF32C1}, i_ht{ht.data(), H, W, kF32C1},
      i_lt{lt.data(), H, W, kF32C1};
  printf("backend %s\n", api.backend());

  std::vector<ratsdf_sample> a(n), b(n);
  TSDFGrid grid(vs, trunc, 0, &api);
  CHECK(grid.last_status() == RATSDF_OK);
  grid.Integrate(i_rgb, i_depth, i_ht, i_lt, max_depth, K, pose);
  CHECK(grid.last_status() == RATSDF_OK);
  const int st_grid = grid.SamplePoints(xyz.data(), n, a.data());

  int st_sys = RATSDF_OK;
  {
    TSDFSystem sys(vs, trunc, max_depth, K, SE3<float>::Identity(), 0, &api);
    sys.Integrate(pose, i_rgb, i_depth, i_ht, i_lt);
    sys.Flush();
    st_sys = sys.Sample(xyz.data(), n, b.data());
    sys.terminate();
  }
  printf("status %d %d\n", st_grid, st_sys);
  if (!api.sample_points) {  // the oracle: not implemented, reported through both layers
    CHECK(st_grid == RATSDF_ERR_NOT_IMPLEMENTED && st_sys == RATSDF_ERR_NOT_IMPLEMENTED);
    CHECK(grid.last_status() == RATSDF_ERR_NOT_IMPLEMENTED);
    printf("not implemented OK\n");
    return 0;
  }
  CHECK(st_grid == RATSDF_OK && st_sys == RATSDF_OK);
  CHECK(grid.SamplePoints(xyz.data(), 0, nullptr) == RATSDF_OK);
  CHECK(grid.SamplePoints(nullptr, 1, a.data()) == RATSDF_ERR_BAD_ARGUMENT);
  FILE* o = fopen(argv[4], "wb");
  CHECK(o);
  CHECK(fwrite(a.data(), sizeof(ratsdf_sample), n, o) == n);
  CHECK(fwrite(b.data(), sizeof(ratsdf_sample), n, o) == n);
  fclose(o);
  printf("sampled OK\n");
  return 0;
}
