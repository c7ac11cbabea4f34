// The ESDF through the C++ host layer (TSDFGrid::ESDF, TSDFSystem::ESDF) against one ABI library.
//   usage: test_host_esdf <library.so> <symbol prefix> <case file> <output file>
// The case file (written by tests/test_host_esdf.py): int32 H, W, ox, oy, oz, X, Y, Z; float32 fx, fy, cx, cy, qx, qy,
// qz, qw, tx, ty, tz, voxel size, truncation, max depth; then rgb (H*W*3 u8), depth, ht, lt (H*W f32 each).
// One frame goes into a TSDFGrid and into a TSDFSystem (identity extrinsics); both compute the field of the box with
// unknown voxels counted as obstacles.  The output file gets the grid's field, its states, then the system's field.
// A library without the entry points (the CPU oracle) must report RATSDF_ERR_NOT_IMPLEMENTED from both calls;
// nothing is written then.
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
  int32_t hdr[8];
  float par[14];
  read_into(f, hdr, 8);
  read_into(f, par, 14);
  const int H = hdr[0], W = hdr[1];
  const int32_t origin[3] = {hdr[2], hdr[3], hdr[4]}, dims[3] = {hdr[5], hdr[6], hdr[7]};
  const size_t n = (size_t)dims[0] * dims[1] * dims[2];
  std::vector<uint8_t> rgb((size_t)H * W * 3);
  std::vector<float> depth((size_t)H * W), ht((size_t)H * W), lt((size_t)H * W);
  read_into(f, rgb.data(), rgb.size());
  read_into(f, depth.data(), depth.size());
  read_into(f, ht.data(), ht.size());
  read_into(f, lt.data(), lt.size());
  fclose(f);
  const CameraIntrinsics<float> K(par[0], par[1], par[2], par[3]);
  const SE3<float> pose(Quaternion<float>{par[4], par[5], par[6], par[7]}, Vector3<float>{par[8], par[9], par[10]});
  const float vs = par[11], trunc = par[12], max_depth = par[13];
  const Image i_rgb{rgb.data(), H, W, kU8C3}, i_depth{depth.data(), H, W, kF32C1}, i_ht{ht.data(), H, W, kF32C1},
      i_lt{lt.data(), H, W, kF32C1};
  printf("backend %s\n", api.backend());

  std::vector<float> a(n), b(n);
  std::vector<uint8_t> sa(n);
  TSDFGrid grid(vs, trunc, 0, &api);
  CHECK(grid.last_status() == RATSDF_OK);
  grid.Integrate(i_rgb, i_depth, i_ht, i_lt, max_depth, K, pose);
  CHECK(grid.last_status() == RATSDF_OK);
  const int st_grid = grid.ESDF(origin, dims, 0.f, RATSDF_ESDF_UNKNOWN_OCCUPIED, a.data(), sa.data());

  int st_sys = RATSDF_OK;
  {
    TSDFSystem sys(vs, trunc, max_depth, K, SE3<float>::Identity(), 0, &api);
    sys.Integrate(pose, i_rgb, i_depth, i_ht, i_lt);
    sys.Flush();
    st_sys = sys.ESDF(origin, dims, 0.f, RATSDF_ESDF_UNKNOWN_OCCUPIED, b.data());
    sys.terminate();
  }
  printf("status %d %d\n", st_grid, st_sys);
  if (!api.esdf) {  // the oracle: not implemented, reported through both layers
    CHECK(st_grid == RATSDF_ERR_NOT_IMPLEMENTED && st_sys == RATSDF_ERR_NOT_IMPLEMENTED);
    CHECK(grid.last_status() == RATSDF_ERR_NOT_IMPLEMENTED);
    printf("not implemented OK\n");
    return 0;
  }
  CHECK(st_grid == RATSDF_OK && st_sys == RATSDF_OK);
  const int32_t zero[3] = {8, 0, 8};
  CHECK(grid.ESDF(origin, zero, 0.f, 0, a.data()) == RATSDF_ERR_BAD_ARGUMENT);
  CHECK(grid.ESDF(origin, dims, 0.f, 0, nullptr) == RATSDF_ERR_BAD_ARGUMENT);
  FILE* o = fopen(argv[4], "wb");
  CHECK(o);
  CHECK(fwrite(a.data(), sizeof(float), n, o) == n);
  CHECK(fwrite(sa.data(), 1, n, o) == n);
  CHECK(fwrite(b.data(), sizeof(float), n, o) == n);
  fclose(o);
  printf("esdf OK\n");
  return 0;
}
