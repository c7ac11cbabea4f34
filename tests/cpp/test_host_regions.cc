// The regions through the C++ host layer (TSDFGrid::Regions, TSDFSystem::Regions) against one ABI library.
//   usage: test_host_regions <library.so> <symbol prefix> <case file> <output file>
// The case file (written by tests/test_host_regions.py): int32 H, W, ox, oy, oz, X, Y, Z, states; float32 fx, fy, cx,
// cy, qx, qy, qz, qw, tx, ty, tz, voxel size, truncation, max depth, occupied_below, min_prob; then rgb (H*W*3 u8),
// depth, ht, lt (H*W f32 each).
// One frame goes into a TSDFGrid and into a TSDFSystem (identity extrinsics); both label the box.  The output file
// gets, for the grid and then for the system: the number of regions (uint64), the labels, the table.
// A library without the entry points (the CPU oracle) must report RATSDF_ERR_NOT_IMPLEMENTED from both calls and
// hand back nothing; nothing is written then.
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

static void write_result(FILE* o, const std::vector<int32_t>& labels, const std::vector<ratsdf_region>& regions) {
  const uint64_t n = regions.size();
  CHECK(fwrite(&n, sizeof(n), 1, o) == 1);
  CHECK(fwrite(labels.data(), sizeof(int32_t), labels.size(), o) == labels.size());
  CHECK(fwrite(regions.data(), sizeof(ratsdf_region), regions.size(), o) == regions.size());
}

int main(int argc, char** argv) {
  CHECK(argc == 5);
  const Api& api = Api::Load(argv[1], argv[2]);
  FILE* f = fopen(argv[3], "rb");
  CHECK(f);
  int32_t hdr[9];
  float par[16];
  read_into(f, hdr, 9);
  read_into(f, par, 16);
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
  const ratsdf_regions_params params = {par[14], par[15], (uint32_t)hdr[8], 0u};
  const Image i_rgb{rgb.data(), H, W, kU8C3}, i_depth{depth.data(), H, W, kF32C1}, i_ht{ht.data(), H, W, kF32C1},
      i_lt{lt.data(), H, W, kF32C1};
  printf("backend %s\n", api.backend());

  std::vector<int32_t> la(3, 7), lb(5, 7);          // (what they hold is replaced, or dropped on a failure)
  std::vector<ratsdf_region> ra(2), rb(4);
  TSDFGrid grid(vs, trunc, 0, &api);
  CHECK(grid.last_status() == RATSDF_OK);
  grid.Integrate(i_rgb, i_depth, i_ht, i_lt, max_depth, K, pose);
  CHECK(grid.last_status() == RATSDF_OK);
  const int st_grid = grid.Regions(origin, dims, params, &la, &ra);

  int st_sys = RATSDF_OK;
  {
    TSDFSystem sys(vs, trunc, max_depth, K, SE3<float>::Identity(), 0, &api);
    sys.Integrate(pose, i_rgb, i_depth, i_ht, i_lt);
    sys.Flush();
    st_sys = sys.Regions(origin, dims, params, &lb, &rb);
    sys.terminate();
  }
  printf("status %d %d\n", st_grid, st_sys);
  if (!api.regions) {  // the oracle: not implemented, reported through both layers
    CHECK(st_grid == RATSDF_ERR_NOT_IMPLEMENTED && st_sys == RATSDF_ERR_NOT_IMPLEMENTED);
    CHECK(grid.last_status() == RATSDF_ERR_NOT_IMPLEMENTED);
    CHECK(la.empty() && lb.empty() && ra.empty() && rb.empty());
    printf("not implemented OK\n");
    return 0;
  }
  CHECK(st_grid == RATSDF_OK && st_sys == RATSDF_OK);
  CHECK(la.size() == n && lb.size() == n);
  // the table alone equals the table with labels; refusals hand back nothing
  std::vector<ratsdf_region> rc;
  CHECK(grid.Regions(origin, dims, params, nullptr, &rc) == RATSDF_OK);
  CHECK(rc.size() == ra.size() && (ra.empty() || !memcmp(rc.data(), ra.data(), ra.size() * sizeof(ratsdf_region))));
  const int32_t zero[3] = {8, 0, 8};
  std::vector<int32_t> lc(9, 1);
  CHECK(grid.Regions(origin, zero, params, &lc, &rc) == RATSDF_ERR_BAD_ARGUMENT && lc.empty() && rc.empty());
  ratsdf_regions_params bad = params;
  bad.states = 8u;
  CHECK(grid.Regions(origin, dims, bad, &lc, &rc) == RATSDF_ERR_BAD_ARGUMENT && lc.empty() && rc.empty());
  CHECK(grid.Regions(origin, dims, params, &lc, nullptr) == RATSDF_ERR_BAD_ARGUMENT);
  FILE* o = fopen(argv[4], "wb");
  CHECK(o);
  write_result(o, la, ra);
  write_result(o, lb, rb);
  fclose(o);
  printf("regions OK\n");
  return 0;
}
