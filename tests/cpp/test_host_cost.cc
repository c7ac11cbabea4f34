// The cost-to-go field through the C++ host layer (TSDFGrid::CostToGo, TSDFSystem::CostToGo) against one ABI library.
//   usage: test_host_cost <library.so> <symbol prefix> <case file> <output file>
// The case file (written by tests/test_host_cost.py): int32 H, W, ox, oy, oz, X, Y, Z, flags, n_goals; float32 fx, fy,
// cx, cy, qx, qy, qz, qw, tx, ty, tz, voxel size, truncation, max depth, occupied_below, clearance; then rgb (H*W*3 u8),
// depth, ht, lt (H*W f32 each); then the goals (n_goals int32 triples).
// One frame goes into a TSDFGrid and into a TSDFSystem (identity extrinsics); both compute the field of the box.  The
// output file gets, for the grid and then for the system: the summary with `rounds` zeroed, the cost words, the
// direction bytes.
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

static void write_result(FILE* o, ratsdf_cost_summary s, const std::vector<uint32_t>& cost,
                         const std::vector<uint8_t>& next) {
  CHECK(s.rounds >= 1 && s.pending == 0);
  s.rounds = 0;  // (how many rounds it took is not part of the contract)
  CHECK(fwrite(&s, sizeof(s), 1, o) == 1);
  CHECK(fwrite(cost.data(), sizeof(uint32_t), cost.size(), o) == cost.size());
  CHECK(fwrite(next.data(), 1, next.size(), o) == next.size());
}

int main(int argc, char** argv) {
  CHECK(argc == 5);
  const Api& api = Api::Load(argv[1], argv[2]);
  FILE* f = fopen(argv[3], "rb");
  CHECK(f);
  int32_t hdr[10];
  float par[16];
  read_into(f, hdr, 10);
  read_into(f, par, 16);
  const int H = hdr[0], W = hdr[1];
  const int32_t origin[3] = {hdr[2], hdr[3], hdr[4]}, dims[3] = {hdr[5], hdr[6], hdr[7]};
  const int32_t n_goals = hdr[9];
  const size_t n = (size_t)dims[0] * dims[1] * dims[2];
  std::vector<uint8_t> rgb((size_t)H * W * 3);
  std::vector<float> depth((size_t)H * W), ht((size_t)H * W), lt((size_t)H * W);
  std::vector<int32_t> goals((size_t)n_goals * 3);
  read_into(f, rgb.data(), rgb.size());
  read_into(f, depth.data(), depth.size());
  read_into(f, ht.data(), ht.size());
  read_into(f, lt.data(), lt.size());
  read_into(f, goals.data(), goals.size());
  fclose(f);
  const CameraIntrinsics<float> K(par[0], par[1], par[2], par[3]);
  const SE3<float> pose(Quaternion<float>{par[4], par[5], par[6], par[7]}, Vector3<float>{par[8], par[9], par[10]});
  const float vs = par[11], trunc = par[12], max_depth = par[13];
  const ratsdf_cost_params params = {par[14], par[15], (uint32_t)hdr[8], 0};
  const Image i_rgb{rgb.data(), H, W, kU8C3}, i_depth{depth.data(), H, W, kF32C1}, i_ht{ht.data(), H, W, kF32C1},
      i_lt{lt.data(), H, W, kF32C1};
  printf("backend %s\n", api.backend());

  std::vector<uint32_t> ca(3, 7), cb(5, 7);          // (what they hold is replaced, or dropped on a failure)
  std::vector<uint8_t> na(2, 1), nb(4, 1);
  ratsdf_cost_summary sa, sb;
  memset(&sa, 0x5A, sizeof(sa));
  memset(&sb, 0x5A, sizeof(sb));
  TSDFGrid grid(vs, trunc, 0, &api);
  CHECK(grid.last_status() == RATSDF_OK);
  grid.Integrate(i_rgb, i_depth, i_ht, i_lt, max_depth, K, pose);
  CHECK(grid.last_status() == RATSDF_OK);
  const int st_grid = grid.CostToGo(origin, dims, params, goals.data(), n_goals, &ca, &na, &sa);

  int st_sys = RATSDF_OK;
  {
    TSDFSystem sys(vs, trunc, max_depth, K, SE3<float>::Identity(), 0, &api);
    sys.Integrate(pose, i_rgb, i_depth, i_ht, i_lt);
    sys.Flush();
    st_sys = sys.CostToGo(origin, dims, params, goals.data(), n_goals, &cb, &nb, &sb);
    sys.terminate();
  }
  printf("status %d %d\n", st_grid, st_sys);
  if (!api.cost_to_go) {  // the oracle: not implemented, reported through both layers
    CHECK(st_grid == RATSDF_ERR_NOT_IMPLEMENTED && st_sys == RATSDF_ERR_NOT_IMPLEMENTED);
    CHECK(grid.last_status() == RATSDF_ERR_NOT_IMPLEMENTED);
    CHECK(ca.empty() && cb.empty() && na.empty() && nb.empty());
    CHECK(sa.goals == 0x5A5A5A5A && sb.goals == 0x5A5A5A5A);
    printf("not implemented OK\n");
    return 0;
  }
  CHECK(st_grid == RATSDF_OK && st_sys == RATSDF_OK);
  CHECK(ca.size() == n && cb.size() == n && na.size() == n && nb.size() == n);
  // the cost alone equals the cost with the moves; refusals hand back nothing
  std::vector<uint32_t> cc;
  CHECK(grid.CostToGo(origin, dims, params, goals.data(), n_goals, &cc, nullptr, nullptr) == RATSDF_OK);
  CHECK(cc.size() == n && !memcmp(cc.data(), ca.data(), n * sizeof(uint32_t)));
  const int32_t zero[3] = {8, 0, 8};
  std::vector<uint8_t> nc(9, 1);
  CHECK(grid.CostToGo(origin, zero, params, goals.data(), n_goals, &cc, &nc, nullptr) == RATSDF_ERR_BAD_ARGUMENT);
  CHECK(cc.empty() && nc.empty());
  ratsdf_cost_params bad = params;
  bad.rounds = 1;
  CHECK(grid.CostToGo(origin, dims, bad, goals.data(), n_goals, &cc, &nc, nullptr) == RATSDF_ERR_BAD_ARGUMENT);
  CHECK(cc.empty() && nc.empty());
  CHECK(grid.CostToGo(origin, dims, params, goals.data(), n_goals, nullptr, &nc, nullptr) == RATSDF_ERR_BAD_ARGUMENT);
  FILE* o = fopen(argv[4], "wb");
  CHECK(o);
  write_result(o, sa, ca, na);
  write_result(o, sb, cb, nb);
  fclose(o);
  printf("cost OK\n");
  return 0;
}
