// The exposure read-out through the C++ host layer (TSDFGrid::Exposure, TSDFSystem::Exposure) against one ABI library.
//   usage: test_host_exposure <library.so> <symbol prefix> <case file> <output file>
// The case file (written by tests/test_host_exposure.py): int32 H, W, ox, oy, oz, X, Y, Z, flags, n_lamps, max_points;
// float32 fx, fy, cx, cy, qx, qy, qz, qw, tx, ty, tz, voxel size, truncation, max depth, occupied_below, max_range,
// min_irradiance, p_cutoff; then rgb (H*W*3 u8), depth, ht, lt (H*W f32 each); then the lamps (n_lamps x 4 float32).
// One frame goes into a TSDFGrid and into a TSDFSystem (identity extrinsics); both take the box's surface points, keep
// the first max_points and compute their exposure.  The output file gets, for the grid and then for the system: the
// summary, the lamp table, the doses, the masks.
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

static void write_result(FILE* o, const ratsdf_exposure_summary& s, const std::vector<ratsdf_lamp_record>& table,
                         const std::vector<float>& dose, const std::vector<uint64_t>& mask) {
  CHECK(fwrite(&s, sizeof(s), 1, o) == 1);
  CHECK(fwrite(table.data(), sizeof(ratsdf_lamp_record), table.size(), o) == table.size());
  CHECK(fwrite(dose.data(), sizeof(float), dose.size(), o) == dose.size());
  CHECK(fwrite(mask.data(), sizeof(uint64_t), mask.size(), o) == mask.size());
}

int main(int argc, char** argv) {
  CHECK(argc == 5);
  const Api& api = Api::Load(argv[1], argv[2]);
  FILE* f = fopen(argv[3], "rb");
  CHECK(f);
  int32_t hdr[11];
  float par[18];
  read_into(f, hdr, 11);
  read_into(f, par, 18);
  const int H = hdr[0], W = hdr[1];
  const int32_t origin[3] = {hdr[2], hdr[3], hdr[4]}, dims[3] = {hdr[5], hdr[6], hdr[7]};
  const int32_t n_lamps = hdr[9];
  const size_t max_points = (size_t)hdr[10];
  std::vector<uint8_t> rgb((size_t)H * W * 3);
  std::vector<float> depth((size_t)H * W), ht((size_t)H * W), lt((size_t)H * W);
  std::vector<ratsdf_lamp> lamps((size_t)n_lamps);
  read_into(f, rgb.data(), rgb.size());
  read_into(f, depth.data(), depth.size());
  read_into(f, ht.data(), ht.size());
  read_into(f, lt.data(), lt.size());
  read_into(f, lamps.data(), lamps.size());
  fclose(f);
  const CameraIntrinsics<float> K(par[0], par[1], par[2], par[3]);
  const SE3<float> pose(Quaternion<float>{par[4], par[5], par[6], par[7]}, Vector3<float>{par[8], par[9], par[10]});
  const float vs = par[11], trunc = par[12], max_depth = par[13];
  const ratsdf_exposure_params params = {par[14], par[15], par[16], par[17], (uint32_t)hdr[8], {0u, 0u, 0u}};
  const ratsdf_surface_params sp = {1, 0.0f, 0u, 0u};
  const Image i_rgb{rgb.data(), H, W, kU8C3}, i_depth{depth.data(), H, W, kF32C1}, i_ht{ht.data(), H, W, kF32C1},
      i_lt{lt.data(), H, W, kF32C1};
  printf("backend %s\n", api.backend());

  std::vector<ratsdf_surface_point> pa, pb;
  std::vector<float> da(3, 7.0f), db(5, 7.0f);          // (what they hold is replaced, or dropped on a failure)
  std::vector<uint64_t> ma(2, 1), mb(4, 1);
  std::vector<ratsdf_lamp_record> ta(1), tb(2);
  ratsdf_exposure_summary sa, sb;
  memset(&sa, 0x5A, sizeof(sa));
  memset(&sb, 0x5A, sizeof(sb));
  TSDFGrid grid(vs, trunc, 0, &api);
  CHECK(grid.last_status() == RATSDF_OK);
  grid.Integrate(i_rgb, i_depth, i_ht, i_lt, max_depth, K, pose);
  CHECK(grid.last_status() == RATSDF_OK);
  const int st_points = grid.SurfacePoints(origin, dims, sp, &pa);
  if (pa.size() > max_points) pa.resize(max_points);
  // (without surface points the call is still made, on a made-up point: its status is what is checked)
  const ratsdf_surface_point made_up = {{0.0f, 0.0f, 1.0f}, {0.0f, 0.0f, -1.0f}, 0.5f, {0, 0, 0, 1}};
  if (st_points != RATSDF_OK) pa.assign(1, made_up);
  const int st_grid = grid.Exposure(origin, dims, params, pa.data(), (int64_t)pa.size(), lamps.data(), n_lamps, &da,
                                    &ma, &ta, &sa);

  int st_sys = RATSDF_OK;
  {
    TSDFSystem sys(vs, trunc, max_depth, K, SE3<float>::Identity(), 0, &api);
    sys.Integrate(pose, i_rgb, i_depth, i_ht, i_lt);
    sys.Flush();
    if (sys.SurfacePoints(origin, dims, sp, &pb) != RATSDF_OK) pb.assign(1, made_up);
    if (pb.size() > max_points) pb.resize(max_points);
    st_sys = sys.Exposure(origin, dims, params, pb.data(), (int64_t)pb.size(), lamps.data(), n_lamps, &db, &mb, &tb,
                          &sb);
    sys.terminate();
  }
  printf("status %d %d\n", st_grid, st_sys);
  if (!api.exposure) {  // the oracle: not implemented, reported through both layers
    CHECK(st_grid == RATSDF_ERR_NOT_IMPLEMENTED && st_sys == RATSDF_ERR_NOT_IMPLEMENTED);
    CHECK(grid.last_status() == RATSDF_ERR_NOT_IMPLEMENTED);
    CHECK(da.empty() && db.empty() && ma.empty() && mb.empty() && ta.empty() && tb.empty());
    CHECK(sa.points_lit == 0x5A5A5A5A && sb.points_lit == 0x5A5A5A5A);
    printf("not implemented OK\n");
    return 0;
  }
  CHECK(st_points == RATSDF_OK && st_grid == RATSDF_OK && st_sys == RATSDF_OK);
  const size_t n = pa.size();
  CHECK(n > 0 && pb.size() == n && !memcmp(pa.data(), pb.data(), n * sizeof(ratsdf_surface_point)));
  CHECK(da.size() == n && db.size() == n && ma.size() == n && mb.size() == n);
  CHECK(ta.size() == (size_t)n_lamps && tb.size() == (size_t)n_lamps);
  // the dose alone equals the dose with the rest; with ACCUMULATE on a dose of zeros as well
  std::vector<float> dc(1, 3.0f);
  CHECK(grid.Exposure(origin, dims, params, pa.data(), (int64_t)n, lamps.data(), n_lamps, &dc, nullptr, nullptr,
                      nullptr) == RATSDF_OK);
  CHECK(dc.size() == n && !memcmp(dc.data(), da.data(), n * sizeof(float)));
  ratsdf_exposure_params more = params;
  more.flags |= RATSDF_EXPOSURE_ACCUMULATE;
  std::vector<float> dd(n, 0.0f);
  std::vector<uint64_t> md;
  CHECK(grid.Exposure(origin, dims, more, pa.data(), (int64_t)n, lamps.data(), n_lamps, &dd, &md, nullptr, nullptr) ==
        RATSDF_OK);
  CHECK(!memcmp(dd.data(), da.data(), n * sizeof(float)) && !memcmp(md.data(), ma.data(), n * sizeof(uint64_t)));
  // refusals hand back nothing
  std::vector<float> short_dose(n - 1, 0.0f);
  CHECK(grid.Exposure(origin, dims, more, pa.data(), (int64_t)n, lamps.data(), n_lamps, &short_dose, &md, nullptr,
                      nullptr) == RATSDF_ERR_BAD_ARGUMENT);
  CHECK(short_dose.empty() && md.empty());
  const int32_t zero[3] = {8, 0, 8};
  std::vector<ratsdf_lamp_record> tc(9);
  CHECK(grid.Exposure(origin, zero, params, pa.data(), (int64_t)n, lamps.data(), n_lamps, &dc, &md, &tc, nullptr) ==
        RATSDF_ERR_BAD_ARGUMENT);
  CHECK(dc.empty() && md.empty() && tc.empty());
  CHECK(grid.Exposure(origin, dims, params, pa.data(), (int64_t)n, lamps.data(), 65, &dc, &md, &tc, nullptr) ==
        RATSDF_ERR_BAD_ARGUMENT);
  CHECK(grid.Exposure(origin, dims, params, pa.data(), (int64_t)n, lamps.data(), n_lamps, nullptr, &md, &tc, nullptr) ==
        RATSDF_ERR_BAD_ARGUMENT);
  // no points and no lamps are valid inputs
  CHECK(grid.Exposure(origin, dims, params, nullptr, 0, nullptr, 0, &dc, &md, &tc, &sa) == RATSDF_OK);
  CHECK(dc.empty() && md.empty() && tc.empty() && sa.lit_pairs == 0 && sa.lamps_accepted == 0);
  CHECK(grid.Exposure(origin, dims, params, pa.data(), (int64_t)n, lamps.data(), n_lamps, &da, &ma, &ta, &sa) ==
        RATSDF_OK);
  FILE* o = fopen(argv[4], "wb");
  CHECK(o);
  write_result(o, sa, ta, da, ma);
  write_result(o, sb, tb, db, mb);
  fclose(o);
  printf("exposure OK\n");
  return 0;
}
