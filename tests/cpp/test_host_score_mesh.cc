// The label score against a mesh through the C++ host layer (TSDFGrid::MakeLabelMesh / ScoreMesh,
// TSDFSystem::MakeLabelMesh / ScoreMesh, the LabelMesh owner) against one ABI library.
//   usage: test_host_score_mesh <library.so> <symbol prefix> <case file> <output file>
// The case file (written by tests/test_host_score_mesh.py): int32 H, W, n vertices, n triangles, min_weight; float32
// fx, fy, cx, cy, qx, qy, qz, qw, tx, ty, tz, voxel size, truncation, max depth, cell, tsdf_below, max_dist, p_cutoff;
// then rgb (H*W*3 u8), depth, ht, lt (H*W f32 each), the vertices (3 f32 each), their labels (u8 each) and the
// triangles (3 int32 each).
// One frame goes into a TSDFGrid and into a TSDFSystem (identity extrinsics); each makes a mesh set and scores its
// map against it, and the grid also scores against the SYSTEM's set (a set belongs to the device).  The output file
// gets, for the grid and then for the system: the set's info (72 bytes), the score (4160 bytes), the number of
// per-voxel records (uint64) and the records.
// A library without the entry points (the CPU oracle) must report RATSDF_ERR_NOT_IMPLEMENTED from every call and
// hand back nothing; nothing is written then.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
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

static void write_result(FILE* o, const LabelMesh& mesh, const ratsdf_label_score& score,
                         const std::vector<ratsdf_voxel_label>& pv) {
  const ratsdf_labelmesh_info info = mesh.info();
  const uint64_t n = pv.size();
  CHECK(fwrite(&info, sizeof(info), 1, o) == 1);
  CHECK(fwrite(&score, sizeof(score), 1, o) == 1);
  CHECK(fwrite(&n, sizeof(n), 1, o) == 1);
  CHECK(fwrite(pv.data(), sizeof(ratsdf_voxel_label), pv.size(), o) == pv.size());
}

int main(int argc, char** argv) {
  CHECK(argc == 5);
  const Api& api = Api::Load(argv[1], argv[2]);
  FILE* f = fopen(argv[3], "rb");
  CHECK(f);
  int32_t hdr[5];
  float par[18];
  read_into(f, hdr, 5);
  read_into(f, par, 18);
  const int H = hdr[0], W = hdr[1];
  const size_t nv = (size_t)hdr[2], nt = (size_t)hdr[3];
  std::vector<uint8_t> rgb((size_t)H * W * 3), labels(nv);
  std::vector<float> depth((size_t)H * W), ht((size_t)H * W), lt((size_t)H * W), xyz(3 * nv);
  std::vector<int32_t> tri(3 * nt);
  read_into(f, rgb.data(), rgb.size());
  read_into(f, depth.data(), depth.size());
  read_into(f, ht.data(), ht.size());
  read_into(f, lt.data(), lt.size());
  read_into(f, xyz.data(), xyz.size());
  read_into(f, labels.data(), labels.size());
  read_into(f, tri.data(), tri.size());
  fclose(f);
  const CameraIntrinsics<float> K(par[0], par[1], par[2], par[3]);
  const SE3<float> pose(Quaternion<float>{par[4], par[5], par[6], par[7]}, Vector3<float>{par[8], par[9], par[10]});
  const float vs = par[11], trunc = par[12], max_depth = par[13], cell = par[14];
  ratsdf_score_params params;
  memset(&params, 0, sizeof(params));
  params.tsdf_below = par[15], params.max_dist = par[16], params.p_cutoff = par[17];
  params.min_weight = (uint32_t)hdr[4];
  const Image i_rgb{rgb.data(), H, W, kU8C3}, i_depth{depth.data(), H, W, kF32C1}, i_ht{ht.data(), H, W, kF32C1},
      i_lt{lt.data(), H, W, kF32C1};
  printf("backend %s\n", api.backend());

  ratsdf_label_score sa, sb, sc;
  memset(&sa, 0x55, sizeof(sa)), memset(&sb, 0x55, sizeof(sb)), memset(&sc, 0x55, sizeof(sc));
  const ratsdf_label_score untouched = sa;
  std::vector<ratsdf_voxel_label> va(3), vb(5);  // (what they hold is replaced, or dropped on a failure)
  LabelMesh mesh_a, mesh_b;
  TSDFGrid grid(vs, trunc, 0, &api);
  CHECK(grid.last_status() == RATSDF_OK);
  grid.Integrate(i_rgb, i_depth, i_ht, i_lt, max_depth, K, pose);
  CHECK(grid.last_status() == RATSDF_OK);
  const int st_make = grid.MakeLabelMesh(xyz.data(), labels.data(), nv, tri.data(), nt, cell, &mesh_a);
  const int st_grid = grid.ScoreMesh(mesh_a, params, &sa, &va);

  int st_sys_make = RATSDF_OK, st_sys = RATSDF_OK, st_cross = RATSDF_OK;
  {
    TSDFSystem sys(vs, trunc, max_depth, K, SE3<float>::Identity(), 0, &api);
    sys.Integrate(pose, i_rgb, i_depth, i_ht, i_lt);
    sys.Flush();
    st_sys_make = sys.MakeLabelMesh(xyz.data(), labels.data(), nv, tri.data(), nt, cell, &mesh_b);
    st_sys = sys.ScoreMesh(mesh_b, params, &sb, &vb);
    st_cross = grid.ScoreMesh(mesh_b, params, &sc);
    sys.terminate();
  }
  printf("status %d %d %d %d %d\n", st_make, st_grid, st_sys_make, st_sys, st_cross);
  if (!api.score_mesh) {  // the oracle: not implemented, reported through both layers
    CHECK(st_make == RATSDF_ERR_NOT_IMPLEMENTED && st_grid == RATSDF_ERR_NOT_IMPLEMENTED);
    CHECK(st_sys_make == RATSDF_ERR_NOT_IMPLEMENTED && st_sys == RATSDF_ERR_NOT_IMPLEMENTED);
    CHECK(grid.last_status() == RATSDF_ERR_NOT_IMPLEMENTED);
    CHECK(!mesh_a.valid() && !mesh_b.valid() && va.empty() && vb.empty());
    CHECK(!memcmp(&sa, &untouched, sizeof(sa)) && !memcmp(&sb, &untouched, sizeof(sb)));
    printf("not implemented OK\n");
    return 0;
  }
  CHECK(st_make == RATSDF_OK && st_grid == RATSDF_OK && st_sys_make == RATSDF_OK && st_sys == RATSDF_OK);
  CHECK(st_cross == RATSDF_OK && mesh_a.valid() && mesh_b.valid());
  CHECK(mesh_a.info().vertices == (int64_t)nv && mesh_a.info().triangles == (int64_t)nt);
  CHECK(mesh_a.info().kept <= (int64_t)nt && mesh_a.info().refs >= mesh_a.info().kept);
  CHECK((int64_t)va.size() == sa.voxels && (int64_t)vb.size() == sb.voxels);
  // the system's set serves the grid (the set outlives the system that made it), and the table alone is the table
  CHECK(!memcmp(&sc, &sa, sizeof(sa)));
  // a moved set keeps its triangles; the source is empty
  LabelMesh moved(std::move(mesh_a));
  CHECK(moved.valid() && !mesh_a.valid() && mesh_a.info().triangles == 0);
  ratsdf_label_score sd;
  CHECK(grid.ScoreMesh(moved, params, &sd) == RATSDF_OK && !memcmp(&sd, &sa, sizeof(sa)));
  // refusals hand back nothing and leave the score alone
  ratsdf_score_params bad = params;
  bad.flags = 1u;
  std::vector<ratsdf_voxel_label> vc(9);
  ratsdf_label_score se = untouched;
  CHECK(grid.ScoreMesh(moved, bad, &se, &vc) == RATSDF_ERR_BAD_ARGUMENT && vc.empty());
  CHECK(grid.ScoreMesh(mesh_a, params, &se, &vc) == RATSDF_ERR_BAD_ARGUMENT && vc.empty());  // (no set)
  CHECK(grid.ScoreMesh(moved, params, nullptr) == RATSDF_ERR_BAD_ARGUMENT);
  CHECK(!memcmp(&se, &untouched, sizeof(se)));
  const uint8_t wrong[3] = {1, 3, 1};
  const int32_t one[3] = {0, 1, 2}, beyond[3] = {0, 1, 3}, minus[3] = {0, -1, 2};
  LabelMesh none;
  CHECK(grid.MakeLabelMesh(xyz.data(), wrong, 3, one, 1, cell, &none) == RATSDF_ERR_BAD_ARGUMENT && !none.valid());
  CHECK(grid.MakeLabelMesh(xyz.data(), labels.data(), 3, beyond, 1, cell, &none) == RATSDF_ERR_BAD_ARGUMENT);
  CHECK(grid.MakeLabelMesh(xyz.data(), labels.data(), 3, minus, 1, cell, &none) == RATSDF_ERR_BAD_ARGUMENT);
  CHECK(!none.valid());
  CHECK(grid.MakeLabelMesh(xyz.data(), labels.data(), nv, tri.data(), nt, cell, nullptr) == RATSDF_ERR_BAD_ARGUMENT);
  FILE* o = fopen(argv[4], "wb");
  CHECK(o);
  write_result(o, moved, sa, va);
  write_result(o, mesh_b, sb, vb);
  fclose(o);
  printf("score OK\n");
  return 0;
}
