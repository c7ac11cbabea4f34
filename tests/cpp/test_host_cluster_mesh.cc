// The clustered mesh through the C++ host layer (TSDFGrid::ClusterMesh, TSDFSystem::ClusterMesh) against one ABI library.
//   usage: test_host_cluster_mesh <library.so> <symbol prefix> <case file> <output file>
// The case file (written by tests/test_host_cluster_mesh.py, the layout of test_host_surface_mesh's): int32 H, W, ox, oy,
// oz, X, Y, Z; float32 fx, fy, cx, cy, qx, qy, qz, qw, tx, ty, tz, voxel size, truncation, max depth; then rgb
// (H*W*3 u8), depth, ht, lt (H*W f32 each).
// One frame goes into a TSDFGrid and into a TSDFSystem (identity extrinsics); both take the clustered mesh of the
// box (min_weight 1, factor 2).  The output file gets the grid's counts (uint64 vertices, uint64 triangles), records
// and index triples, then the system's.
// A library without the entry points (the CPU oracle) must report RATSDF_ERR_NOT_IMPLEMENTED from both calls and
// leave the vectors empty; nothing is written then.
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

  ratsdf_cluster_mesh_params params;
  memset(&params, 0, sizeof(params));
  params.min_weight = 1;
  params.factor = 2;
  std::vector<ratsdf_surface_point> av(3), bv(3);  // (stale content: a failed call must leave them empty)
  std::vector<int32_t> at(3), bt(3);
  TSDFGrid grid(vs, trunc, 0, &api);
  CHECK(grid.last_status() == RATSDF_OK);
  grid.Integrate(i_rgb, i_depth, i_ht, i_lt, max_depth, K, pose);
  CHECK(grid.last_status() == RATSDF_OK);
  const int st_grid = grid.ClusterMesh(origin, dims, params, &av, &at);

  int st_sys = RATSDF_OK;
  {
    TSDFSystem sys(vs, trunc, max_depth, K, SE3<float>::Identity(), 0, &api);
    sys.Integrate(pose, i_rgb, i_depth, i_ht, i_lt);
    sys.Flush();
    st_sys = sys.ClusterMesh(origin, dims, params, &bv, &bt);
    sys.terminate();
  }
  printf("status %d %d\n", st_grid, st_sys);
  std::vector<ratsdf_surface_point> cv(5);
  std::vector<int32_t> ct(5);
  CHECK(grid.ClusterMesh(origin, dims, params, nullptr, &ct) == RATSDF_ERR_BAD_ARGUMENT && ct.empty());
  CHECK(grid.ClusterMesh(origin, dims, params, &cv, nullptr) == RATSDF_ERR_BAD_ARGUMENT && cv.empty());
  if (!api.cluster_mesh) {  // the oracle: not implemented, reported through both layers
    CHECK(st_grid == RATSDF_ERR_NOT_IMPLEMENTED && st_sys == RATSDF_ERR_NOT_IMPLEMENTED);
    CHECK(av.empty() && at.empty() && bv.empty() && bt.empty());
    av.resize(2), at.resize(2);
    CHECK(grid.ClusterMesh(origin, dims, params, &av, &at) == RATSDF_ERR_NOT_IMPLEMENTED && av.empty() && at.empty());
    CHECK(grid.last_status() == RATSDF_ERR_NOT_IMPLEMENTED);
    printf("not implemented OK\n");
    return 0;
  }
  CHECK(st_grid == RATSDF_OK && st_sys == RATSDF_OK);
  CHECK(at.size() % 3 == 0 && !at.empty());
  for (const int32_t i : at) CHECK(i >= 0 && (size_t)i < av.size());
  const int32_t zero[3] = {8, 0, 8};
  cv.resize(5), ct.resize(5);
  CHECK(grid.ClusterMesh(origin, zero, params, &cv, &ct) == RATSDF_ERR_BAD_ARGUMENT && cv.empty() && ct.empty());
  params.min_weight = 0;
  CHECK(grid.ClusterMesh(origin, dims, params, &cv, &ct) == RATSDF_ERR_BAD_ARGUMENT);
  params.min_weight = 1;
  params.factor = 3;
  cv.resize(5), ct.resize(5);
  CHECK(grid.ClusterMesh(origin, dims, params, &cv, &ct) == RATSDF_ERR_BAD_ARGUMENT && cv.empty() && ct.empty());
  params.factor = 2;
  const int32_t nowhere[3] = {20000, 20000, 20000};
  cv.resize(5), ct.resize(5);
  CHECK(grid.ClusterMesh(nowhere, dims, params, &cv, &ct) == RATSDF_OK && cv.empty() && ct.empty());
  FILE* o = fopen(argv[4], "wb");
  CHECK(o);
  for (int k = 0; k < 2; ++k) {
    const std::vector<ratsdf_surface_point>& v = k ? bv : av;
    const std::vector<int32_t>& t = k ? bt : at;
    const uint64_t n[2] = {v.size(), t.size() / 3};
    CHECK(fwrite(n, sizeof(uint64_t), 2, o) == 2);
    CHECK(fwrite(v.data(), sizeof(ratsdf_surface_point), v.size(), o) == v.size());
    CHECK(fwrite(t.data(), sizeof(int32_t), t.size(), o) == t.size());
  }
  fclose(o);
  printf("cluster mesh OK\n");
  return 0;
}
