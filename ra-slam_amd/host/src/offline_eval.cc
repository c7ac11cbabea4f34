// offline_eval.cc -- the reference's offline harness (main/offline_eval.cc:37-99) on the host layer:
// a folder dataset is read frame by frame and integrated through TSDFSystem; the map can then be
// written in the reference's formats (DownloadAll records, DownloadAllMesh triple).
//
// Differences that are deliberate:
//   * no segmentation network here: Integrate gets empty ht / lt, i.e. the all-ones
//     images of modules/tsdf_module.cc:27-31;
//   * the queue is drained (Flush) before the downloads; the reference calls terminate() right after
//     the last Integrate, which drops whatever is still queued (SURVEY 8b quirk i);
//   * kept as is: the reader's extrinsics are passed to TSDFSystem although folder_reader has already
//     multiplied them into every pose (SURVEY 8b quirk iii, offline_eval.cc:57);
//   * <folder> may be a ScanNet .sens stream (scannet_sens_reader, as examples/scannet_evaluation/
//     eval_one.cc:41-87 uses it).
//
// usage: ratsdf_offline_eval <folder> [--lib libratsdf.so] [--voxel 0.01]
//          [--max-depth 6] [--device 0] [--frames N] [--download-all FILE] [--download-mesh PREFIX]
//          [--reader-only] [--dump-frames DIR] [--dump-raw-color (.sens: also DIR/<i>.color, the colour
//          frame before the resize, and DIR/raw_meta.txt = its width and height)]
//          [--threads N (decoder threads, default 4)]
//          [--load-map FILE (a map checkpoint to continue, before the first frame; its voxel size must be --voxel)]
//          [--first-frame K (skip the first K frames of the dataset)] [--save-map FILE (after the last frame)]
//          [--fuse-map FILE (a checkpoint fused into the map after the last frame, before --save-map / the downloads)]
//          [--save-coarse-map FILE [--coarse-levels K (default 1, 1 .. 8)] (after the last frame and --fuse-map: the
//          checkpoint of the map coarsened K times by two, include/ratsdf_coarsen.h -- voxel size 2^K * --voxel, same
//          truncation; the levels are chained through temporary grids)]
//          [--surface-points FILE (after the last frame: the oriented surface points of the map's bounding box,
//          32-byte records of include/ratsdf_surface.h, min_weight 1; a box beyond 512 voxels along an axis is
//          covered by block-aligned boxes of at most 512, z then y then x, each in the header's order)]
//          [--surface-mesh FILE.ply (after the last frame: the welded triangle mesh of the map's bounding box,
//          include/ratsdf_surface_mesh.h, min_weight 1, as one binary little-endian PLY -- vertices x y z nx ny nz
//          (float), red green blue (uchar), prob (float), weight (uchar); faces as lists of three int indices.  The box
//          is tiled as for --surface-points; each tile's mesh is self-contained, so the vertices on a face two tiles
//          share are written once per tile: duplicates there are accepted)]
//          [--cluster-mesh FILE.ply [--cluster-factor K (2, 4 or 8; default 4)] (after the last frame: the clustered
//          mesh of the map's bounding box, include/ratsdf_cluster_mesh.h, min_weight 1, in the PLY layout of
//          --surface-mesh.  ONE box, not tiled: clustered meshes of neighbouring boxes do not stitch, so a bounding box
//          of more than 1024 voxels along an axis is refused)]
//          [--score-labels FILE [--score-cutoff P (0.5)] [--score-max-dist D (4 cells of the set)]
//          [--score-tsdf-below T (0.1)] (after the last frame: the map scored against the labelled points of FILE, raw
//          16-byte records {float x, y, z; uint32 label} with label 0 unannotated, 1 low-touch, 2 high-touch --
//          include/ratsdf_score.h, what python_utils/scannet_eval/scanneteval.py computes from a DownloadAll file.
//          Prints "score TP FP FN TN" with the four counts and "iou V" to stdout)]
//          [--score-mesh FILE (likewise, against the labelled triangle mesh of FILE -- include/ratsdf_score_mesh.h, the
//          script's nn_method="mesh"; raw little-endian: int64 V, int64 T, then V records {float x, y, z; uint32 label},
//          then T records of three int32 vertex indices.  The other --score-* options apply.  Prints the same two
//          lines; given together with --score-labels the lines of the two are prefixed "points " and "mesh ")]
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include "ratsdf/dataset.hpp"
#include "ratsdf/tsdf_system.hpp"

using namespace ratsdf;

namespace {
void write_file(const std::string& path, const void* data, size_t bytes) {
  std::ofstream f(path, std::ios::binary);
  f.write(static_cast<const char*>(data), (std::streamsize)bytes);
  if (!f) {
    fprintf(stderr, "cannot write %s\n", path.c_str());
    exit(2);
  }
}

// the block-aligned bounding box of the map's voxels, lo .. hi inclusive; false when the map is empty
bool map_bounds(TSDFSystem& tsdf, float vs, int lo[3], int hi[3]) {
  const float far = 32000.f * vs;  // (every voxel index the directory can hold lies within +-32768)
  const std::vector<VoxelSpatialTSDF> vox = tsdf.Query(BoundingCube<float>{-far, far, -far, far, -far, far});
  for (int a = 0; a < 3; ++a) lo[a] = 32767, hi[a] = -32768;
  for (const VoxelSpatialTSDF& v : vox) {
    const int idx[3] = {(int)lrintf(v.x / vs), (int)lrintf(v.y / vs), (int)lrintf(v.z / vs)};
    for (int a = 0; a < 3; ++a) lo[a] = std::min(lo[a], idx[a]), hi[a] = std::max(hi[a], idx[a]);
  }
  for (int a = 0; a < 3; ++a) lo[a] = std::max(lo[a] & ~7, -32768), hi[a] = std::min(hi[a] | 7, 32767);  // whole blocks
  return !vox.empty();
}

// the oriented surface points of the map's bounding box (include/ratsdf_surface.h) as a file of records
int write_surface_points(TSDFSystem& tsdf, float vs, const std::string& path) {
  std::vector<ratsdf_surface_point> all, part;
  int lo[3], hi[3];
  if (map_bounds(tsdf, vs, lo, hi)) {
    ratsdf_surface_params params;
    memset(&params, 0, sizeof(params));
    params.min_weight = 1;
    for (int z = lo[2]; z <= hi[2]; z += 512)
      for (int y = lo[1]; y <= hi[1]; y += 512)
        for (int x = lo[0]; x <= hi[0]; x += 512) {
          const int32_t origin[3] = {x, y, z};
          const int32_t dims[3] = {std::min(512, hi[0] - x + 1), std::min(512, hi[1] - y + 1),
                                   std::min(512, hi[2] - z + 1)};
          const int st = tsdf.SurfacePoints(origin, dims, params, &part);
          if (st != RATSDF_OK) return st;
          all.insert(all.end(), part.begin(), part.end());
        }
  }
  write_file(path, all.data(), all.size() * sizeof(ratsdf_surface_point));
  fprintf(stderr, "[offline_eval] %zu surface points to %s\n", all.size(), path.c_str());
  return RATSDF_OK;
}

// a mesh as a binary little-endian PLY: vertices x y z nx ny nz (float), red green blue (uchar), prob (float), weight
// (uchar); faces as lists of three int indices
void write_ply(const std::vector<ratsdf_surface_point>& vertices, const std::vector<int32_t>& triangles,
               const char* kind, float vs, const std::string& path) {
  const size_t nv = vertices.size(), nt = triangles.size() / 3;
  char header[512];
  const int hn = snprintf(header, sizeof(header),
                          "ply\nformat binary_little_endian 1.0\ncomment ratsdf %s mesh, voxel size %g\n"
                          "element vertex %zu\nproperty float x\nproperty float y\nproperty float z\n"
                          "property float nx\nproperty float ny\nproperty float nz\n"
                          "property uchar red\nproperty uchar green\nproperty uchar blue\n"
                          "property float prob\nproperty uchar weight\n"
                          "element face %zu\nproperty list uchar int vertex_indices\nend_header\n",
                          kind, vs, nv, nt);
  std::vector<uint8_t> file((size_t)hn + nv * 32 + nt * 13);
  uint8_t* p = file.data();
  memcpy(p, header, (size_t)hn), p += hn;
  for (const ratsdf_surface_point& v : vertices) {  // 24 + 3 + 4 + 1 bytes: the record, colour before probability
    memcpy(p, v.pos, 12), memcpy(p + 12, v.normal, 12);
    p[24] = v.rgbw.r, p[25] = v.rgbw.g, p[26] = v.rgbw.b;
    memcpy(p + 27, &v.prob, 4);
    p[31] = v.rgbw.weight;
    p += 32;
  }
  for (size_t i = 0; i < nt; ++i) {
    *p = 3;
    memcpy(p + 1, &triangles[3 * i], 12);
    p += 13;
  }
  write_file(path, file.data(), file.size());
  fprintf(stderr, "[offline_eval] %zu vertices, %zu triangles to %s\n", nv, nt, path.c_str());
}

// the welded triangle mesh of the map's bounding box (include/ratsdf_surface_mesh.h) as a binary little-endian PLY;
// tiled exactly as write_surface_points tiles, each tile's indices offset by the vertices written before it
int write_surface_mesh(TSDFSystem& tsdf, float vs, const std::string& path) {
  std::vector<ratsdf_surface_point> vertices, part_v;
  std::vector<int32_t> triangles, part_t;
  int lo[3], hi[3];
  if (map_bounds(tsdf, vs, lo, hi)) {
    ratsdf_surface_mesh_params params;
    memset(&params, 0, sizeof(params));
    params.min_weight = 1;
    for (int z = lo[2]; z <= hi[2]; z += 512)
      for (int y = lo[1]; y <= hi[1]; y += 512)
        for (int x = lo[0]; x <= hi[0]; x += 512) {
          const int32_t origin[3] = {x, y, z};
          const int32_t dims[3] = {std::min(512, hi[0] - x + 1), std::min(512, hi[1] - y + 1),
                                   std::min(512, hi[2] - z + 1)};
          const int st = tsdf.SurfaceMesh(origin, dims, params, &part_v, &part_t);
          if (st != RATSDF_OK) return st;
          if (vertices.size() + part_v.size() > (size_t)INT32_MAX) return RATSDF_ERR_BAD_ARGUMENT;  // (int indices)
          const int32_t base = (int32_t)vertices.size();
          vertices.insert(vertices.end(), part_v.begin(), part_v.end());
          for (const int32_t i : part_t) triangles.push_back(base + i);
        }
  }
  write_ply(vertices, triangles, "surface", vs, path);
  return RATSDF_OK;
}

// the clustered mesh of the map's bounding box (include/ratsdf_cluster_mesh.h) as a PLY of the same layout.  ONE box:
// meshes of boxes that tile space do not stitch (a cluster that a box cuts averages only that box's members), so a
// bounding box beyond the header's limits (1024 voxels along an axis, 2^27 voxels) is refused by the library
int write_cluster_mesh(TSDFSystem& tsdf, float vs, int factor, const std::string& path) {
  std::vector<ratsdf_surface_point> vertices;
  std::vector<int32_t> triangles;
  int lo[3], hi[3];
  if (map_bounds(tsdf, vs, lo, hi)) {
    ratsdf_cluster_mesh_params params;
    memset(&params, 0, sizeof(params));
    params.min_weight = 1;
    params.factor = factor;
    const int32_t origin[3] = {lo[0], lo[1], lo[2]};
    const int32_t dims[3] = {hi[0] - lo[0] + 1, hi[1] - lo[1] + 1, hi[2] - lo[2] + 1};
    const int st = tsdf.ClusterMesh(origin, dims, params, &vertices, &triangles);
    if (st != RATSDF_OK) return st;
  }
  write_ply(vertices, triangles, "cluster", vs, path);
  return RATSDF_OK;
}

// the map scored against the labelled points of a file of {float x, y, z; uint32 label} records
// (include/ratsdf_score.h); max_dist <= 0: four cells of the set
int score_labels(TSDFSystem& tsdf, const std::string& path, float tsdf_below, float max_dist, float cutoff,
                 const char* prefix) {
  std::ifstream f(path, std::ios::binary | std::ios::ate);
  if (!f) return RATSDF_ERR_BAD_ARGUMENT;
  const size_t bytes = (size_t)f.tellg();
  if (bytes % 16) return RATSDF_ERR_BAD_ARGUMENT;
  std::vector<uint32_t> raw(bytes / 4);
  f.seekg(0);
  f.read(reinterpret_cast<char*>(raw.data()), (std::streamsize)bytes);
  if (!f) return RATSDF_ERR_BAD_ARGUMENT;
  const size_t n = bytes / 16;
  std::vector<float> xyz(3 * n);
  std::vector<uint8_t> labels(n);
  for (size_t i = 0; i < n; ++i) {
    memcpy(&xyz[3 * i], &raw[4 * i], 12);
    if (raw[4 * i + 3] > 2u) return RATSDF_ERR_BAD_ARGUMENT;
    labels[i] = (uint8_t)raw[4 * i + 3];
  }
  LabelSet set;
  int st = tsdf.MakeLabelSet(xyz.data(), labels.data(), n, 0.f, &set);
  if (st != RATSDF_OK) return st;
  ratsdf_score_params params;
  memset(&params, 0, sizeof(params));
  params.tsdf_below = tsdf_below;
  params.max_dist = max_dist > 0.f ? max_dist : 4.f * set.info().cell;
  params.p_cutoff = cutoff;
  ratsdf_label_score score;
  st = tsdf.ScoreLabels(set, params, &score);
  if (st != RATSDF_OK) return st;
  const double tp = (double)score.confusion[0], fp = (double)score.confusion[1], fn = (double)score.confusion[2];
  fprintf(stderr, "[offline_eval] %zu labelled points (%lld kept); %lld voxels, %lld selected, %lld unmatched, "
          "%lld unannotated\n", n, (long long)set.info().kept, (long long)score.voxels, (long long)score.selected,
          (long long)score.unmatched, (long long)score.unannotated);
  printf("%sscore %lld %lld %lld %lld\n", prefix, (long long)score.confusion[0], (long long)score.confusion[1],
         (long long)score.confusion[2], (long long)score.confusion[3]);
  printf("%siou %.17g\n", prefix, tp / (tp + fp + fn + 1e-15));  // scanneteval.py:100
  return RATSDF_OK;
}

// the map scored against the labelled triangle mesh of a file: int64 V, int64 T, V records {float x, y, z; uint32
// label}, T records of three int32 (include/ratsdf_score_mesh.h); max_dist <= 0: four cells of the set
int score_mesh(TSDFSystem& tsdf, const std::string& path, float tsdf_below, float max_dist, float cutoff,
               const char* prefix) {
  std::ifstream f(path, std::ios::binary | std::ios::ate);
  if (!f) return RATSDF_ERR_BAD_ARGUMENT;
  const size_t bytes = (size_t)f.tellg();
  int64_t head[2] = {0, 0};
  f.seekg(0);
  f.read(reinterpret_cast<char*>(head), 16);
  if (!f || head[0] < 0 || head[1] < 0 || head[0] > ((int64_t)1 << 26) || head[1] > ((int64_t)1 << 26))
    return RATSDF_ERR_BAD_ARGUMENT;
  const size_t nv = (size_t)head[0], nt = (size_t)head[1];
  if (bytes != 16 + 16 * nv + 12 * nt) return RATSDF_ERR_BAD_ARGUMENT;
  std::vector<uint32_t> raw(4 * nv);
  std::vector<int32_t> tri(3 * nt);
  f.read(reinterpret_cast<char*>(raw.data()), (std::streamsize)(16 * nv));
  f.read(reinterpret_cast<char*>(tri.data()), (std::streamsize)(12 * nt));
  if (!f) return RATSDF_ERR_BAD_ARGUMENT;
  std::vector<float> xyz(3 * nv);
  std::vector<uint8_t> labels(nv);
  for (size_t i = 0; i < nv; ++i) {
    memcpy(&xyz[3 * i], &raw[4 * i], 12);
    if (raw[4 * i + 3] > 2u) return RATSDF_ERR_BAD_ARGUMENT;
    labels[i] = (uint8_t)raw[4 * i + 3];
  }
  LabelMesh mesh;
  int st = tsdf.MakeLabelMesh(xyz.data(), labels.data(), nv, tri.data(), nt, 0.f, &mesh);
  if (st != RATSDF_OK) return st;
  const ratsdf_labelmesh_info info = mesh.info();
  ratsdf_score_params params;
  memset(&params, 0, sizeof(params));
  params.tsdf_below = tsdf_below;
  params.max_dist = max_dist > 0.f ? max_dist : 4.f * info.cell;
  params.p_cutoff = cutoff;
  ratsdf_label_score score;
  st = tsdf.ScoreMesh(mesh, params, &score);
  if (st != RATSDF_OK) return st;
  const double tp = (double)score.confusion[0], fp = (double)score.confusion[1], fn = (double)score.confusion[2];
  fprintf(stderr, "[offline_eval] %zu labelled triangles (%lld kept, %lld of mixed labels, %lld cell references); "
          "%lld voxels, %lld selected, %lld unmatched, %lld unannotated\n", nt, (long long)info.kept,
          (long long)info.mixed, (long long)info.refs, (long long)score.voxels, (long long)score.selected,
          (long long)score.unmatched, (long long)score.unannotated);
  printf("%sscore %lld %lld %lld %lld\n", prefix, (long long)score.confusion[0], (long long)score.confusion[1],
         (long long)score.confusion[2], (long long)score.confusion[3]);
  printf("%siou %.17g\n", prefix, tp / (tp + fp + fn + 1e-15));  // scanneteval.py:100
  return RATSDF_OK;
}

// the map coarsened `levels` times by two (include/ratsdf_coarsen.h) as a checkpoint: a chain of grids of twice the
// voxel size each, a level destroyed as soon as the next one exists
int write_coarse_map(TSDFSystem& tsdf, const Api& api, float vs, float trunc, int device, int levels,
                     const std::string& path) {
  std::unique_ptr<TSDFGrid> cur;
  for (int l = 0; l < levels; ++l) {
    vs = 2.0f * vs;
    auto next = std::make_unique<TSDFGrid>(vs, trunc, device, &api);
    if (next->last_status() != RATSDF_OK) return next->last_status();
    ratsdf_fuse_stats fs;
    memset(&fs, 0, sizeof(fs));
    const int st = cur ? next->FuseMapCoarsened(*cur, &fs) : tsdf.CoarsenInto(*next, &fs);
    if (st != RATSDF_OK) return st;
    fprintf(stderr, "[offline_eval] level %d: voxel size %g, %lld blocks, %lld voxels\n", l + 1, vs,
            (long long)fs.blocks_allocated, (long long)fs.voxels_copied);
    cur = std::move(next);
  }
  return cur->SaveMap(path);
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s <folder> [options]\n", argv[0]);
    return 2;
  }
  const std::string data_path = argv[1];
  const char* lib = nullptr;
  float voxel_size = 0.01f, max_depth = 6.f;  // offline_eval.cc:49-53
  int device = 0, max_frames = -1, threads = 4, first_frame = 0;
  std::string download_all, download_mesh, dump_dir, load_map, save_map, fuse_map, surface_points, save_coarse_map;
  std::string surface_mesh, cluster_mesh, score_file, score_mesh_file;
  int cluster_factor = 4;
  float score_cutoff = 0.5f, score_max_dist = 0.f, score_tsdf_below = 0.1f;
  int coarse_levels = 1;
  bool reader_only = false, dump_raw_color = false;
  for (int i = 2; i < argc; ++i) {
    const std::string a = argv[i];
    auto next = [&]() -> const char* {
      if (i + 1 >= argc) {
        fprintf(stderr, "missing value after %s\n", a.c_str());
        exit(2);
      }
      return argv[++i];
    };
    if (a == "--lib") lib = next();
    else if (a == "--voxel") voxel_size = strtof(next(), nullptr);
    else if (a == "--max-depth") max_depth = strtof(next(), nullptr);
    else if (a == "--device") device = atoi(next());
    else if (a == "--frames") max_frames = atoi(next());
    else if (a == "--threads") threads = atoi(next());
    else if (a == "--download-all") download_all = next();
    else if (a == "--download-mesh") download_mesh = next();
    else if (a == "--dump-frames") dump_dir = next();
    else if (a == "--reader-only") reader_only = true;
    else if (a == "--dump-raw-color") dump_raw_color = true;
    else if (a == "--load-map") load_map = next();
    else if (a == "--save-map") save_map = next();
    else if (a == "--fuse-map") fuse_map = next();
    else if (a == "--surface-points") surface_points = next();
    else if (a == "--surface-mesh") surface_mesh = next();
    else if (a == "--cluster-mesh") cluster_mesh = next();
    else if (a == "--cluster-factor") cluster_factor = atoi(next());
    else if (a == "--score-labels") score_file = next();
    else if (a == "--score-mesh") score_mesh_file = next();
    else if (a == "--score-cutoff") score_cutoff = strtof(next(), nullptr);
    else if (a == "--score-max-dist") score_max_dist = strtof(next(), nullptr);
    else if (a == "--score-tsdf-below") score_tsdf_below = strtof(next(), nullptr);
    else if (a == "--save-coarse-map") save_coarse_map = next();
    else if (a == "--coarse-levels") coarse_levels = atoi(next());
    else if (a == "--first-frame") first_frame = atoi(next());
    else {
      fprintf(stderr, "unknown option %s\n", a.c_str());
      return 2;
    }
  }
  if (coarse_levels < 1 || coarse_levels > 8) {
    fprintf(stderr, "--coarse-levels must lie in 1 .. 8\n");
    return 2;
  }
  const bool is_sens = data_path.size() > 5 && data_path.substr(data_path.size() - 5) == ".sens";
  try {
    std::unique_ptr<offline_data_provider> provider;
    if (is_sens) provider = std::make_unique<scannet_sens_reader>(data_path);
    else provider = std::make_unique<folder_reader>(data_path);
    const offline_data_provider& reader = *provider;
    int n = reader.get_size();
    if (max_frames >= 0 && max_frames < n) n = max_frames;
    const CameraIntrinsics<float> K = reader.get_camera_intrinsics();
    const SE3<float> ext = reader.get_camera_extrinsics();
    if (!dump_dir.empty()) {
      std::ofstream meta(dump_dir + "/meta.txt");
      meta.precision(9);
      const ratsdf_pose e = ext.abi();
      meta << reader.get_width() << " " << reader.get_height() << " " << n << " " << K.fx << " " << K.fy << " "
           << K.cx << " " << K.cy << " " << reader.get_depth_map_factor() << "\n"
           << e.qx << " " << e.qy << " " << e.qz << " " << e.qw << " " << e.tx << " " << e.ty << " " << e.tz
           << "\n";
    }
    if (dump_raw_color && is_sens && !dump_dir.empty()) {
      const auto& sr = static_cast<const scannet_sens_reader&>(reader);
      std::ofstream(dump_dir + "/raw_meta.txt") << sr.color_width() << " " << sr.color_height() << "\n";
      for (int i = 0; i < n; ++i) {
        const RgbImage full = sr.decode_color_full(i);
        write_file(dump_dir + "/" + std::to_string(i) + ".color", full.data.data(), full.data.size());
      }
    }
    std::unique_ptr<TSDFSystem> tsdf;
    if (!reader_only)
      tsdf = std::make_unique<TSDFSystem>(voxel_size, voxel_size * 6, max_depth, K, ext, device,
                                          &Api::Load(lib));
    fprintf(stderr, "[offline_eval] stream size %d (%dx%d)\n", n, reader.get_width(), reader.get_height());
    if (tsdf && !load_map.empty()) {  // map checkpoint (include/ratsdf_map.h): the run continues it
      const Api& api = Api::Load(lib);
      ratsdf_config cfg;
      int64_t n_blocks = 0;
      const int st = api.map_file_info ? api.map_file_info(load_map.c_str(), &cfg, &n_blocks)
                                       : RATSDF_ERR_NOT_IMPLEMENTED;
      if (st != RATSDF_OK) {
        fprintf(stderr, "[offline_eval] --load-map %s: %s\n", load_map.c_str(), api.status_string(st));
        return 1;
      }
      if (cfg.voxel_size != voxel_size) {
        fprintf(stderr, "[offline_eval] --load-map %s: voxel size %g, --voxel %g\n", load_map.c_str(),
                cfg.voxel_size, voxel_size);
        return 1;
      }
      if (tsdf->LoadMap(load_map) != RATSDF_OK) return 1;
      fprintf(stderr, "[offline_eval] loaded %lld blocks from %s\n", (long long)n_blocks, load_map.c_str());
    }
    std::vector<float> poses;
    double t_read = 0;
    const auto t_begin = std::chrono::steady_clock::now();
    FramePrefetcher source(reader, n, threads);  // decodes ahead; frames still arrive in order
    Frame fr;
    for (int frame_idx = 0; frame_idx < n; ++frame_idx) {  // offline_eval.cc:66-85
      if (tsdf && tsdf->is_terminated()) break;
      const auto t0 = std::chrono::steady_clock::now();
      if (!source.next(&fr)) break;  // pose, colour frame, depth frame in metres (:69-74)
      t_read += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      if (frame_idx < first_frame) continue;  // (--first-frame: integrated by the run that saved the map)
      const SE3<float>& cam_T_world = fr.pose;
      const PngImage& rgb = fr.rgb;
      const std::vector<float>& depth = fr.depth;
      if (!dump_dir.empty()) {
        const std::string stem = dump_dir + "/" + std::to_string(frame_idx);
        write_file(stem + ".rgb", rgb.data.data(), rgb.data.size());
        write_file(stem + ".depth", depth.data(), depth.size() * 4);
        const ratsdf_pose p = cam_T_world.abi();
        const float v[7] = {p.qx, p.qy, p.qz, p.qw, p.tx, p.ty, p.tz};
        poses.insert(poses.end(), v, v + 7);
      }
      if (tsdf) {
        const Image img_rgb{rgb.data.data(), rgb.height, rgb.width, kU8C3};
        const Image img_depth{depth.data(), rgb.height, rgb.width, kF32C1};
        tsdf->Integrate(cam_T_world, img_rgb, img_depth);  // no ht / lt: ones (tsdf_module.cc:27-31)
      }
    }
    if (!dump_dir.empty()) write_file(dump_dir + "/poses.bin", poses.data(), poses.size() * 4);
    if (tsdf) {
      tsdf->Flush();
      const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count();
      fprintf(stderr, "[offline_eval] %d frames in %.3f s (%.1f frames/s; waited %.3f s for the decoders)\n", n, dt,
              n / dt, t_read);
      if (!fuse_map.empty()) {  // map fusion (include/ratsdf_fuse.h): another session's checkpoint merged into this map
        ratsdf_fuse_stats fs;
        memset(&fs, 0, sizeof(fs));
        const int st = tsdf->FuseMapFile(fuse_map, &fs);
        if (st != RATSDF_OK) {
          fprintf(stderr, "[offline_eval] --fuse-map %s: %s\n", fuse_map.c_str(), Api::Load(lib).status_string(st));
          return 1;
        }
        fprintf(stderr, "[offline_eval] fused %lld blocks from %s (%lld new, %lld voxels copied, %lld averaged)\n",
                (long long)fs.blocks_seen, fuse_map.c_str(), (long long)fs.blocks_allocated, (long long)fs.voxels_copied,
                (long long)fs.voxels_averaged);
      }
      if (!save_map.empty() && tsdf->SaveMap(save_map) != RATSDF_OK) return 1;
      if (!save_coarse_map.empty()) {
        const int st = write_coarse_map(*tsdf, Api::Load(lib), voxel_size, voxel_size * 6, device, coarse_levels,
                                        save_coarse_map);
        if (st != RATSDF_OK) {
          fprintf(stderr, "[offline_eval] --save-coarse-map %s: %s\n", save_coarse_map.c_str(),
                  Api::Load(lib).status_string(st));
          return 1;
        }
      }
      if (!download_all.empty()) tsdf->DownloadAll(download_all);
      if (!download_mesh.empty())  // offline_eval.cc:95-98
        tsdf->DownloadAllMesh(download_mesh + "_vertices.bin", download_mesh + "_indices.bin",
                              download_mesh + "_vertices_prob.bin");
      if (!surface_points.empty()) {
        const int st = write_surface_points(*tsdf, voxel_size, surface_points);
        if (st != RATSDF_OK) {
          fprintf(stderr, "[offline_eval] --surface-points %s: %s\n", surface_points.c_str(),
                  Api::Load(lib).status_string(st));
          return 1;
        }
      }
      if (!surface_mesh.empty()) {
        const int st = write_surface_mesh(*tsdf, voxel_size, surface_mesh);
        if (st != RATSDF_OK) {
          fprintf(stderr, "[offline_eval] --surface-mesh %s: %s\n", surface_mesh.c_str(),
                  Api::Load(lib).status_string(st));
          return 1;
        }
      }
      if (!cluster_mesh.empty()) {
        const int st = write_cluster_mesh(*tsdf, voxel_size, cluster_factor, cluster_mesh);
        if (st != RATSDF_OK) {
          fprintf(stderr, "[offline_eval] --cluster-mesh %s: %s\n", cluster_mesh.c_str(),
                  Api::Load(lib).status_string(st));
          return 1;
        }
      }
      const bool score_both = !score_file.empty() && !score_mesh_file.empty();
      if (!score_file.empty()) {
        const int st = score_labels(*tsdf, score_file, score_tsdf_below, score_max_dist, score_cutoff,
                                    score_both ? "points " : "");
        if (st != RATSDF_OK) {
          fprintf(stderr, "[offline_eval] --score-labels %s: %s\n", score_file.c_str(),
                  Api::Load(lib).status_string(st));
          return 1;
        }
      }
      if (!score_mesh_file.empty()) {
        const int st = score_mesh(*tsdf, score_mesh_file, score_tsdf_below, score_max_dist, score_cutoff,
                                  score_both ? "mesh " : "");
        if (st != RATSDF_OK) {
          fprintf(stderr, "[offline_eval] --score-mesh %s: %s\n", score_mesh_file.c_str(),
                  Api::Load(lib).status_string(st));
          return 1;
        }
      }
      tsdf->terminate();
    } else {
      const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count();
      fprintf(stderr, "[offline_eval] read %d frames in %.3f s (%.1f frames/s, %d decoder threads)\n", n, dt,
              n / dt, threads);
    }
  } catch (const std::exception& e) {
    fprintf(stderr, "[offline_eval] %s\n", e.what());
    return 1;
  }
  printf("OK\n");
  return 0;
}
