// tsdf_grid.hpp -- TSDFGrid with the reference's method names (utils/tsdf/voxel_tsdf.cuh:39-145),
// forwarding to the C ABI of include/ratsdf.h.  The ABI library is bound at run time (dlopen), so
// this host layer builds with g++ alone; the default binding is the in-tree HIP engine.
#pragma once
#include <cstring>
#include <string>
#include <vector>

#include "types.hpp"

#ifndef RATSDF_ABI_PREFIX
#define RATSDF_ABI_PREFIX "ratsdf_"
#endif

namespace ratsdf {

// Every entry point this layer binds, X(name, required): ratsdf_<name> of the headers types.hpp includes.  A new one is
// one row here.  Those of include/ratsdf.h are required; those of the feature headers (ratsdf_map.h, ratsdf_sample.h,
// ...) are optional: the CPU oracle has none of them, and then the methods below report RATSDF_ERR_NOT_IMPLEMENTED.
#define RATSDF_API_ENTRIES(X)                                                                                        \
  X(create, 1) X(destroy, 1) X(integrate, 1) X(integrate_batch, 1) X(host_alloc, 1) X(host_free, 1)                  \
  X(synchronize, 1) X(recover, 1) X(query, 1) X(gather_valid, 1) X(gather_valid_semantic, 1) X(download_all, 1)      \
  X(raycast, 1) X(gather_valid_mesh, 1) X(download_all_mesh, 1) X(free_buffer, 1) X(num_active_blocks, 1)            \
  X(status_string, 1) X(backend, 1)                                                                                  \
  X(save_map, 0) X(load_map, 0) X(map_file_info, 0) X(sample_points, 0) X(esdf, 0) X(surface_points, 0)              \
  X(surface_mesh, 0) X(cluster_mesh, 0) X(regions, 0) X(cost_to_go, 0) X(exposure, 0)                                \
  X(labelset_create, 0) X(labelset_info_get, 0) X(labelset_destroy, 0) X(score_labels, 0)                            \
  X(labelmesh_create, 0) X(labelmesh_info_get, 0) X(labelmesh_destroy, 0) X(score_mesh, 0)                           \
  X(fuse_map, 0) X(fuse_blocks, 0) X(fuse_map_file, 0) X(fuse_map_transformed, 0) X(fuse_map_coarsened, 0)

// The entry points resolved from one shared library; each member has the type of its prototype.
struct Api {
#define X(name, required) decltype(&ratsdf_##name) name = nullptr;
  RATSDF_API_ENTRIES(X)
#undef X
  void* handle = nullptr;

  // path == nullptr: $RATSDF_LIB or libratsdf.so next to this layer.  The symbol prefix is "ratsdf_"
  // (the HIP engine); only test builds of this layer compile with another RATSDF_ABI_PREFIX to bind
  // the CPU oracle's copy of the ABI -- the product binaries have no switch for it.
  static const Api& Load(const char* path = nullptr, const char* prefix = RATSDF_ABI_PREFIX);
};

// Labelled records on the device, the common part of LabelSet and LabelMesh: the handle, its release and its info
// through the two Api members given.
template <class Handle, class Info, auto destroy, auto info_get>
class LabelHandle {
 public:
  LabelHandle() = default;
  ~LabelHandle() { reset(); }
  LabelHandle(LabelHandle&& o) noexcept : api_(o.api_), handle_(o.handle_) { o.handle_ = nullptr; }
  LabelHandle& operator=(LabelHandle&& o) noexcept {
    if (this != &o) {
      reset();
      api_ = o.api_, handle_ = o.handle_;
      o.handle_ = nullptr;
    }
    return *this;
  }
  LabelHandle(const LabelHandle&) = delete;
  LabelHandle& operator=(const LabelHandle&) = delete;
  void reset() {
    if (handle_ && api_ && api_->*destroy) (api_->*destroy)(handle_);
    handle_ = nullptr;
  }
  bool valid() const { return handle_ != nullptr; }
  Handle* handle() const { return handle_; }
  Info info() const {  // (zeros when there is none)
    Info i;
    memset(&i, 0, sizeof(i));
    if (handle_ && api_ && api_->*info_get) (api_->*info_get)(handle_, &i);
    return i;
  }

 private:
  friend class TSDFGrid;
  const Api* api_ = nullptr;
  Handle* handle_ = nullptr;
};

// Labelled points on the device (include/ratsdf_score.h): made by TSDFGrid::MakeLabelSet / TSDFSystem::MakeLabelSet,
// immutable, destroyed with the object.  It belongs to the device, not to the grid that made it: any grid of that
// device may score against it, and it may outlive them.
class LabelSet
    : public LabelHandle<ratsdf_labelset, ratsdf_labelset_info, &Api::labelset_destroy, &Api::labelset_info_get> {};

// A labelled triangle mesh on the device (include/ratsdf_score_mesh.h): made by TSDFGrid::MakeLabelMesh /
// TSDFSystem::MakeLabelMesh, immutable, destroyed with the object.  Like a LabelSet it belongs to the device, not to
// the grid that made it.
class LabelMesh : public LabelHandle<ratsdf_labelmesh, ratsdf_labelmesh_info, &Api::labelmesh_destroy,
                                     &Api::labelmesh_info_get> {};

class TSDFGrid {
 public:
  TSDFGrid(float voxel_size, float truncation, int device = 0, const Api* api = nullptr);
  ~TSDFGrid();
  TSDFGrid(const TSDFGrid&) = delete;
  TSDFGrid& operator=(const TSDFGrid&) = delete;

  // voxel_tsdf.cuh:65-67.  Like the reference (errors.cuh:13-20) failures do not throw; the last
  // status is kept and printed to stderr.
  void Integrate(const Image& img_rgb, const Image& img_depth, const Image& img_ht,
                 const Image& img_lt, float max_depth, const CameraIntrinsics<float>& intrinsics,
                 const SE3<float>& cam_T_world);
  // n frames in one call (ratsdf_integrate_batch): what the TSDFSystem worker does with its queue.
  // ht / lt may be null (all-ones images); `pinned`: every buffer comes from Api::host_alloc
  void IntegrateBatch(int n, const uint8_t* const* rgb, const float* const* depth,
                      const float* const* ht, const float* const* lt, int rows, int cols,
                      float max_depth, const CameraIntrinsics<float>& intrinsics,
                      const SE3<float>* cam_T_world, bool pinned);
  // voxel_tsdf.cuh:78-79; the two uchar4 images go to host buffers (H*W*4 bytes each, may be null)
  // instead of GLImage8UC4 textures
  void RayCast(float max_depth, const CameraParams& virtual_cam, const SE3<float>& cam_T_world,
               uint8_t* tsdf_rgba = nullptr, uint8_t* tsdf_normal = nullptr);
  std::vector<VoxelSpatialTSDF> GatherValid();                                   // :86
  std::vector<VoxelSpatialTSDFSEGM> GatherValidSemantic();                       // :93
  std::vector<VoxelSpatialTSDF> GatherVoxels(const BoundingCube<float>& volumn);  // :102
  // voxel_tsdf.cuh:104-106 (Vector3f / Vector3i buffers become flat float / int arrays, 3 per item)
  void GatherValidMesh(std::vector<float>* vertex_buffer, std::vector<int32_t>* index_buffer,
                       std::vector<float>* vertex_prob_buffer);
  void DownloadAll(const std::string& file_path);  // the write of tsdf_module.cc:57-64
  void DownloadAllMesh(const std::string& vertices_path, const std::string& indices_path,
                       const std::string& prob_path);  // tsdf_module.cc:66-86
  int NumActiveBlock();                            // voxel_hash.cu:225
  // cudaStreamSynchronize(stream_), voxel_tsdf.cu:450: the Integrate* calls do not wait for their frames; this does,
  // and it is where a device error of those frames surfaces (last_status())
  void Synchronize();
  // ratsdf_recover: after a sticky engine error (last_status() != 0 for good) rebuild what is derived from the block
  // directory and clear the error; true when the engine is usable again.  No reference counterpart (it asserts).
  bool Recover();
  // map checkpoints (include/ratsdf_map.h): the map to a file / the map replaced by a file's, which continues
  // bit-exactly.  Return the status (also kept in last_status()); no reference counterpart.
  int SaveMap(const std::string& path);
  int LoadMap(const std::string& path);
  // batched point sampling (include/ratsdf_sample.h): n world points (xyz: 3 floats each, metres) -> n records of the
  // trilinear TSDF, its gradient, the nearest voxel's probability and colour.  Returns the status (also kept in
  // last_status()); no reference counterpart (its nearest relative is RetrieveTSDF, with mirrored weights).
  int SamplePoints(const float* xyz, size_t n, ratsdf_sample* out);
  // Euclidean signed distance field over a box of voxels (include/ratsdf_esdf.h): origin / dims in voxel indices,
  // out: dims[0]*dims[1]*dims[2] floats (metres, x fastest), state: as many bytes or nullptr.  Returns the status
  // (also kept in last_status()); no reference counterpart.
  int ESDF(const int32_t origin[3], const int32_t dims[3], float occupied_below, uint32_t flags, float* out,
           uint8_t* state = nullptr);
  // oriented surface points of a box of voxels (include/ratsdf_surface.h): every sign change of the TSDF between two
  // neighbouring voxels as position, normal into free space, probability, colour and weight, in the header's order.
  // Returns the status (also kept in last_status()); *out is empty unless it is RATSDF_OK.  No reference counterpart.
  int SurfacePoints(const int32_t origin[3], const int32_t dims[3], const ratsdf_surface_params& params,
                    std::vector<ratsdf_surface_point>* out);
  // welded triangle mesh of a box of voxels (include/ratsdf_surface_mesh.h): the surface points the triangles of the
  // box's complete cells use, each once, and three indices into them per triangle, wound towards free space.  Returns
  // the status (also kept in last_status()); both vectors are empty unless it is RATSDF_OK.  No reference counterpart.
  int SurfaceMesh(const int32_t origin[3], const int32_t dims[3], const ratsdf_surface_mesh_params& params,
                  std::vector<ratsdf_surface_point>* vertices, std::vector<int32_t>* triangles);
  // clustered mesh of a box of voxels (include/ratsdf_cluster_mesh.h): SurfaceMesh with its vertices merged per
  // lattice-aligned cluster of params.factor^3 voxels (one record per non-empty cluster, the mean of its members) and
  // its triangles re-indexed, the degenerate ones dropped, each once.  Returns the status (also kept in
  // last_status()); both vectors are empty unless it is RATSDF_OK.  The reference simplifies on the host (Open3D).
  int ClusterMesh(const int32_t origin[3], const int32_t dims[3], const ratsdf_cluster_mesh_params& params,
                  std::vector<ratsdf_surface_point>* vertices, std::vector<int32_t>* triangles);
  // connected regions of a box of voxels (include/ratsdf_regions.h): the voxels that params admits grouped by face
  // adjacency inside the box; *labels (may be nullptr) receives dims[0] * dims[1] * dims[2] labels, *regions the table,
  // ascending in root.  Returns the status (also kept in last_status()); both vectors are empty unless it is RATSDF_OK.
  // No reference counterpart.
  int Regions(const int32_t origin[3], const int32_t dims[3], const ratsdf_regions_params& params,
              std::vector<int32_t>* labels, std::vector<ratsdf_region>* regions);
  // cost-to-go field of a box of voxels (include/ratsdf_cost.h): the least chamfer length of a path through
  // traversable voxels from every voxel to one of the n_goals goals (absolute voxel triples); *cost receives dims[0] *
  // dims[1] * dims[2] words, *next (may be nullptr) as many direction bytes, *summary (may be nullptr) the summary.
  // params.rounds must be 0: the call runs to convergence.  Returns the status (also kept in last_status()); both
  // vectors are empty unless it is RATSDF_OK.  No reference counterpart.
  int CostToGo(const int32_t origin[3], const int32_t dims[3], const ratsdf_cost_params& params, const int32_t* goals,
               int32_t n_goals, std::vector<uint32_t>* cost, std::vector<uint8_t>* next,
               ratsdf_cost_summary* summary);
  // exposure of surface points to lamps through a box of voxels (include/ratsdf_surface.h, ratsdf_exposure): which of
  // the n_lamps lamps light each of the n_points points, and the summed irradiance.  *dose is in/out: with
  // RATSDF_EXPOSURE_ACCUMULATE it must hold n_points floats and the sums go on from them, without the flag it is
  // replaced by n_points zeros first; *mask and *lamp_table (each may be nullptr) receive n_points words and n_lamps
  // records, *summary (may be nullptr) the summary.  Returns the status (also kept in last_status()); the vectors are
  // empty unless it is RATSDF_OK.  No reference counterpart.
  int Exposure(const int32_t origin[3], const int32_t dims[3], const ratsdf_exposure_params& params,
               const ratsdf_surface_point* points, int64_t n_points, const ratsdf_lamp* lamps, int32_t n_lamps,
               std::vector<float>* dose, std::vector<uint64_t>* mask, std::vector<ratsdf_lamp_record>* lamp_table,
               ratsdf_exposure_summary* summary);
  // the map scored against labelled points (include/ratsdf_score.h).  MakeLabelSet: n points (xyz: 3 floats each,
  // metres) with a label each (RATSDF_LABEL_*) into *out (what it held is destroyed first); cell: the edge of the
  // search grid, 0 for 8 voxel sizes.  ScoreLabels: every voxel that params selects takes the label of its nearest
  // point and counts against it in *out; *per_voxel (may be nullptr) receives one record per voxel in the order of
  // GatherValidSemantic.  Return the status (also kept in last_status()); after a failure the set is not valid, *out
  // is untouched and *per_voxel empty.  Replaces python_utils/scannet_eval/scanneteval.py on a DownloadAll file.
  int MakeLabelSet(const float* xyz, const uint8_t* labels, size_t n, float cell, LabelSet* out);
  int ScoreLabels(const LabelSet& set, const ratsdf_score_params& params, ratsdf_label_score* out,
                  std::vector<ratsdf_voxel_label>* per_voxel = nullptr);
  // the map scored against a labelled triangle mesh (include/ratsdf_score_mesh.h).  MakeLabelMesh: n_vertices points
  // (xyz: 3 floats each, metres) with a label each (RATSDF_LABEL_*) and n_triangles index triples into *out (what it
  // held is destroyed first); a triangle carries the label of its first vertex.  ScoreMesh: ScoreLabels with the
  // nearest triangle in place of the nearest point; per_voxel->nearest is a triangle's index.  Return the status (also
  // kept in last_status()); after a failure the mesh is not valid, *out is untouched and *per_voxel empty.  Replaces
  // scanneteval.py's nn_method="mesh" on a DownloadAll file.
  int MakeLabelMesh(const float* xyz, const uint8_t* labels, size_t n_vertices, const int32_t* tri, size_t n_triangles,
                    float cell, LabelMesh* out);
  int ScoreMesh(const LabelMesh& mesh, const ratsdf_score_params& params, ratsdf_label_score* out,
                std::vector<ratsdf_voxel_label>* per_voxel = nullptr);
  // map fusion (include/ratsdf_fuse.h): another grid's map (same device, voxel size and truncation; only read), n
  // blocks in ratsdf_import_blocks' layout, or a checkpoint file merged into this map with the weighted-average voxel
  // update.  stats may be nullptr.  Return the status (also kept in last_status()); no reference counterpart.
  int FuseMap(TSDFGrid& src, ratsdf_fuse_stats* stats = nullptr);
  int FuseBlocks(int32_t n, const int16_t* block_pos, const float* tsdf, const ratsdf_rgbw* rgbw, const float* prob,
                 ratsdf_fuse_stats* stats = nullptr);
  int FuseMapFile(const std::string& path, ratsdf_fuse_stats* stats = nullptr);
  // transformed map fusion (include/ratsdf_resample.h): another grid's map resampled onto this grid's lattice under
  // dst_T_src (p_dst = R(q) p_src + t, metres: a map-to-map pose, not a camera pose) and fused.  Return the status.
  int FuseMapTransformed(TSDFGrid& src, const ratsdf_pose& dst_T_src, ratsdf_fuse_stats* stats = nullptr);
  // map coarsening (include/ratsdf_coarsen.h): another grid's map of HALF this grid's voxel size (same device and
  // truncation; only read) coarsened by two and fused into this map.  Return the status.
  int FuseMapCoarsened(TSDFGrid& src, ratsdf_fuse_stats* stats = nullptr);
  int last_status() const { return status_; }
  ratsdf_engine* handle() { return engine_; }
  const Api& api() const { return *api_; }

 private:
  void note(int st, const char* what);
  // the guarded call of an optional entry point `f` on the engine: without an engine RATSDF_ERR_BAD_ARGUMENT, without
  // the entry point RATSDF_ERR_NOT_IMPLEMENTED, else its status, noted under `what`.  Returns last_status().
  template <class F, class... Args>
  int call(const char* what, F f, Args... args) {
    if (!engine_) return status_ = RATSDF_ERR_BAD_ARGUMENT;
    note(f ? f(engine_, args...) : RATSDF_ERR_NOT_IMPLEMENTED, what);
    return status_;
  }
  // a result buffer of the library into *out (when the call succeeded and *out is wanted), freed on every path
  template <class T>
  void take(T* buf, size_t n, std::vector<T>* out) {
    if (status_ == RATSDF_OK && out) out->assign(buf, buf + (buf ? n : 0));
    if (buf) api_->free_buffer(buf);
  }
  // the bodies of the three Gather*, SurfaceMesh / ClusterMesh, ScoreLabels / ScoreMesh and MakeLabelSet /
  // MakeLabelMesh (tsdf_host.cc)
  template <class T, class F, class... Args>
  std::vector<T> gather(const char* what, F f, Args... args);
  template <class F, class Params>
  int mesh(const char* what, F f, const int32_t origin[3], const int32_t dims[3], const Params& params,
           std::vector<ratsdf_surface_point>* vertices, std::vector<int32_t>* triangles);
  template <class F, class Labelled>
  int score(const char* what, F f, const Labelled& labelled, const ratsdf_score_params& params,
            ratsdf_label_score* out, std::vector<ratsdf_voxel_label>* per_voxel);
  template <class Labelled, class F, class... Args>
  int make_labelled(const char* what, Labelled* out, F f, Args... args);
  const Api* api_;
  ratsdf_engine* engine_ = nullptr;
  int status_ = 0;
};

}  // namespace ratsdf
