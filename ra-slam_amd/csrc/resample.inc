// resample.inc -- transformed map fusion (include/ratsdf_resample.h): the host side of kernels_resample.h.  Included at
// the end of ratsdf_engine.hip, behind fuse.inc (the resampled records go through fuse_chunk).
#include "../../include/ratsdf_resample.h"

namespace {

static_assert(kMapChunk <= kFuseChunk, "a staging chunk of resampled records is one chunk of fuse_chunk");

// every component finite, the quaternion a unit one within 1e-3 of its squared norm
static bool resample_pose_ok(const ratsdf_pose* T) {
  if (!T) return false;
  const float v[7] = {T->qx, T->qy, T->qz, T->qw, T->tx, T->ty, T->tz};
  for (float x : v)
    if (!std::isfinite(x)) return false;
  const double n2 = (double)T->qx * T->qx + (double)T->qy * T->qy + (double)T->qz * T->qz + (double)T->qw * T->qw;
  return std::fabs(n2 - 1.0) <= 1e-3;
}

// G of the contract: the inverse pose in voxel units (fp32, as written there)
static Se3 resample_transform(const ratsdf_pose* T, float vs) {
  const Se3 Ti = se3_inverse(Se3{Quat{T->qx, T->qy, T->qz, T->qw}, V3{T->tx, T->ty, T->tz}});
  return Se3{Ti.q, V3{Ti.t.x / vs, Ti.t.y / vs, Ti.t.z / vs}};
}

static int resample_launch(ratsdf_engine* src, hipStream_t stream, const Se3& G, int32_t n, const int16_t* d_pos,
                           uint32_t* d_rec, int32_t* d_contrib) {
  hipLaunchKernelGGL(k_resample_blocks, dim3((unsigned)n), dim3(512), 0, stream, src->tab, src->pool, G, d_pos, d_rec,
                     d_contrib);
  HIPCHK(hipGetLastError());
  return RATSDF_OK;
}

// The destination blocks that can hold a contributing voxel, sorted and distinct, as n x 3 int16.
//
// The kernel maps a destination voxel d to g = A d + c with A the linear map of quat_rotate(G.q, .) and c = G.t; the
// forward transform is its inverse, d = A^-1 (g - c), taken here from the very G the kernel gets (in double), so the
// two agree whatever the quaternion's norm.  A voxel can contribute from source block b only if a needed corner lies
// in b, i.e. g inside the open reach (8b - 1, 8b + 8) per axis; a linear map takes that box to a parallelepiped inside
// the axis-aligned box of its 8 corners.  The margin covers the kernel's fp32 evaluation of g: about ten roundings of
// intermediates no larger than 4 |d| + |c|, under 40 ulp = 2.4e-6 of the largest coordinate M involved, times
// |A^-1|_inf <= 1.75 -- 8e-6 M is twice that -- and 0.01 voxel on top for the double arithmetic here.
static std::vector<int16_t> resample_candidates(const Se3& G, const std::vector<ratsdf_block>& blocks,
                                                int32_t src_num_block) {
  std::vector<int16_t> out;
  const double q[4] = {G.q.x, G.q.y, G.q.z, G.q.w}, c[3] = {G.t.x, G.t.y, G.t.z};
  if (!std::isfinite(c[0]) || !std::isfinite(c[1]) || !std::isfinite(c[2])) return out;  // (no voxel is in range)
  auto rotate = [&](const double v[3], double r[3]) {  // quat_rotate in double
    double uv[3] = {q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]};
    for (double& x : uv) x += x;
    const double cc[3] = {q[1] * uv[2] - q[2] * uv[1], q[2] * uv[0] - q[0] * uv[2], q[0] * uv[1] - q[1] * uv[0]};
    for (int i = 0; i < 3; ++i) r[i] = v[i] + q[3] * uv[i] + cc[i];
  };
  double A[3][3], Ai[3][3];  // A[row][col]
  for (int j = 0; j < 3; ++j) {
    const double e[3] = {j == 0 ? 1.0 : 0.0, j == 1 ? 1.0 : 0.0, j == 2 ? 1.0 : 0.0};
    double r[3];
    rotate(e, r);
    for (int i = 0; i < 3; ++i) A[i][j] = r[i];
  }
  const double det = A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0]) +
                     A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0]);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {  // adjugate / det
      const int a = (j + 1) % 3, b = (j + 2) % 3, cc = (i + 1) % 3, d = (i + 2) % 3;
      Ai[i][j] = (A[a][cc] * A[b][d] - A[a][d] * A[b][cc]) / det;
    }
  double cmax = std::max({std::fabs(c[0]), std::fabs(c[1]), std::fabs(c[2])});
  std::vector<uint64_t> keys;
  for (const ratsdf_block& bl : blocks) {
    if (bl.idx < 0 || bl.idx >= src_num_block) continue;  // (a pending entry names no block)
    const int b3[3] = {bl.x, bl.y, bl.z};
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300}, M = cmax;
    for (int k = 0; k < 8; ++k) {
      double gc[3], d[3];
      for (int a = 0; a < 3; ++a) {
        const double gk = 8.0 * b3[a] + (((k >> a) & 1) ? 8.0 : -1.0);
        M = std::max(M, std::fabs(gk));
        gc[a] = gk - c[a];
      }
      for (int a = 0; a < 3; ++a) {
        d[a] = Ai[a][0] * gc[0] + Ai[a][1] * gc[1] + Ai[a][2] * gc[2];
        lo[a] = std::min(lo[a], d[a]);
        hi[a] = std::max(hi[a], d[a]);
        M = std::max(M, std::fabs(d[a]));
      }
    }
    const double margin = 0.01 + 8e-6 * M;
    int bl_lo[3], bl_hi[3];
    bool some = true;
    for (int a = 0; a < 3; ++a) {
      // integer voxels of the padded box, clipped to the grid before they become integers
      const double vlo = std::ceil(std::max(lo[a] - margin, -32768.0)), vhi = std::floor(std::min(hi[a] + margin, 32767.0));
      if (!(vlo <= vhi)) {  // (also a NaN)
        some = false;
        break;
      }
      bl_lo[a] = (int)vlo >> 3;
      bl_hi[a] = (int)vhi >> 3;
    }
    if (!some) continue;
    for (int z = bl_lo[2]; z <= bl_hi[2]; ++z)
      for (int y = bl_lo[1]; y <= bl_hi[1]; ++y)
        for (int x = bl_lo[0]; x <= bl_hi[0]; ++x)
          keys.push_back((uint64_t)(z + 4096) << 26 | (uint64_t)(y + 4096) << 13 | (uint64_t)(x + 4096));
    if (keys.size() > ((size_t)1 << 22)) {  // (keep the list near its distinct size)
      std::sort(keys.begin(), keys.end());
      keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    }
  }
  std::sort(keys.begin(), keys.end());
  keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
  out.reserve(keys.size() * 3);
  for (uint64_t k : keys) {
    out.push_back((int16_t)((int)(k & 8191u) - 4096));
    out.push_back((int16_t)((int)((k >> 13) & 8191u) - 4096));
    out.push_back((int16_t)((int)((k >> 26) & 8191u) - 4096));
  }
  return out;
}

// The source of a record-producing fusion: settled, sound, its live entries on the host (control data, read as
// ratsdf_dump_directory reads them; no voxel crosses).  The source's stream is idle when this returns.
static int fuse_source_blocks(ratsdf_engine* src, std::vector<ratsdf_block>* blocks) {
  STCHK(src->settle());
  STCHK(src->sticky());
  STCHK(src->select(kSelValid, GridBounds{}, &src->ctl->n_sel));
  uint32_t n_sel = 0;
  STCHK(src->read_small(&n_sel, &src->ctl->n_sel, 4));
  if (n_sel > src->vis_cap) return RATSDF_ERR_CAPACITY;
  blocks->resize(n_sel);
  if (n_sel == 0) return RATSDF_OK;
  std::vector<int32_t> entry(n_sel);
  return dump_selected_entries(src, n_sel, blocks->data(), entry.data());
}

// Candidate blocks of the destination lattice (n x 3 int16) turned into records by `launch(stream, m, d_pos, d_rec,
// d_contrib)` in chunks of kMapChunk and fused: the empty ones dropped (k_resample_mark), the others through fuse_chunk.
// Staging: the records of one chunk and their counts, made on the destination's stream (the source is settled and
// idle), so the record path follows in stream order.
template <class Launch>
static int fuse_candidate_records(ratsdf_engine* dst, const std::vector<int16_t>& cand, Launch launch,
                                  ratsdf_fuse_stats* stats) {
  ratsdf_fuse_stats acc;
  memset(&acc, 0, sizeof(acc));
  const size_t n_cand = cand.size() / 3;
  if (n_cand == 0) {  // nothing to launch
    STCHK(dst->settle());
    return dst->sticky();
  }
  FuseScratch s;
  int32_t free_before = 0;
  STCHK(fuse_begin(dst, &s, &free_before));
  DevMem stage, counts;
  StreamDrain drain{dst->stream};
  STCHK(stage.alloc((size_t)kMapChunk * kMapRecordBytes));
  STCHK(counts.alloc((size_t)kMapChunk * 4));
  uint32_t* rec = stage.as<uint32_t>();
  int st = RATSDF_OK;
  for (size_t first = 0; first < n_cand && st == RATSDF_OK; first += kMapChunk) {
    const int32_t m = (int32_t)std::min<size_t>(kMapChunk, n_cand - first);
    if (hipMemcpyAsync(s.pos, cand.data() + first * 3, (size_t)m * 6, hipMemcpyHostToDevice, dst->stream) != hipSuccess) {
      st = RATSDF_ERR_DEVICE;
      break;
    }
    st = fuse_clear(dst, s);
    if (st != RATSDF_OK) break;
    st = launch(dst->stream, m, s.pos, rec, counts.as<int32_t>());
    if (st != RATSDF_OK) break;
    hipLaunchKernelGGL(k_resample_mark, dim3(((unsigned)m + 255u) / 256u), dim3(256), 0, dst->stream,
                       counts.as<int32_t>(), (uint32_t)m, s.done, s.cnt);
    uint32_t listed = 0;  // (control data: 4 bytes per chunk; a chunk of empty candidates needs no allocation pass)
    st = dst->read_small(&listed, &s.cnt->listed, 4);
    if (st != RATSDF_OK || listed == 0) continue;
    acc.blocks_seen += listed;
    st = fuse_chunk(dst, s, m, s.pos, nullptr, rec, rec + 512, rec + 1024, 1536u, &acc);
  }
  return fuse_end(dst, st, free_before, &acc, stats);
}

}  // namespace

extern "C" {

int ratsdf_resample_blocks_device(ratsdf_engine* src, const ratsdf_pose* dst_T_src, int32_t n, const void* d_block_pos,
                                  void* d_voxels, void* d_contrib) {
  ENTRY(src, n >= 0 && resample_pose_ok(dst_T_src) && (n == 0 || (d_block_pos && d_voxels)) &&
                 ((uintptr_t)d_voxels & 15u) == 0 && ((uintptr_t)d_contrib & 3u) == 0);
  STCHK(src->settle());
  STCHK(sticky_raised(src));
  if (n == 0) return RATSDF_OK;
  return resample_launch(src, src->stream, resample_transform(dst_T_src, src->vs), n, (const int16_t*)d_block_pos,
                         (uint32_t*)d_voxels, (int32_t*)d_contrib);
}

int ratsdf_fuse_map_transformed(ratsdf_engine* dst, ratsdf_engine* src, const ratsdf_pose* dst_T_src,
                                ratsdf_fuse_stats* stats) {
  ENTRY(dst, src && dst != src && dst->device == src->device && memcmp(&dst->vs, &src->vs, 4) == 0 &&
                 memcmp(&dst->trunc, &src->trunc, 4) == 0 && resample_pose_ok(dst_T_src));
  if (stats) memset(stats, 0, sizeof(*stats));
  std::vector<ratsdf_block> blocks;
  STCHK(fuse_source_blocks(src, &blocks));
  const Se3 G = resample_transform(dst_T_src, src->vs);
  // (an empty source, or one wholly outside the destination's grid, has no candidates: nothing is launched)
  return fuse_candidate_records(
      dst, resample_candidates(G, blocks, src->tab.num_block),
      [&](hipStream_t stream, int32_t m, const int16_t* d_pos, uint32_t* d_rec, int32_t* d_contrib) {
        return resample_launch(src, stream, G, m, d_pos, d_rec, d_contrib);
      },
      stats);
}

}  // extern "C"
