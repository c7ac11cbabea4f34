// map_read.h -- what the kernels that only READ the map share: which pool block a block position names, the range
// tests of the grid, the trilinear sample of the sampling contract, and the box of the read-outs that take one.  The
// kernels that need the entry's index or write the directory keep find_block (kernels_alloc.h).
#pragma once
#include "kernels_alloc.h"

namespace ratsdf {

// The pool index of block (x, y, z), -1 if absent: the chain walk of find_block from the home pair (entries e0 and
// e0 + 1) already loaded -- a kernel that needs several blocks loads all their pairs back to back first (k_sample).
// An entry left pending by a failed frame, kPlaceholderIdx, names no pool block: absent, never read (every reader
// turns an entry into a pool index here and nowhere else).
__device__ inline int32_t resolve_block(const Table& t, int x, int y, int z, uint32_t e0, const EntryWords& a,
                                        const EntryWords& b) {
  const uint32_t k0 = key0(x, y), k1 = key1(z);
  int32_t r = -1;
  if (entry_matches(a, k0, k1)) {
    r = a.idx;
  } else if (entry_matches(b, k0, k1)) {
    r = b.idx;
  } else {
    uint32_t last = e0 + 1;
    int off = entry_offset(b);
    uint32_t guard = 0;
    while (off && guard++ < t.num_entry) {
      last = (last + (uint32_t)off) & t.entry_mask;
      const EntryWords w = load_entry(t.entries, last);
      if (entry_matches(w, k0, k1)) {
        r = w.idx;
        break;
      }
      off = entry_offset(w);
    }
  }
  return r < t.num_block ? r : -1;
}
// ... with the probe of the home pair
__device__ inline int32_t lookup_block(const Table& t, int x, int y, int z) {
  const uint32_t e0 = block_hash(x, y, z, t.bucket_mask) << 1;
  return resolve_block(t, x, y, z, e0, load_entry(t.entries, e0), load_entry(t.entries, e0 + 1));
}

// A block position inside the grid of int16 voxels.  The directory keys 16 bits per axis: a position outside would
// wrap around onto a real block, so a caller that can step outside asks this first.
__device__ inline bool block_in_grid(int x, int y, int z) {
  return x >= -4096 && x <= 4095 && y >= -4096 && y <= 4095 && z >= -4096 && z <= 4095;
}
// The floors of a sample position (in voxels) whose eight corners all lie inside the grid (a NaN fails every
// comparison; +-inf fails one): no wrap-around onto a real block.
__device__ inline bool cell_in_grid(float lxf, float lyf, float lzf) {
  return lxf >= -32768.f && lxf <= 32766.f && lyf >= -32768.f && lyf <= 32766.f && lzf >= -32768.f && lzf <= 32766.f;
}

// The trilinear sample of corners t000 .. t111 (t[4 i + 2 j + k]: x + i, y + j, z + k) at fractions f, u = 1 - f: the
// contract of include/ratsdf_sample.h, evaluated as written (-ffp-contract=off).  The intermediates are what the
// gradient of k_sample is made of.
struct Trilinear {
  float c00, c01, c10, c11, c0, c1, value;
};
__device__ inline Trilinear trilinear(const float (&t)[8], float fx, float fy, float fz, float ux, float uy,
                                      float uz) {
  Trilinear r;
  r.c00 = t[0] * uz + t[1] * fz, r.c01 = t[2] * uz + t[3] * fz;
  r.c10 = t[4] * uz + t[5] * fz, r.c11 = t[6] * uz + t[7] * fz;
  r.c0 = r.c00 * uy + r.c01 * fy, r.c1 = r.c10 * uy + r.c11 * fy;
  r.value = r.c0 * ux + r.c1 * fx;
  return r;
}

// A box of voxels and a grid of map blocks over it, x fastest: the cells of the read-outs that take a box (the ESDF,
// the surface points, the welded mesh, the regions).  The block grid is the caller's choice: map_box() sets the blocks
// the box meets, the welded mesh widens it to the blocks of its vertex owners (surface_mesh_box).
struct MapBox {
  int ox, oy, oz;     // voxel index of the minimum corner
  int X, Y, Z;        // voxels per axis
  int bx0, by0, bz0;  // the first map block of the grid
  int nbx, nby, nbz;  // map blocks per axis
};
inline size_t box_cells(const MapBox& b) {  // (host) cells of the box's block grid: one workgroup each
  return (size_t)b.nbx * (size_t)b.nby * (size_t)b.nbz;
}

// (host) the box of an entry point's origin and dims, *n its voxels; false (RATSDF_ERR_BAD_ARGUMENT) unless every voxel
// lies in the int16 range, no axis has more than 1024 and the box no more than kBoxMaxVoxels
constexpr size_t kBoxMaxVoxels = (size_t)1 << 27;
inline bool map_box(const int32_t* origin, const int32_t* dims, MapBox* b, size_t* n) {
  if (!origin || !dims) return false;
  size_t m = 1;
  for (int a = 0; a < 3; ++a) {
    if (dims[a] < 1 || dims[a] > 1024 || origin[a] < -32768 || (int64_t)origin[a] + dims[a] - 1 > 32767) return false;
    m *= (size_t)dims[a];
  }
  if (m > kBoxMaxVoxels) return false;
  b->ox = origin[0], b->oy = origin[1], b->oz = origin[2];
  b->X = dims[0], b->Y = dims[1], b->Z = dims[2];
  b->bx0 = origin[0] >> 3, b->by0 = origin[1] >> 3, b->bz0 = origin[2] >> 3;
  b->nbx = ((origin[0] + dims[0] - 1) >> 3) - b->bx0 + 1;
  b->nby = ((origin[1] + dims[1] - 1) >> 3) - b->by0 + 1;
  b->nbz = ((origin[2] + dims[2] - 1) >> 3) - b->bz0 + 1;
  *n = m;
  return true;
}

}  // namespace ratsdf
