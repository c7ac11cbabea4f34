/*
 * ratsdf_surface_mesh.h -- the surface inside a box of the HIP engine's map as a welded, oriented, indexed triangle
 * mesh, compacted on the device: the surface points of ratsdf_surface.h as vertices, each exactly once, and the
 * marching-cubes triangles over them as indices.
 *
 * Kept apart from ratsdf.h because the CPU oracle does not implement these entry points (as ratsdf_surface.h).  No
 * reference counterpart: ratsdf_gather_valid_mesh stays the reference's mesh (whole map, weight > 10, an edge-length
 * filter, every block its own vertex lattice).
 *
 * The contract (bit-exact in the vertices, exact in the indices: a test restates it).  Every term not defined here
 * means what it means in ratsdf_surface.h: observed(w) with min_weight and the fresh-voxel exclusion, the edge (v, a)
 * owned by v, a crossing's f, pos, normal, the chosen endpoint, prob, rgbw.
 *   Cells      The cell of voxel v has the eight corners v + kCorner[i],
 *                kCorner = (0,0,0) (1,0,0) (1,0,1) (0,0,1) (0,1,0) (1,1,0) (1,1,1) (0,1,1)
 *              (corner 3 is (0,0,1), corner 4 is (0,1,0)).  A cell is IN THE BOX iff v is
 *              (origin[b] <= v[b] < origin[b] + dims[b]) and COMPLETE iff all eight corners are observed; a corner
 *              outside the int16 voxel range is never observed.  Its case is the sum over i of (t(corner i) < 0) << i:
 *              -0.0f and 0.0f are not negative.
 *   Triangles  A complete cell in the box emits the triangles of its case from the published 256-case table (cube
 *              edge e joins corners (0,1) (1,2) (2,3) (3,0) (4,5) (5,6) (6,7) (7,4) (0,4) (1,5) (2,6) (3,7)), in table
 *              order; an incomplete cell emits nothing.  No edge-length filter: a triangle of zero area (an endpoint's
 *              tsdf exactly 0) is kept, so the index topology stays closed.  A table triple of cube edges (e0, e1, e2)
 *              is written as the vertex indices of e0, e1, e2, in that order: with this corner numbering the table's
 *              own order winds towards free space (case 1 is "083": points on +x, +y, +z of corner 0, the negative
 *              one, and (p8 - p0) x (p3 - p0) points away from it), so (p1 - p0) x (p2 - p0) of an emitted triangle
 *              points into free space, as the vertex normals do.  Cube edge e of cell v is the lattice edge
 *              (v + lower corner of e, axis of e).
 *   Vertices   Every lattice edge (w, a) that is an edge of at least one complete cell in the box and whose endpoints
 *              differ in sign ((t(w) < 0) != (t(w + e_a) < 0)).  Every such edge is used by a triangle of that cell:
 *              no vertex is unreferenced, every index names a vertex.  Owners w lie in [origin, origin + dims] per
 *              axis, one voxel beyond the box on the upper side.  A vertex's record is the ratsdf_surface_point of
 *              that crossing, computed exactly as ratsdf_surface.h says, gradient neighbours included (whether or not
 *              they belong to a complete cell).  There is no min_prob: dropping a vertex would tear triangles.
 *   Order      Vertices in the order of ratsdf_surface.h: block z, y, x of the owner, then x + 8 y + 64 z within the
 *              block, then the axis.  Triangles in the same order of the cell's voxel v, then table order.  Indices
 *              are int32, three per triangle.
 *   Tiling     Boxes that tile space give every triangle exactly once.  A vertex on a shared face appears in both
 *              boxes' vertex lists, with identical bytes: each mesh is self-contained.
 * Limits, errors and side effects are those of ratsdf_surface.h: every dims[a] in [1, 1024]; dims[0] * dims[1] *
 * dims[2] <= 2^27; origin[a] and origin[a] + dims[a] - 1 in [-32768, 32767] (origin[a] + dims[a] may be 32768: that
 * voxel does not exist, so the cells touching it are incomplete).  Anything else is RATSDF_ERR_BAD_ARGUMENT, and so are
 * a NULL origin, dims or params, min_weight outside [1, 255], non-zero flags or reserved words, a NULL vertices,
 * n_vertices, triangles or n_triangles (host form), a negative capacity, a NULL buffer with a capacity > 0, a
 * d_vertices that is not 16-byte aligned, a d_triangles that is not 4-byte aligned and a d_counts that is NULL or not
 * 8-byte aligned (device form).  Nothing is launched then.
 * Both calls apply the last frame's deferred pool releases first, so a mesh taken right after a frame sees that
 * frame's map.  The map is only read (directory, pool, free list and directory-delta record stay as they are).  A
 * sticky engine error is returned, never hidden.  Workspace is engine-owned and grows on demand (1 KiB and a few words
 * per block position the box meets); a failed allocation is RATSDF_ERR_DEVICE (not sticky: the next call tries again).
 */
#ifndef RATSDF_SURFACE_MESH_H_
#define RATSDF_SURFACE_MESH_H_

#include "ratsdf_surface.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ratsdf_surface_mesh_params {
  int32_t min_weight; /* 1..255 */
  uint32_t flags;     /* must be 0 */
  uint32_t reserved0; /* must be 0 */
  uint32_t reserved1; /* must be 0 */
} ratsdf_surface_mesh_params;

/* origin: voxel index of the box's minimum corner; dims: voxels per axis.  Synchronous, host memory: *vertices
 * receives *n_vertices records and *triangles 3 * *n_triangles indices in the orders above, each owned by the caller
 * until ratsdf_free_buffer; an empty mesh is two NULLs and two zeros. */
int ratsdf_surface_mesh(ratsdf_engine* e, const int32_t origin[3], const int32_t dims[3],
                        const ratsdf_surface_mesh_params* params, ratsdf_surface_point** vertices,
                        size_t* n_vertices, int32_t** triangles, size_t* n_triangles);
/* Same on device pointers of the engine's device.  Asynchronous on the engine's stream, ordered after everything
 * enqueued on it before.  Writes the first min(total, capacity) records of each list (records beyond a capacity are
 * not touched) and the true totals as two int64 to d_counts: vertices, triangles.  A triangle written while one of its
 * vertices fell beyond vertex_capacity keeps its true index: the caller compares counts with capacities.  A capacity
 * of 0 with a NULL pointer is a pure count. */
int ratsdf_surface_mesh_device(ratsdf_engine* e, const int32_t origin[3], const int32_t dims[3],
                               const ratsdf_surface_mesh_params* params, void* d_vertices, int64_t vertex_capacity,
                               void* d_triangles, int64_t triangle_capacity, void* d_counts);

#ifdef __cplusplus
}
#endif
#endif /* RATSDF_SURFACE_MESH_H_ */
