/*
 * ratsdf_cluster_mesh.h -- the surface inside a box of the HIP engine's map as a CLUSTERED triangle mesh, compacted on
 * the device: the welded mesh of ratsdf_surface_mesh.h for the same box and min_weight, its vertices merged per
 * lattice-aligned cluster of k x k x k voxels (k = 2, 4 or 8), its triangles re-indexed, the degenerate ones dropped
 * and the duplicates removed.  A tenth to a hundredth of the welded mesh, for a planner, a viewer or a network link.
 *
 * Kept apart from ratsdf.h because the CPU oracle does not implement these entry points (as ratsdf_surface_mesh.h).
 * The reference simplifies its exported mesh on the host (Open3D's vertex clustering, average contraction).  This is
 * NOT that output byte for byte: Open3D's grid hangs on the mesh's bounding box and its sums run in hash order.  The
 * shared semantics are the average contraction, the dropped degenerate triangles, the smallest-first rotation and the
 * duplicate removal.
 *
 * The contract (bit-exact in the vertices, exact in the indices: a test restates it).  Every term not defined here
 * means what it means in ratsdf_surface.h / ratsdf_surface_mesh.h.  All arithmetic is fp32, evaluated as written, no
 * contraction, sqrtf and division correctly rounded, denormals kept.
 *   Inputs     (V, T): the vertices and triangles of ratsdf_surface_mesh.h for this box and min_weight, in their
 *              orders.  A vertex is a lattice edge (w, a) with f = t0 / (t0 - t1); its chosen endpoint is
 *              u = w + e_a iff f >= 0.5f, else w (ratsdf_surface.h).  u is a corner of a complete cell in the box, so it
 *              is an existing voxel in [origin, origin + dims].
 *   Clusters   s = log2 k.  The cluster of voxel u is q = (u[0] >> s, u[1] >> s, u[2] >> s), the shift arithmetic
 *              (floor, also for negative indices); its base voxel is base = q << s.  k divides 8: a cluster lies inside
 *              one voxel block.  A vertex is a MEMBER of the cluster of its chosen endpoint.
 *   Vertices   One ratsdf_surface_point per cluster with at least one member; n is its member count.  Per member the
 *              summed quantities are rel[a] = (float)(w[a] - base[a]) + f and rel[b] = (float)(w[b] - base[b]) for the
 *              two other axes (w[a] - base[a] may be -1), the three components of its normal as ratsdf_surface.h
 *              computes them, its prob, and, as integers, r, g, b, weight of its rgbw.
 *              Per voxel u of the cluster S(u) starts at 0.0f and the members whose chosen endpoint is u are added one
 *              after the other in the order (u - e_0, 0), (u, 0), (u - e_1, 1), (u, 1), (u - e_2, 2), (u, 2); a voxel
 *              without members keeps 0.0f.  Over the k^3 voxels with local index j = x + k y + k^2 z (local
 *              coordinates u & (k - 1)) the sums combine as a fixed binary tree: for level l = 0 .. 3 s - 1 every j
 *              with bit l clear becomes S[j] + S[j | (1 << l)], the lower index as the LEFT operand; the cluster's sum
 *              is S[0] after the last level (what a lane-xor butterfly computes: x bits, then y bits, then z bits).  A
 *              sequential sum is NOT this contract.
 *                pos[b]    = ((float)base[b] + Srel[b] / (float)n) * vs
 *                len       = sqrtf(N0 * N0 + N1 * N1 + N2 * N2), N the summed normals
 *                normal[b] = N[b] / len, or all three 0.0f when len is 0 or not finite
 *                prob      = Sprob / (float)n
 *                r, g, b, weight: each (2 * sum + n) / (2 * n) in unsigned integer arithmetic (the rounded mean;
 *                n <= 3072, the sums fit 32 bits)
 *   Order      Clusters ascend by block z, then block y, then block x (block = q >> (3 - s)), then within a block by
 *              lx + (8/k) ly + (8/k)^2 lz with l = q & (8/k - 1).  A cluster's vertex index is its rank in this order
 *              among the non-empty clusters.  Unlike the welded mesh a vertex may be unreferenced (a component that
 *              lies wholly inside one cluster); it is kept, as Open3D keeps it.
 *   Triangles  Every triangle of T becomes the triple of its vertices' cluster indices.  It is DROPPED iff two of the
 *              three are equal; otherwise it is rotated cyclically so that its smallest index comes first (the winding
 *              is kept), and identical triples after rotation are emitted once.  (a, b, c) and (a, c, b) are different
 *              triangles and both stay.  The three clusters of one triangle are clusters of corners of one cell, so the
 *              second and the third differ from the first by -1, 0 or +1 per axis in cluster coordinates; with
 *              code(d) = (d0 + 1) + 3 (d1 + 1) + 9 (d2 + 1) the output ascends in the first index, then
 *              code(q_second - q_first), then code(q_third - q_first).  Indices are int32, three per triangle.
 *   Box edges  The result is a function of THIS box's welded mesh alone: a cluster that the box cuts averages only the
 *              members this box has.  Meshes of boxes that tile space therefore do not stitch byte for byte; a caller
 *              who wants one mesh takes one box.
 * Limits, errors and side effects are those of ratsdf_surface_mesh.h: every dims[a] in [1, 1024]; dims[0] * dims[1] *
 * dims[2] <= 2^27; origin[a] and origin[a] + dims[a] - 1 in [-32768, 32767] (origin[a] + dims[a] may be 32768: that
 * voxel does not exist, so the cells touching it are incomplete).  Anything else is RATSDF_ERR_BAD_ARGUMENT, and so are
 * a NULL origin, dims or params, min_weight outside [1, 255], a factor not in {2, 4, 8}, non-zero flags or a non-zero
 * reserved word, a NULL vertices, n_vertices, triangles or n_triangles (host form), a negative capacity, a NULL buffer
 * with a capacity > 0, a d_vertices that is not 16-byte aligned, a d_triangles that is not 4-byte aligned and a
 * d_counts that is NULL or not 8-byte aligned (device form).  Nothing is launched then.
 * Both calls apply the last frame's deferred pool releases first, so a mesh taken right after a frame sees that
 * frame's map.  The map is only read (directory, pool, free list and directory-delta record stay as they are).  A
 * sticky engine error is returned, never hidden.  Workspace is engine-owned and grows on demand (a few words per block
 * position the box meets); a failed allocation is RATSDF_ERR_DEVICE (not sticky: the next call tries again).
 */
#ifndef RATSDF_CLUSTER_MESH_H_
#define RATSDF_CLUSTER_MESH_H_

#include "ratsdf_surface_mesh.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ratsdf_cluster_mesh_params {
  int32_t min_weight; /* 1..255 */
  int32_t factor;     /* k: 2, 4 or 8 voxels per cluster edge */
  uint32_t flags;     /* must be 0 */
  uint32_t reserved;  /* must be 0 */
} ratsdf_cluster_mesh_params;

/* origin: voxel index of the box's minimum corner; dims: voxels per axis.  Synchronous, host memory: *vertices
 * receives *n_vertices records and *triangles 3 * *n_triangles indices in the orders above, each owned by the caller
 * until ratsdf_free_buffer; an empty mesh is two NULLs and two zeros. */
int ratsdf_cluster_mesh(ratsdf_engine* e, const int32_t origin[3], const int32_t dims[3],
                        const ratsdf_cluster_mesh_params* params, ratsdf_surface_point** vertices,
                        size_t* n_vertices, int32_t** triangles, size_t* n_triangles);
/* Same on device pointers of the engine's device.  Asynchronous on the engine's stream, ordered after everything
 * enqueued on it before.  Writes the first min(total, capacity) records of each list (records beyond a capacity are
 * not touched) and the true totals as two int64 to d_counts: vertices, triangles.  A triangle written while one of its
 * vertices fell beyond vertex_capacity keeps its true index: the caller compares counts with capacities.  A capacity
 * of 0 with a NULL pointer is a pure count. */
int ratsdf_cluster_mesh_device(ratsdf_engine* e, const int32_t origin[3], const int32_t dims[3],
                               const ratsdf_cluster_mesh_params* params, void* d_vertices, int64_t vertex_capacity,
                               void* d_triangles, int64_t triangle_capacity, void* d_counts);

#ifdef __cplusplus
}
#endif
#endif /* RATSDF_CLUSTER_MESH_H_ */
