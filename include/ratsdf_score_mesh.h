/*
 * ratsdf_score_mesh.h -- the map scored against a labelled triangle mesh: every near-surface voxel of the HIP engine's
 * map takes the label of its nearest ground-truth TRIANGLE, and the voxel's probability is counted against that label.
 * The second method of the reference's evaluation (python_utils/scannet_eval/scanneteval.py, nn_method="mesh":
 * pymesh.distance_to_mesh, lines 72-92, the face's label that of its first vertex, lines 83-90), on the device.  The
 * first method, the nearest labelled POINT, is ratsdf_score.h; the two differ wherever the mesh is coarser than the
 * voxels.  Parameters, score record and per-voxel record are those of ratsdf_score.h, reused unchanged.
 *
 * Kept apart from ratsdf.h because the CPU oracle does not implement these entry points (as ratsdf_score.h).
 *
 * 1. A mesh set: n_vertices points with a label each (RATSDF_LABEL_IGNORE / LOW / HIGH) and n_triangles index triples
 *    (tri[3 t + k], k = 0..2), built once, immutable, kept on the device of the creating engine.  Lifetime and device
 *    rules are those of a label set (ratsdf_score.h 1.): creation is synchronous; any engine of the same device may
 *    score against it; destroy it before the process ends its device and not while a scoring call may still be queued.
 *    RATSDF_ERR_BAD_ARGUMENT, with nothing left allocated, for: n_vertices or n_triangles > 2^26; an index outside
 *    [0, n_vertices) in any triangle; a label above 2 on any vertex, used or not (the device form counts both in its
 *    build kernel, which tests an index before it loads through it, and reads the counts back); a NaN, negative or
 *    infinite cell; a NULL xyz or labels with n_vertices > 0, a NULL tri with n_triangles > 0; a NULL out.
 *    n_vertices == 0 or n_triangles == 0 is a valid, empty set.
 *    A triangle is KEPT iff its nine coordinates are finite and no two of its vertices compare equal in all three
 *    coordinates (fp32 ==, so -0.0 == 0.0).  The others are dropped: they can never be nearest, and the indices of the
 *    rest stay the original ones.  The label of triangle t is labels[tri[3 t]], that of its first vertex.
 *    The kept triangles are held in a dense grid of cubic cells over the bounding box of their vertices (origin = its
 *    lower corner, cells[a] = floor((max[a] - min[a]) / cell) + 1, cell indices floor((x - origin) / cell), all in
 *    double precision).  A triangle is referenced from every cell its axis-aligned box meets; refs is the number of
 *    such references, the sum over kept triangles of the product of their box's cell spans.  cell == 0 asks for
 *    8 * voxel_size of the creating engine; the edge is doubled until it is at least 1e-6, the grid has at most 2^24
 *    cells and refs <= RATSDF_LABELMESH_MAX_REFS (a memory bound: four bytes per reference).  info reports what was
 *    used (an empty set: cells = {1, 1, 1}, origin = {0, 0, 0}, refs = 0).  The grid only accelerates the search: no
 *    result below depends on it.
 *
 * 2. Scoring (bit-exact: tests/score_mesh_ref.py restates it).  Voxels, their order, their position
 *    (float)grid_index * voxel_size, the selection rule, the prediction rule, the bins, the per-voxel defaults (-1 and
 *    -2 with the quiet NaN) and the score's fields and identities are those of ratsdf_score.h 2., word for word;
 *    `nearest` is a triangle's original index.
 *    The distance, fp32, evaluated as written, no contraction, correctly rounded division;
 *    dot(u, v) = (ux * vx + uy * vy) + uz * vz.  With voxel position p and triangle a, b, c the first case that holds
 *    decides (Ericson, Real-Time Collision Detection 5.1.5, with a final clamp added):
 *        ab = b - a, ac = c - a, ap = p - a;   d1 = dot(ab, ap), d2 = dot(ac, ap)
 *          if d1 <= 0 && d2 <= 0:                     q = a
 *        bp = p - b;   d3 = dot(ab, bp), d4 = dot(ac, bp)
 *          if d3 >= 0 && d4 <= d3:                    q = b
 *        vc = d1 * d4 - d3 * d2
 *          if vc <= 0 && d1 >= 0 && d3 <= 0:          v = d1 / (d1 - d3);                 q = a + v * ab
 *        cp = p - c;   d5 = dot(ab, cp), d6 = dot(ac, cp)
 *          if d6 >= 0 && d5 <= d6:                    q = c
 *        vb = d5 * d2 - d1 * d6
 *          if vb <= 0 && d2 >= 0 && d6 <= 0:          w = d2 / (d2 - d6);                 q = a + w * ac
 *        va = d3 * d6 - d5 * d4;  e1 = d4 - d3;  e2 = d5 - d6
 *          if va <= 0 && e1 >= 0 && e2 >= 0:          w = e1 / (e1 + e2);                 q = b + w * (c - b)
 *          otherwise:  den = 1 / ((va + vb) + vc);  v = vb * den;  w = vc * den;          q = (a + ab * v) + ac * w
 *        per axis:  lo = min(a, b, c), hi = max(a, b, c);   q = q < lo ? lo : (q > hi ? hi : q)   (a NaN stays a NaN)
 *        d = q - p;   dist2 = dot(d, d)
 *    The nearest triangle minimises (dist2, original index) lexicographically among the kept triangles with
 *    dist2 <= max_dist * max_dist (the fp32 product); a NaN dist2 never satisfies that.
 *
 * Host and device forms, alignment rules, capacity == 0 as a pure count, the settle step, read-only access to the map
 * and the sticky engine error are those of ratsdf_score_labels / ratsdf_score_labels_device, and so is the list of
 * refused arguments (RATSDF_ERR_BAD_ARGUMENT, nothing launched, nothing written), with max_dist bounded by 64 cells of
 * the mesh set.
 */
#ifndef RATSDF_SCORE_MESH_H_
#define RATSDF_SCORE_MESH_H_

#include "ratsdf_score.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RATSDF_LABELMESH_MAX_REFS 33554432 /* 2^25 cell references: 128 MiB */

typedef struct ratsdf_labelmesh ratsdf_labelmesh;

typedef struct ratsdf_labelmesh_info { /* 72 bytes */
  int64_t vertices;  /* vertices given */
  int64_t triangles; /* triangles given */
  int64_t kept;      /* triangles with nine finite coordinates and three distinct vertices */
  int64_t mixed;     /* kept triangles whose three vertex labels are not all equal (scanneteval.py's TODO) */
  int64_t refs;      /* cell references: sum over kept triangles of the cells their boxes meet */
  float cell;        /* cell edge actually used, metres */
  float origin[3];   /* lower corner of the grid */
  int32_t cells[3];
  uint32_t reserved;
} ratsdf_labelmesh_info;

int ratsdf_labelmesh_create(ratsdf_engine* e, const float* xyz, const uint8_t* labels, size_t n_vertices,
                            const int32_t* tri, size_t n_triangles, float cell, ratsdf_labelmesh** out);
int ratsdf_labelmesh_create_device(ratsdf_engine* e, const void* d_xyz, const void* d_labels, size_t n_vertices,
                                   const void* d_tri, size_t n_triangles, float cell, ratsdf_labelmesh** out);
int ratsdf_labelmesh_info_get(const ratsdf_labelmesh* m, ratsdf_labelmesh_info* out);
int ratsdf_labelmesh_destroy(ratsdf_labelmesh* m);

int ratsdf_score_mesh(ratsdf_engine* e, const ratsdf_labelmesh* m, const ratsdf_score_params* p,
                      ratsdf_label_score* out, ratsdf_voxel_label** per_voxel /* may be NULL */, size_t* n);
int ratsdf_score_mesh_device(ratsdf_engine* e, const ratsdf_labelmesh* m, const ratsdf_score_params* p, void* d_score,
                             void* d_per_voxel /* may be NULL */, int64_t capacity, void* d_count);

#ifdef __cplusplus
}
#endif
#endif /* RATSDF_SCORE_MESH_H_ */
