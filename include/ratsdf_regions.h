/*
 * ratsdf_regions.h -- connected regions of a box of the HIP engine's map: which voxels of a chosen kind hang
 * together, as a label per voxel and a table of the regions with size, bounding box, the box faces they reach and
 * the number of their voxels that border unobserved space.  What a planner asks after the ESDF: which free voxels
 * connect to the robot's (reachability), where reachable free space meets unknown space (frontiers), which occupied
 * voxels form one object (speckle removal, high-touch targets with prob >= p).
 *
 * Kept apart from ratsdf.h because the CPU oracle does not implement these entry points (as ratsdf_esdf.h).  No
 * reference counterpart.
 *
 * The contract (bit-exact: a test restates it).  The box, its limits and the index
 *   i = (x - ox) + X * ((y - oy) + Y * (z - oz))          (X, Y, Z = dims; ox, oy, oz = origin)
 * are those of ratsdf_esdf.h: every dims[a] in [1, 1024], dims[0] * dims[1] * dims[2] <= 2^27, origin[a] and
 * origin[a] + dims[a] - 1 in the int16 voxel range.  Only the voxels of the box exist.
 *   state(v)   ratsdf_esdf.h's state of voxel v (UNKNOWN, FREE or OCCUPIED) with params->occupied_below
 *   p(v)       the map's probability word of v if state(v) is FREE or OCCUPIED; 0.0f if it is UNKNOWN, whatever the
 *              pool holds
 *   member(v)  bit state(v) of params->states is set, and not p(v) < params->min_prob (fp32 comparison as written,
 *              as ratsdf_surface.h drops points: a NaN probability is kept; min_prob = 0 keeps everything the mask
 *              admits)
 *   Regions    the classes of the members under face adjacency (6 neighbours) between voxels that are BOTH inside
 *              the box.  Members that touch only through an edge, a corner or a voxel outside the box are different
 *              regions.
 *   Labels     labels[i] = -1 for a non-member, otherwise the smallest box index of its region (the region's root).
 *   Table      one ratsdf_region per region, ascending in root.  voxels: its members.  frontier: its members with at
 *              least one face neighbour INSIDE the box whose state is UNKNOWN -- a member counts once however many
 *              such neighbours it has, an UNKNOWN neighbour counts whether or not it is itself a member, neighbours
 *              outside the box do not count.  faces: bit 2a is set if a member has v[a] == origin[a], bit 2a + 1 if
 *              a member has v[a] == origin[a] + dims[a] - 1.  lo / hi: the bounding box of the members, absolute
 *              voxel indices, inclusive.  reserved is written as 0.
 * The result does not depend on scheduling: all of it is integers, defined by the map alone.
 *
 * Host form: labels (may be NULL) receives X * Y * Z int32; *out / *n receive the table in a buffer for
 * ratsdf_free_buffer (NULL / 0 when there is no region).  Synchronous.
 * Device form: d_labels (may be NULL; 16-byte aligned) receives the labels; the first min(total, capacity) records go
 * to d_regions (16-byte aligned; records at capacity and beyond are untouched) and the total as an int64 to d_count
 * (8-byte aligned).  capacity == 0 with a NULL d_regions is a pure count.  Asynchronous on the engine's stream, ordered
 * after everything enqueued on it before.
 *
 * RATSDF_ERR_BAD_ARGUMENT, with nothing launched, for: a box ratsdf_esdf refuses; a NULL origin, dims or params; a
 * NaN occupied_below or min_prob; states == 0 or states > 7; non-zero flags (18- and 26-connectivity are not
 * implemented: the bits stay reserved); a NULL out or n (host form); a negative capacity, a NULL d_regions with
 * capacity > 0, a misaligned pointer, a NULL d_count (device form).
 * Both calls apply the last frame's deferred pool releases first, so regions taken right after a frame see that
 * frame's map.  The map is only read (directory, pool, free list and directory-delta record stay as they are).  A
 * sticky engine error is returned, never hidden.  Workspace is engine-owned and grows on demand; a failed allocation
 * is RATSDF_ERR_DEVICE (not sticky: the next call tries again).
 */
#ifndef RATSDF_REGIONS_H_
#define RATSDF_REGIONS_H_

#include "ratsdf_esdf.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ratsdf_region { /* 32 bytes */
  int32_t root;          /* the region's label: box index of its first voxel */
  int32_t voxels;        /* members of the region */
  int32_t frontier;      /* members with at least one face neighbour INSIDE the box whose state is UNKNOWN */
  uint32_t faces;        /* bit 2a: a member has v[a] == origin[a]; bit 2a+1: a member has v[a] == origin[a]+dims[a]-1 */
  int16_t lo[3], hi[3];  /* bounding box of the members, absolute voxel indices, inclusive */
  uint32_t reserved;     /* written as 0 */
} ratsdf_region;

typedef struct ratsdf_regions_params { /* 16 bytes */
  float occupied_below; /* as in ratsdf_esdf.h; NaN refused */
  float min_prob;       /* see member(v); NaN refused */
  uint32_t states;      /* bit s set <=> voxels of RATSDF_ESDF_STATE_s may be members; 1..7 */
  uint32_t flags;       /* must be 0 */
} ratsdf_regions_params;

int ratsdf_regions(ratsdf_engine* e, const int32_t origin[3], const int32_t dims[3],
                   const ratsdf_regions_params* params, int32_t* labels /* may be NULL */, ratsdf_region** out,
                   size_t* n);
int ratsdf_regions_device(ratsdf_engine* e, const int32_t origin[3], const int32_t dims[3],
                          const ratsdf_regions_params* params, void* d_labels /* may be NULL */, void* d_regions,
                          int64_t capacity, void* d_count);

#ifdef __cplusplus
}
#endif
#endif /* RATSDF_REGIONS_H_ */
