"""ctypes view of the C ABI declared in include/ratsdf.h.

The same ABI is exported by the HIP engine (prefix ``ratsdf_``) and, for tests only, by the CPU
oracle (prefix ``ratsdf_oracle_``).  This module only knows the ABI's shape; which shared library
and prefix to bind is the caller's choice (the product binds libratsdf.so, see ``__init__``).
"""
import ctypes as C
import os

import numpy as np

BLOCK_VOLUME = 512

STATUS = {
    0: "ok",
    1: "bad argument",
    2: "device error",
    3: "voxel block pool exhausted",
    4: "internal work list overflow",
    5: "no device",
    6: "not implemented",
    7: "in-launch wait timed out",
}


class RatsdfError(RuntimeError):
    def __init__(self, status, what):
        super().__init__(f"{what}: status {status} ({STATUS.get(status, 'unknown')})")
        self.status = status


class Intrinsics(C.Structure):
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float)]


class Pose(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("qx", "qy", "qz", "qw", "tx", "ty", "tz")]


class Bounds(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("xmin", "xmax", "ymin", "ymax", "zmin", "zmax")]


class FrameStats(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("visible_blocks", "updated_voxels", "allocated_blocks",
                                         "deleted_blocks", "active_blocks", "slow_requests")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class Config(C.Structure):
    _fields_ = [("voxel_size", C.c_float), ("truncation", C.c_float), ("device", C.c_int32),
                ("block_bits", C.c_int32), ("bucket_bits", C.c_int32), ("shard_rank", C.c_int32),
                ("shard_count", C.c_int32), ("shard_slab_bits", C.c_int32), ("threads", C.c_int32),
                ("reserved", C.c_int32 * 7)]


# numpy views of the POD records (layouts fixed by the reference, see ratsdf.h)
BLOCK_DTYPE = np.dtype([("x", "<i2"), ("y", "<i2"), ("z", "<i2"), ("offset", "<i2"), ("idx", "<i4")])
RGBW_DTYPE = np.dtype([("r", "u1"), ("g", "u1"), ("b", "u1"), ("weight", "u1")])
VOXEL_TSDF_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("tsdf", "<f4")])
VOXEL_SEGM_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("tsdf", "<f4"),
                             ("prob", "<f4")])
assert BLOCK_DTYPE.itemsize == 12 and VOXEL_TSDF_DTYPE.itemsize == 16
assert VOXEL_SEGM_DTYPE.itemsize == 20 and RGBW_DTYPE.itemsize == 4

# The records, constants and parameter structs of the feature headers, header by header; their entry points are rows
# of the ABI table below.
# include/ratsdf_sample.h (batched point sampling): ratsdf_sample (32 bytes); flags: SAMPLE_ALLOCATED |
# SAMPLE_OBSERVED | SAMPLE_NEAREST
SAMPLE_DTYPE = np.dtype([("tsdf", "<f4"), ("grad", "<f4", (3,)), ("prob", "<f4"), ("rgbw", RGBW_DTYPE),
                         ("min_weight", "u1"), ("flags", "u1"), ("reserved", "u1", (6,))])
SAMPLE_ALLOCATED, SAMPLE_OBSERVED, SAMPLE_NEAREST = 1, 2, 4
assert SAMPLE_DTYPE.itemsize == 32
# include/ratsdf_esdf.h (Euclidean signed distance field over a box)
ESDF_UNKNOWN_OCCUPIED = 1
ESDF_STATE_UNKNOWN, ESDF_STATE_FREE, ESDF_STATE_OCCUPIED = 0, 1, 2
# include/ratsdf_fuse.h (map fusion): ratsdf_fuse_stats (40 bytes)
FUSE_STATS = np.dtype([("blocks_seen", "<i8"), ("blocks_allocated", "<i8"), ("blocks_skipped", "<i8"),
                       ("voxels_copied", "<i8"), ("voxels_averaged", "<i8")])
assert FUSE_STATS.itemsize == 40
# include/ratsdf_surface.h (oriented surface points of a box): ratsdf_surface_point (32 bytes)
SURFACE_DTYPE = np.dtype([("pos", "<f4", (3,)), ("normal", "<f4", (3,)), ("prob", "<f4"), ("rgbw", RGBW_DTYPE)])
assert SURFACE_DTYPE.itemsize == 32


class SurfaceParams(C.Structure):
    """ratsdf_surface_params"""
    _fields_ = [("min_weight", C.c_int32), ("min_prob", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


# ... and the exposure of such points to lamps (ratsdf_exposure*): ratsdf_lamp (16 bytes), ratsdf_lamp_record (16 bytes),
# ratsdf_exposure_summary (32 bytes)
EXPOSURE_UNKNOWN_OCCUPIED, EXPOSURE_ACCUMULATE = 1, 2
EXPOSURE_MAX_LAMPS = 64
LAMP_DTYPE = np.dtype([("pos", "<f4", (3,)), ("power", "<f4")])
LAMP_RECORD_DTYPE = np.dtype([("accepted", "<i4"), ("lit", "<i4"), ("lit_high", "<i4"), ("reserved", "<i4")])
EXPOSURE_SUMMARY_DTYPE = np.dtype([("lit_pairs", "<i8"), ("points_lit", "<i4"), ("points_outside", "<i4"),
                                   ("lamps_accepted", "<i4"), ("reserved", "<u4", (3,))])
assert LAMP_DTYPE.itemsize == 16 and LAMP_RECORD_DTYPE.itemsize == 16 and EXPOSURE_SUMMARY_DTYPE.itemsize == 32


class ExposureParams(C.Structure):
    """ratsdf_exposure_params"""
    _fields_ = [("occupied_below", C.c_float), ("max_range", C.c_float), ("min_irradiance", C.c_float),
                ("p_cutoff", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class SurfaceMeshParams(C.Structure):
    """ratsdf_surface_mesh_params (include/ratsdf_surface_mesh.h: welded triangle mesh of a box)"""
    _fields_ = [("min_weight", C.c_int32), ("flags", C.c_uint32), ("reserved0", C.c_uint32),
                ("reserved1", C.c_uint32)]


class ClusterMeshParams(C.Structure):
    """ratsdf_cluster_mesh_params (include/ratsdf_cluster_mesh.h: clustered mesh of a box)"""
    _fields_ = [("min_weight", C.c_int32), ("factor", C.c_int32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


# include/ratsdf_regions.h (connected regions of a box): ratsdf_region (32 bytes)
REGION_DTYPE = np.dtype([("root", "<i4"), ("voxels", "<i4"), ("frontier", "<i4"), ("faces", "<u4"),
                         ("lo", "<i2", (3,)), ("hi", "<i2", (3,)), ("reserved", "<u4")])
assert REGION_DTYPE.itemsize == 32


class RegionsParams(C.Structure):
    """ratsdf_regions_params"""
    _fields_ = [("occupied_below", C.c_float), ("min_prob", C.c_float), ("states", C.c_uint32), ("flags", C.c_uint32)]


# include/ratsdf_cost.h (cost-to-go field of a box)
COST_UNKNOWN_OCCUPIED, COST_THROUGH_UNKNOWN, COST_FACES_ONLY, COST_CONTINUE = 1, 2, 4, 8
COST_NONE = 0xFFFFFFFF
COST_AT_GOAL, COST_NO_STEP = 255, 254       # `next` bytes that are no direction code
# ratsdf_cost_summary (32 bytes)
COST_SUMMARY_DTYPE = np.dtype([("goals", "<i4"), ("traversable", "<i4"), ("reached", "<i4"), ("max_cost", "<u4"),
                               ("pending", "<i4"), ("rounds", "<i4"), ("reserved", "<u4", (2,))])
assert COST_SUMMARY_DTYPE.itemsize == 32


def cost_direction(code):
    """(dx, dy, dz) of a direction code (dx + 1) + 3 * (dy + 1) + 9 * (dz + 1)"""
    code = int(code)
    return code % 3 - 1, code // 3 % 3 - 1, code // 9 - 1


class CostParams(C.Structure):
    """ratsdf_cost_params"""
    _fields_ = [("occupied_below", C.c_float), ("clearance", C.c_float), ("flags", C.c_uint32), ("rounds", C.c_int32)]


# include/ratsdf_score.h (label sets and the map's score against them)
LABEL_IGNORE, LABEL_LOW, LABEL_HIGH = 0, 1, 2
# ratsdf_label_score (4160 bytes) and ratsdf_voxel_label (8 bytes)
LABEL_SCORE_DTYPE = np.dtype([("voxels", "<i8"), ("selected", "<i8"), ("unmatched", "<i8"), ("unannotated", "<i8"),
                              ("confusion", "<i8", (4,)), ("hist", "<i8", (2, 256))])
VOXEL_LABEL_DTYPE = np.dtype([("nearest", "<i4"), ("dist2", "<f4")])
assert LABEL_SCORE_DTYPE.itemsize == 4160 and VOXEL_LABEL_DTYPE.itemsize == 8


class ScoreParams(C.Structure):
    """ratsdf_score_params"""
    _fields_ = [("tsdf_below", C.c_float), ("max_dist", C.c_float), ("p_cutoff", C.c_float),
                ("min_weight", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class LabelSetInfo(C.Structure):
    """ratsdf_labelset_info"""
    _fields_ = [("points", C.c_int64), ("kept", C.c_int64), ("cell", C.c_float), ("origin", C.c_float * 3),
                ("cells", C.c_int32 * 3), ("reserved", C.c_uint32)]


class _LabelHandle:
    """a set of labelled records on the device, LabelSet or LabelMesh: the handle, its info and its release.  A
    subclass names the symbols' prefix, the info struct and the fields of it that `info` reports."""
    _prefix, _Info, _fields = None, None, ()

    def __init__(self, lib, handle):
        self.lib, self._h = lib, handle

    @property
    def info(self):
        i = self._Info()
        _check(self.lib.fn[self._prefix + "_info_get"](self._h, C.byref(i)), self._prefix + "_info_get")
        values = ((f, getattr(i, f)) for f in self._fields)
        return {f: tuple(v) if isinstance(v, C.Array) else v for f, v in values}

    def close(self):
        if getattr(self, "_h", None):
            self.lib.fn[self._prefix + "_destroy"](self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class LabelSet(_LabelHandle):
    """labelled points on the device (ratsdf_labelset): built by Engine.label_set, immutable, usable by every engine of
    the same device until close()"""
    _prefix, _Info, _fields = "labelset", LabelSetInfo, ("points", "kept", "cell", "origin", "cells")


class LabelScore:
    """the counts of ratsdf_label_score with the reference's figures (scanneteval.py:95-124: IoU, precision and recall
    with its 1e-15 in the denominator, the voxel accuracy without, so NaN when nothing was counted).  Counts of shard
    ranks add: a + b."""

    def __init__(self, record):
        self.record = np.array(record, dtype=LABEL_SCORE_DTYPE).reshape(())

    voxels = property(lambda self: int(self.record["voxels"]))
    selected = property(lambda self: int(self.record["selected"]))
    unmatched = property(lambda self: int(self.record["unmatched"]))
    unannotated = property(lambda self: int(self.record["unannotated"]))
    confusion = property(lambda self: tuple(int(v) for v in self.record["confusion"]))
    hist = property(lambda self: self.record["hist"])

    @staticmethod
    def _figures(tp, fp, fn, tn):
        return {"iou": tp / (tp + fp + fn + 1e-15), "precision": tp / (tp + fp + 1e-15),
                "recall": tp / (tp + fn + 1e-15),
                "accuracy": (tp + tn) / (tp + tn + fp + fn) if tp + tn + fp + fn else float("nan")}

    iou = property(lambda self: self._figures(*self.confusion)["iou"])
    precision = property(lambda self: self._figures(*self.confusion)["precision"])
    recall = property(lambda self: self._figures(*self.confusion)["recall"])
    accuracy = property(lambda self: self._figures(*self.confusion)["accuracy"])

    def pr_curve(self):
        """the figures at every cutoff k / 256, k = 0..255, from the histogram: a voxel in bin b has a probability in
        [b / 256, (b + 1) / 256), so it is predicted high at cutoff k / 256 exactly when b >= k -- except that a
        probability EQUAL to k / 256 is not above it: the curve is that of the test prob >= k / 256 for k > 0 and
        counts bin 0 (zero, negative and NaN probabilities included) as high at k = 0.  Returns a dict of arrays
        (cutoff, tp, fp, fn, tn, iou, precision, recall, accuracy)."""
        h = self.hist.astype(np.int64)
        above = np.cumsum(h[:, ::-1], axis=1)[:, ::-1]           # voxels in bins >= k
        total = h.sum(axis=1, keepdims=True)
        fp, tp = above[0], above[1]
        tn, fn = total[0] - fp, total[1] - tp
        out = {"cutoff": np.arange(256) / 256.0, "tp": tp, "fp": fp, "fn": fn, "tn": tn}
        with np.errstate(invalid="ignore", divide="ignore"):
            out.update({"iou": tp / (tp + fp + fn + 1e-15), "precision": tp / (tp + fp + 1e-15),
                        "recall": tp / (tp + fn + 1e-15), "accuracy": (tp + tn) / (tp + tn + fp + fn)})
        return out

    def __add__(self, other):
        r = self.record.copy()
        for k in LABEL_SCORE_DTYPE.names:
            r[k] = self.record[k] + other.record[k]
        return LabelScore(r)

    def __eq__(self, other):
        return isinstance(other, LabelScore) and self.record.tobytes() == other.record.tobytes()

    def __repr__(self):
        return (f"LabelScore(voxels={self.voxels}, selected={self.selected}, unmatched={self.unmatched}, "
                f"unannotated={self.unannotated}, confusion={self.confusion}, iou={self.iou:.6f})")


# include/ratsdf_score_mesh.h (labelled triangle meshes and the map's score against them)
LABELMESH_MAX_REFS = 1 << 25


class LabelMeshInfo(C.Structure):
    """ratsdf_labelmesh_info"""
    _fields_ = [("vertices", C.c_int64), ("triangles", C.c_int64), ("kept", C.c_int64), ("mixed", C.c_int64),
                ("refs", C.c_int64), ("cell", C.c_float), ("origin", C.c_float * 3), ("cells", C.c_int32 * 3),
                ("reserved", C.c_uint32)]


class LabelMesh(_LabelHandle):
    """a labelled triangle mesh on the device (ratsdf_labelmesh): built by Engine.label_mesh, immutable, usable by
    every engine of the same device until close()"""
    _prefix, _Info = "labelmesh", LabelMeshInfo
    _fields = ("vertices", "triangles", "kept", "mixed", "refs", "cell", "origin", "cells")


class _OwnedBuffer:
    """a result buffer handed over by the library (malloc'ed there): exposes it through the array interface and gives
    it back with ratsdf_free_buffer when the last array built on it is collected"""

    def __init__(self, lib, address, nbytes):
        self._lib, self._address = lib, address
        self.__array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (address, False), "version": 3}

    def __del__(self):
        try:
            if self._address:
                self._lib.fn["free_buffer"](C.c_void_p(self._address))
                self._address = 0
        except Exception:   # (interpreter shutdown: the library object may be gone already)
            pass


def _ptr(a, ctype):
    return a.ctypes.data_as(C.POINTER(ctype)) if a is not None else None


def descend(next, origin, start, max_steps=None):
    """follows the direction bytes `next` (shape (Z, Y, X), of a box at `origin`) from the absolute voxel `start`:
    the voxel path as an int32 [k, 3] array, start first.  It ends at a COST_AT_GOAL voxel, at a COST_NO_STEP voxel
    (the path is then just what led there), after max_steps moves (default: the box's voxels), or where a move would
    leave the box."""
    nxt = np.asarray(next)
    Z, Y, X = nxt.shape
    v = [int(a) - int(b) for a, b in zip(start, origin)]
    if not (0 <= v[0] < X and 0 <= v[1] < Y and 0 <= v[2] < Z):
        raise ValueError("start outside the box")
    limit = nxt.size if max_steps is None else int(max_steps)
    path = [tuple(v)]
    for _ in range(limit):
        code = int(nxt[v[2], v[1], v[0]])
        if code >= 27:
            break
        dx, dy, dz = cost_direction(code)
        v = [v[0] + dx, v[1] + dy, v[2] + dz]
        if not (0 <= v[0] < X and 0 <= v[1] < Y and 0 <= v[2] < Z):
            break
        path.append(tuple(v))
    return (np.asarray(path, dtype=np.int64) + np.asarray(origin, dtype=np.int64)).astype(np.int32).reshape(-1, 3)


_vp, _str, _int, _i32, _i64, _u32, _f32, _size = (C.c_void_p, C.c_char_p, C.c_int, C.c_int32, C.c_int64, C.c_uint32,
                                                  C.c_float, C.c_size_t)
_P = C.POINTER
_frame = [_vp, _vp, _vp, _vp, _vp, _int, _int, _f32, _P(Intrinsics), _P(Pose)]          # one frame's images and camera
_frames = [_vp, _int, _vp, _vp, _vp, _vp, _int, _int, _f32, _vp, _vp]                   # n frames: tables of them
_view = [_vp, _P(Intrinsics), _int, _int, _P(Pose), _f32]                               # a ray cast's camera
_box = [_vp, _P(_i32), _P(_i32)]                                                        # engine, origin[3], dims[3]
_owned = [_P(_vp), _P(_size)]                      # a result buffer handed over: (pointer, count) out-parameters
_profile = [_vp, _P(C.c_double), _P(_i64)]
_mesh = _owned + _owned                                                                 # vertices, then triangles
_mesh_device = [_vp, _i64, _vp, _i64, _vp]
_labelset = [_vp, _vp, _vp, _size, _f32, _P(_vp)]
_labelmesh = [_vp, _vp, _vp, _size, _vp, _size, _f32, _P(_vp)]
_score = [_vp, _vp, _P(ScoreParams), _vp]

# The shape of the C ABI: header -> {symbol (without prefix): argtypes}, in the headers' order.  A new entry point is
# one row here.  ratsdf.h's symbols must all be exported; those of the other headers are bound when the library has
# them -- the CPU oracle does not, and there they report status 6 (not implemented).
ABI = {
    "ratsdf.h": {
        "create": [_f32, _f32, _int, _P(_vp)],
        "create_ex": [_P(Config), _P(_vp)],
        "destroy": [_vp],
        "integrate": _frame,
        "integrate_device": _frame,
        "integrate_device_batch": _frames,
        "prepare_device_batch": [_vp, _int, _int, _int],
        "integrate_batch": _frames + [_int],
        "host_alloc": [_size, _P(_vp)],
        "host_free": [_vp],
        "synchronize": [_vp],
        "recover": [_vp],
        "stream": [_vp, _P(_vp)],
        "profile_enable": [_vp, _int],
        "profile_read": _profile,
        "profile_read_frames": [_vp, _P(_f32), _P(_f32), _int, _P(_int)],
        "totals": [_vp, _P(_i64), _int],
        "pipeline_counters": [_vp, _P(_i64), _int],
        "num_active_blocks": [_vp, _P(_i32)],
        "last_frame_stats": [_vp, _P(FrameStats)],
        "query": [_vp, _P(Bounds)] + _owned,
        "gather_valid": [_vp] + _owned,
        "gather_valid_semantic": [_vp] + _owned,
        "download_all": [_vp, _str],
        "free_buffer": [_vp],
        "raycast": _view + [_vp, _vp],
        "raycast_rows": _view + [_int, _int, _vp, _vp],
        "raycast_device": _view + [_vp, _vp],
        "gather_valid_mesh": [_vp] + _mesh + [_P(_vp)],
        "download_all_mesh": [_vp, _str, _str, _str],
        "export_directory_device": [_vp, _vp, _i32, _vp],
        "export_directory_delta_device": [_vp, _vp, _i32, _vp],
        "import_blocks": [_vp, _i32, _vp, _vp, _vp, _vp],
        "export_blocks_device": [_vp, _i32, _vp, _vp, _vp],
        "import_blocks_device": [_vp, _i32, _vp, _vp],
        "group_create": [_vp, _int, _P(_vp)],
        "group_destroy": [_vp],
        "group_size": [_vp, _P(_i32)],
        "group_integrate_device_batch": _frames,
        "group_synchronize": [_vp],
        "group_profile_enable": [_vp, _int],
        "group_profile_read": _profile,
        "test_allocate": [_vp, _vp, _i32],
        "test_delete": [_vp, _vp, _i32],
        "test_retrieve": [_vp, _vp, _i32, _vp, _vp, _vp, _vp],
        "test_assign_rgbw": [_vp, _vp, _vp, _i32],
        "dump_directory": [_vp, _P(_vp), _P(_vp), _P(_size)],
        "dump_voxels": [_vp, _vp, _i32, _vp, _vp, _vp],
        "dump_heap": [_vp, _P(_i32), _vp],
        "status_string": [_int],
        "backend": [],
    },
    "ratsdf_map.h": {
        "save_map": [_vp, _str],
        "load_map": [_vp, _str],
        "map_file_info": [_str, _P(Config), _P(_i64)],
    },
    "ratsdf_sample.h": {
        "sample_points": [_vp, _vp, _size, _vp],
        "sample_points_device": [_vp, _vp, _size, _vp],
    },
    "ratsdf_esdf.h": {
        "esdf": _box + [_f32, _u32, _vp, _vp],
        "esdf_device": _box + [_f32, _u32, _vp, _vp],
    },
    "ratsdf_fuse.h": {
        "fuse_map": [_vp, _vp, _vp],
        "fuse_blocks": [_vp, _i32, _vp, _vp, _vp, _vp, _vp],
        "fuse_blocks_device": [_vp, _i32, _vp, _vp, _vp],
        "fuse_map_file": [_vp, _str, _vp],
    },
    "ratsdf_resample.h": {
        "resample_blocks_device": [_vp, _P(Pose), _i32, _vp, _vp, _vp],
        "fuse_map_transformed": [_vp, _vp, _P(Pose), _vp],
    },
    "ratsdf_coarsen.h": {
        "coarsen_blocks_device": [_vp, _i32, _vp, _vp, _vp],
        "fuse_map_coarsened": [_vp, _vp, _vp],
    },
    "ratsdf_surface.h": {
        "surface_points": _box + [_P(SurfaceParams)] + _owned,
        "surface_points_device": _box + [_P(SurfaceParams), _vp, _i64, _vp],
        "exposure": _box + [_P(ExposureParams), _vp, _i64, _vp, _i32, _vp, _vp, _vp, _vp],
        "exposure_device": _box + [_P(ExposureParams), _vp, _i64, _vp, _i32, _vp, _vp, _vp, _vp],
    },
    "ratsdf_surface_mesh.h": {
        "surface_mesh": _box + [_P(SurfaceMeshParams)] + _mesh,
        "surface_mesh_device": _box + [_P(SurfaceMeshParams)] + _mesh_device,
    },
    "ratsdf_cluster_mesh.h": {
        "cluster_mesh": _box + [_P(ClusterMeshParams)] + _mesh,
        "cluster_mesh_device": _box + [_P(ClusterMeshParams)] + _mesh_device,
    },
    "ratsdf_regions.h": {
        "regions": _box + [_P(RegionsParams), _vp] + _owned,
        "regions_device": _box + [_P(RegionsParams), _vp, _vp, _i64, _vp],
    },
    "ratsdf_cost.h": {
        "cost_to_go": _box + [_P(CostParams), _vp, _i32, _vp, _vp, _vp],
        "cost_to_go_device": _box + [_P(CostParams), _vp, _i32, _vp, _vp, _vp],
    },
    "ratsdf_score.h": {
        "labelset_create": _labelset,
        "labelset_create_device": _labelset,
        "labelset_info_get": [_vp, _P(LabelSetInfo)],
        "labelset_destroy": [_vp],
        "score_labels": _score + _owned,
        "score_labels_device": _score + [_vp, _i64, _vp],
    },
    "ratsdf_score_mesh.h": {
        "labelmesh_create": _labelmesh,
        "labelmesh_create_device": _labelmesh,
        "labelmesh_info_get": [_vp, _P(LabelMeshInfo)],
        "labelmesh_destroy": [_vp],
        "score_mesh": _score + _owned,
        "score_mesh_device": _score + [_vp, _i64, _vp],
    },
}
RESTYPE = {"status_string": _str, "backend": _str}      # every other entry point returns a status (int)

# the symbols header by header: the table's keys
(SYMBOLS, MAP_SYMBOLS, SAMPLE_SYMBOLS, ESDF_SYMBOLS, FUSE_SYMBOLS, RESAMPLE_SYMBOLS, COARSEN_SYMBOLS, SURFACE_SYMBOLS,
 SURFACE_MESH_SYMBOLS, CLUSTER_MESH_SYMBOLS, REGIONS_SYMBOLS, COST_SYMBOLS, SCORE_SYMBOLS,
 SCORE_MESH_SYMBOLS) = (list(table) for table in ABI.values())


class Library:
    """A loaded shared library exporting the ABI under ``prefix``."""

    def __init__(self, path, prefix="ratsdf_"):
        self.path = str(path)
        self.prefix = prefix
        self.dll = C.CDLL(self.path)
        self.fn = {}
        for header, table in ABI.items():
            core = header == "ratsdf.h"
            for s, argtypes in table.items():
                try:
                    f = getattr(self.dll, prefix + s)  # AttributeError = missing export
                except AttributeError:
                    # (same-box A/B against engine builds of earlier commits, tools/build_variant.sh: entry points
                    # of ratsdf.h added since are simply absent there; never set for the product library)
                    if core and os.environ.get("RATSDF_LIB_VARIANT") != "1":
                        raise
                    f = C.CFUNCTYPE(C.c_int)(lambda *a: 6)
                    if not core:
                        argtypes = None
                if argtypes is not None:
                    f.restype, f.argtypes = RESTYPE.get(s, C.c_int), argtypes
                self.fn[s] = f

    def backend(self):
        return self.fn["backend"]().decode()

    def map_file_info(self, path):
        """validates a map file on the host (ratsdf_map_file_info): its configuration and number of live blocks"""
        cfg, n = Config(), C.c_int64()
        _check(self.fn["map_file_info"](os.fsencode(path), C.byref(cfg), C.byref(n)), "map_file_info")
        return {"voxel_size": cfg.voxel_size, "truncation": cfg.truncation, "block_bits": cfg.block_bits,
                "bucket_bits": cfg.bucket_bits, "shard_rank": cfg.shard_rank, "shard_count": cfg.shard_count,
                "shard_slab_bits": cfg.shard_slab_bits, "n_blocks": n.value}


def _check(st, what):
    if st != 0:
        raise RatsdfError(st, what)


def _box3(v, what):
    """three int32 of a voxel box (origin or dims) for the ESDF entry points"""
    a = np.asarray(v).reshape(-1)
    if a.shape != (3,) or not np.all(a == np.trunc(a.astype(np.float64))):
        raise ValueError(f"{what} must be three integers")
    if np.any(a < -(1 << 31)) or np.any(a >= (1 << 31)):
        raise ValueError(f"{what} out of the int32 range")
    return (C.c_int32 * 3)(*(int(x) for x in a))


def _box_shape(d):
    """the (Z, Y, X) shape of the per-voxel output of a box with the three int32 dims `d`.  A box beyond the limits
    gets a one-voxel placeholder: the library refuses it, status 1"""
    n = int(np.prod([int(v) for v in d], dtype=object))
    return tuple(int(v) for v in d[::-1]) if all(v > 0 for v in d) and n <= 1 << 27 else (1,)


def _device_ptrs(*buffers):
    """the raw pointer of every device buffer (torch tensor, devmem.DeviceArray or the pointer itself); None for 0"""
    return [(v.data_ptr() if hasattr(v, "data_ptr") else int(v or 0)) or None for v in buffers]


def _esdf_flags(unknown_occupied):
    """the flags word: a bool, or the raw word itself (an int: unknown bits reach the library, which refuses them)"""
    if isinstance(unknown_occupied, (bool, np.bool_)):
        return C.c_uint32(ESDF_UNKNOWN_OCCUPIED if unknown_occupied else 0)
    return C.c_uint32(int(unknown_occupied))


def voxel_box(lo, hi, voxel_size):
    """(origin, dims) of the voxel box that covers the metric box [lo, hi] (3 floats each, metres): per axis the
    voxel indices floor(float32(lo / vs)) .. floor(float32(hi / vs)), both ends inclusive, the quotient evaluated in
    float32 as the engine's kernels do.  Raises ValueError for a non-finite corner or hi below lo."""
    vs = np.float32(voxel_size)
    lo = np.asarray(lo, dtype=np.float32).reshape(3)
    hi = np.asarray(hi, dtype=np.float32).reshape(3)
    if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi))):
        raise ValueError("box corners must be finite")
    a = np.floor(lo / vs).astype(np.int64)
    b = np.floor(hi / vs).astype(np.int64)
    if np.any(b < a):
        raise ValueError("hi must not lie below lo")
    return [int(v) for v in a], [int(v) for v in b - a + 1]


def _as_pose(pose):
    if isinstance(pose, Pose):
        return pose
    q = [float(v) for v in pose]
    if len(q) != 7:
        raise ValueError("pose must be (qx, qy, qz, qw, tx, ty, tz)")
    return Pose(*q)


def _as_intr(k):
    if isinstance(k, Intrinsics):
        return k
    return Intrinsics(*[float(v) for v in k])


class Engine:
    """One TSDF map (the reference's ``TSDFGrid``, utils/tsdf/voxel_tsdf.cuh:39-145)."""

    def __init__(self, lib, voxel_size, truncation, device=0, block_bits=0, bucket_bits=0,
                 shard_rank=0, shard_count=1, shard_slab_bits=0, threads=0):
        self.lib = lib
        self.voxel_size = float(voxel_size)
        self.truncation = float(truncation)
        self.device = int(device)
        cfg = Config()
        cfg.voxel_size = voxel_size
        cfg.truncation = truncation
        cfg.device = device
        cfg.block_bits = block_bits
        cfg.bucket_bits = bucket_bits
        cfg.shard_rank = shard_rank
        cfg.shard_count = shard_count
        cfg.shard_slab_bits = shard_slab_bits
        cfg.threads = threads
        self.block_bits = block_bits or 18
        self.bucket_bits = bucket_bits or 21
        h = C.c_void_p()
        _check(lib.fn["create_ex"](C.byref(cfg), C.byref(h)), "create")
        self._h = h

    # -- lifetime --------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self.lib.fn["destroy"](self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- hot path --------------------------------------------------------------------------
    def integrate(self, rgb, depth, ht, lt, max_depth, intrinsics, pose):
        """TSDFGrid::Integrate (voxel_tsdf.cu:416-452) on host numpy images."""
        depth = np.ascontiguousarray(depth, dtype=np.float32)
        rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
        h, w = depth.shape
        if rgb.shape != (h, w, 3):
            raise ValueError("rgb must be HxWx3 uint8 matching depth")
        if ht is not None:
            ht = np.ascontiguousarray(ht, dtype=np.float32)
        if lt is not None:
            lt = np.ascontiguousarray(lt, dtype=np.float32)
        for a in (ht, lt):
            if a is not None and a.shape != (h, w):
                raise ValueError("ht/lt must match depth")
        k, p = _as_intr(intrinsics), _as_pose(pose)
        st = self.lib.fn["integrate"](self._h, rgb.ctypes.data, depth.ctypes.data,
                                      ht.ctypes.data if ht is not None else None,
                                      lt.ctypes.data if lt is not None else None, h, w,
                                      float(max_depth), C.byref(k), C.byref(p))
        _check(st, "integrate")

    def integrate_device(self, d_rgb, d_depth, d_ht, d_lt, height, width, max_depth, intrinsics,
                         pose):
        """Frame already in HBM (raw device pointers as ints); asynchronous."""
        k, p = _as_intr(intrinsics), _as_pose(pose)
        st = self.lib.fn["integrate_device"](self._h, d_rgb, d_depth, d_ht or None, d_lt or None,
                                             height, width, float(max_depth), C.byref(k),
                                             C.byref(p))
        _check(st, "integrate_device")

    def make_batch(self, d_rgb, d_depth, d_ht, d_lt, height, width, max_depth, intrinsics, poses):
        """Pre-marshals n frames (lists of raw device pointers, intrinsics, poses) for
        integrate_device_batch; returns an opaque tuple that can be replayed many times."""
        n = len(d_rgb)
        arr = lambda ptrs: (C.c_void_p * n)(*ptrs) if ptrs is not None else None
        ks = (Intrinsics * n)(*[_as_intr(k) for k in intrinsics])
        ps = (Pose * n)(*[_as_pose(p) for p in poses])
        return (n, arr(d_rgb), arr(d_depth), arr(d_ht), arr(d_lt), int(height), int(width),
                float(max_depth), ks, ps)

    def integrate_device_batch(self, batch):
        n, rgb, depth, ht, lt, h, w, md, ks, ps = batch
        st = self.lib.fn["integrate_device_batch"](self._h, n, rgb, depth, ht, lt, h, w, md, ks, ps)
        _check(st, "integrate_device_batch")

    def prepare_device_batch(self, n, height, width):
        """scratch + HIP graph of an n-frame batch ahead of time (ratsdf_prepare_device_batch); launches nothing"""
        _check(self.lib.fn["prepare_device_batch"](self._h, int(n), int(height), int(width)), "prepare_device_batch")

    def host_alloc(self, shape, dtype):
        """numpy array in page-locked host memory (ratsdf_host_alloc); release with host_free()."""
        dtype = np.dtype(dtype)
        n = int(np.prod(shape)) * dtype.itemsize
        p = C.c_void_p()
        _check(self.lib.fn["host_alloc"](n, C.byref(p)), "host_alloc")
        buf = (C.c_char * n).from_address(p.value)
        arr = np.frombuffer(buf, dtype=dtype).reshape(shape)
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[arr.ctypes.data] = p
        return arr

    def host_free(self, arr):
        p = getattr(self, "_pinned", {}).pop(arr.ctypes.data, None)
        if p is not None:
            _check(self.lib.fn["host_free"](p), "host_free")

    def integrate_batch(self, frames, max_depth, pinned=False):
        """n frames from host memory in one call (ratsdf_integrate_batch).  frames: dicts with rgb,
        depth, ht, lt (numpy; ht / lt may be None), intrinsics, pose.  pinned=True: every image is a
        host_alloc() array (uploaded without a staging copy)."""
        self.integrate_host_batch(self.make_host_batch(frames, max_depth, pinned))

    def make_host_batch(self, frames, max_depth, pinned=False):
        """Pre-marshals n host frames for integrate_host_batch (the pointer tables of ratsdf_integrate_batch take
        ~0.2 ms of Python per 32 frames: a caller that replays the same buffers builds them once).  The arrays the
        pointers refer to are kept alive by the returned object; it reads them again at every replay."""
        n = len(frames)
        keep = []
        def col(key, dtype):
            ptrs = []
            for f in frames:
                a = f.get(key)
                if a is None:
                    ptrs.append(None)
                else:
                    a = np.ascontiguousarray(a, dtype=dtype)
                    keep.append(a)
                    ptrs.append(a.ctypes.data)
            return (C.c_void_p * n)(*ptrs)
        # semantics are decided frame by frame (tsdf_module.cc:27-31): the tables go whenever ANY frame has both
        # images, with NULL entries for the frames that lack one; NULL tables only when no frame has them
        sem = any(f.get("ht") is not None and f.get("lt") is not None for f in frames)
        h, w = frames[0]["depth"].shape
        ks = (Intrinsics * n)(*[_as_intr(f["intrinsics"]) for f in frames])
        ps = (Pose * n)(*[_as_pose(f["pose"]) for f in frames])
        return (n, col("rgb", np.uint8), col("depth", np.float32), col("ht", np.float32) if sem else None,
                col("lt", np.float32) if sem else None, h, w, float(max_depth), ks, ps, 1 if pinned else 0, keep)

    def integrate_host_batch(self, batch):
        n, rgb, depth, ht, lt, h, w, md, ks, ps, pinned, _keep = batch
        _check(self.lib.fn["integrate_batch"](self._h, n, rgb, depth, ht, lt, h, w, md, ks, ps, pinned), "integrate_batch")

    def synchronize(self):
        _check(self.lib.fn["synchronize"](self._h), "synchronize")

    def recover(self):
        """after a sticky error: rebuild everything derived from the block directory, clear the error (ratsdf_recover)"""
        _check(self.lib.fn["recover"](self._h), "recover")

    def save_map(self, path):
        """writes the map to a checkpoint file (ratsdf_save_map, include/ratsdf_map.h)"""
        _check(self.lib.fn["save_map"](self._h, os.fsencode(path)), "save_map")

    def load_map(self, path):
        """replaces the map with a checkpoint file's; the map continues bit-exactly (ratsdf_load_map)"""
        _check(self.lib.fn["load_map"](self._h, os.fsencode(path)), "load_map")

    def stream(self):
        s = C.c_void_p()
        _check(self.lib.fn["stream"](self._h, C.byref(s)), "stream")
        return s.value or 0

    def profile_enable(self, on=True, every_frame=False):
        """HIP events on k_integrate: every 4th frame (sums), or every frame with per-frame records"""
        _check(self.lib.fn["profile_enable"](self._h, (2 if every_frame else 1) if on else 0), "profile_enable")

    def profile_read_frames(self, capacity=60000):
        """(k_integrate us per frame, start-to-start period us per frame) as float32 arrays"""
        k = np.zeros(capacity, dtype=np.float32)
        p = np.zeros(capacity, dtype=np.float32)
        n = C.c_int()
        _check(self.lib.fn["profile_read_frames"](self._h, _ptr(k, C.c_float), _ptr(p, C.c_float), capacity,
                                                  C.byref(n)), "profile_read_frames")
        m = min(n.value, capacity)
        return k[:m], p[:m]

    def profile_read(self):
        """(summed k_integrate milliseconds, launches) since the last read."""
        ms, n = C.c_double(), C.c_int64()
        _check(self.lib.fn["profile_read"](self._h, C.byref(ms), C.byref(n)), "profile_read")
        return ms.value, n.value

    def totals(self, reset=False):
        """dict(frames, visible_blocks, updated_voxels, allocated_blocks, deleted_blocks) sums."""
        t = (C.c_int64 * 5)()
        _check(self.lib.fn["totals"](self._h, t, 1 if reset else 0), "totals")
        return dict(zip(("frames", "visible_blocks", "updated_voxels", "allocated_blocks",
                         "deleted_blocks"), [int(v) for v in t]))

    def pipeline_counters(self, reset=False):
        """dict(front_tail, in_launch, in_launch_resolver, in_launch_general): frames by where their serial
        allocation-order pass ran (HIP engine only)."""
        t = (C.c_int64 * 4)()
        _check(self.lib.fn["pipeline_counters"](self._h, t, 1 if reset else 0), "pipeline_counters")
        return dict(zip(("front_tail", "in_launch", "in_launch_resolver", "in_launch_general"),
                        [int(v) for v in t]))

    def num_active_blocks(self):
        n = C.c_int32()
        _check(self.lib.fn["num_active_blocks"](self._h, C.byref(n)), "num_active_blocks")
        return n.value

    def last_frame_stats(self):
        s = FrameStats()
        _check(self.lib.fn["last_frame_stats"](self._h, C.byref(s)), "last_frame_stats")
        return s.as_dict()

    # -- query side ------------------------------------------------------------------------
    def _take(self, ptr, n, dtype):
        """the library's result buffer as a numpy array that OWNS it (freed with ratsdf_free_buffer when the array and
        its views are gone): no copy -- a GatherValid of the bench map is 41 MB"""
        if n == 0:
            if ptr.value:
                self.lib.fn["free_buffer"](ptr)
            return np.empty(0, dtype=dtype)
        return np.asarray(_OwnedBuffer(self.lib, ptr.value, n * dtype.itemsize)).view(dtype)

    def _call_owned(self, symbol, dtype, *args, wanted=True):
        """calls an entry point whose last two arguments are the (pointer, count) out-parameters of a result buffer
        (NULL for both unless `wanted`); returns the buffer as an array that owns it, or None"""
        p, n = C.c_void_p(), C.c_size_t()
        _check(self.lib.fn[symbol](self._h, *args, C.byref(p) if wanted else None, C.byref(n) if wanted else None),
               symbol)
        return self._take(p, n.value, dtype) if wanted else None

    def _read_back(self, d_buffer, dtype, n=1):
        """waits for the stream, then the first n `dtype` items of a device buffer that can be read from here: a torch
        tensor or a devmem.DeviceArray.  None for a raw pointer: the caller reads it"""
        self.synchronize()
        if hasattr(d_buffer, "cpu"):         # a torch tensor
            d_buffer = d_buffer.cpu()
        if not hasattr(d_buffer, "numpy"):
            return None
        return d_buffer.numpy().reshape(-1).view(np.uint8)[:n * np.dtype(dtype).itemsize].view(dtype)

    def query(self, bounds):
        """TSDFSystem::Query / TSDFGrid::GatherVoxels (voxel_tsdf.cu:532-559)."""
        b = bounds if isinstance(bounds, Bounds) else Bounds(*[float(v) for v in bounds])
        return self._call_owned("query", VOXEL_TSDF_DTYPE, C.byref(b))

    def gather_valid(self):
        return self._call_owned("gather_valid", VOXEL_TSDF_DTYPE)

    def gather_valid_semantic(self):
        return self._call_owned("gather_valid_semantic", VOXEL_SEGM_DTYPE)

    def download_all(self, path):
        _check(self.lib.fn["download_all"](self._h, str(path).encode()), "download_all")

    def raycast(self, intrinsics, height, width, pose, max_depth):
        """TSDFGrid::RayCast (voxel_tsdf.cu:885-902): returns (rgba, normal) HxWx4 uint8 images."""
        k, p = _as_intr(intrinsics), _as_pose(pose)
        rgba = np.zeros((height, width, 4), dtype=np.uint8)
        normal = np.zeros((height, width, 4), dtype=np.uint8)
        _check(self.lib.fn["raycast"](self._h, C.byref(k), height, width, C.byref(p),
                                      float(max_depth), rgba.ctypes.data, normal.ctypes.data),
               "raycast")
        return rgba, normal

    def raycast_device(self, intrinsics, height, width, pose, max_depth, d_rgba, d_normal):
        """raycast() into DEVICE buffers (H x W x 4 uint8 each; either may be 0), asynchronous on the engine's stream"""
        k, p = _as_intr(intrinsics), _as_pose(pose)
        _check(self.lib.fn["raycast_device"](self._h, C.byref(k), height, width, C.byref(p), float(max_depth),
                                             d_rgba or None, d_normal or None), "raycast_device")

    def raycast_rows(self, intrinsics, height, width, pose, max_depth, row0, row1):
        """rows [row0, row1) of raycast(): (rgba, normal), (row1 - row0) x W x 4 uint8 each"""
        k, p = _as_intr(intrinsics), _as_pose(pose)
        n = max(int(row1) - int(row0), 0)
        rgba = np.zeros((n, width, 4), dtype=np.uint8)
        normal = np.zeros((n, width, 4), dtype=np.uint8)
        _check(self.lib.fn["raycast_rows"](self._h, C.byref(k), height, width, C.byref(p), float(max_depth),
                                           int(row0), int(row1), rgba.ctypes.data, normal.ctypes.data), "raycast_rows")
        return rgba, normal

    def sample_points(self, points):
        """batched point sampling (ratsdf_sample_points, include/ratsdf_sample.h): points of shape (n, 3) in metres;
        returns n SAMPLE_DTYPE records (trilinear tsdf, its gradient per metre, the nearest voxel's probability and
        colour, the corners' smallest weight, flags)"""
        p = np.ascontiguousarray(points, dtype=np.float32)
        if p.ndim != 2 or p.shape[1] != 3:
            raise ValueError("points must have shape (n, 3)")
        n = p.shape[0]
        out = np.zeros(n, dtype=SAMPLE_DTYPE)
        _check(self.lib.fn["sample_points"](self._h, p.ctypes.data if n else None, n, out.ctypes.data if n else None),
               "sample_points")
        return out

    def sample_points_device(self, d_xyz, n, d_out):
        """sample_points() on DEVICE buffers (n x 3 float32 in, n 32-byte records out, 16-byte aligned), asynchronous
        on the engine's stream"""
        _check(self.lib.fn["sample_points_device"](self._h, d_xyz or None, int(n), d_out or None),
               "sample_points_device")

    def esdf(self, origin, dims, occupied_below=0.0, unknown_occupied=False, with_state=False):
        """Euclidean signed distance field over a box of voxels (ratsdf_esdf, include/ratsdf_esdf.h): origin is the
        voxel index of the box's minimum corner, dims the voxels per axis (x, y, z).  Returns a float32 array of shape
        (dims[2], dims[1], dims[0]) -- metres to the nearest obstacle voxel, negative inside obstacles -- and, with
        with_state, the uint8 ESDF_STATE_* of every voxel as a second array of the same shape."""
        o, d = _box3(origin, "origin"), _box3(dims, "dims")
        shape = _box_shape(d)
        out = np.empty(shape, dtype=np.float32)
        state = np.empty(shape, dtype=np.uint8) if with_state else None
        _check(self.lib.fn["esdf"](self._h, o, d, C.c_float(occupied_below), _esdf_flags(unknown_occupied),
                                   out.ctypes.data, state.ctypes.data if with_state else None), "esdf")
        return (out, state) if with_state else out

    def esdf_device(self, origin, dims, d_out, d_state=0, occupied_below=0.0, unknown_occupied=False):
        """esdf() into DEVICE buffers (d_out: dims[0]*dims[1]*dims[2] float32, 16-byte aligned; d_state: as many
        bytes, or 0 for none), asynchronous on the engine's stream.  Raw pointers: torch data_ptr() or
        devmem.DeviceArray.data_ptr()."""
        _check(self.lib.fn["esdf_device"](self._h, _box3(origin, "origin"), _box3(dims, "dims"),
                                          C.c_float(occupied_below), _esdf_flags(unknown_occupied), d_out or None,
                                          d_state or None), "esdf_device")

    def surface_points(self, origin, dims, min_weight=1, min_prob=0.0):
        """oriented surface points of a box of voxels (ratsdf_surface_points, include/ratsdf_surface.h): origin is the
        voxel index of the box's minimum corner, dims the voxels per axis (voxel_box turns a metric box into them).
        Returns SURFACE_DTYPE records -- position in metres, unit normal into free space, probability, colour and
        weight of the nearer voxel -- of every sign change of the TSDF between two neighbouring voxels of at least
        min_weight, in block order (z, y, x), then voxel order within the block, then axis."""
        params = SurfaceParams(int(min_weight), float(min_prob), 0, 0)
        return self._call_owned("surface_points", SURFACE_DTYPE, _box3(origin, "origin"), _box3(dims, "dims"),
                                C.byref(params))

    def surface_points_device(self, origin, dims, d_points, capacity, d_count, min_weight=1, min_prob=0.0):
        """surface_points() into DEVICE buffers, asynchronous on the engine's stream: the first min(total, capacity)
        32-byte records to d_points (16-byte aligned; 0 with capacity 0 for a pure count) and the total as an int64 to
        d_count.  d_points / d_count: a torch tensor, a devmem.DeviceArray or a raw pointer.  Returns the total (this
        waits for the stream)."""
        params = SurfaceParams(int(min_weight), float(min_prob), 0, 0)
        points, count = _device_ptrs(d_points, d_count)
        _check(self.lib.fn["surface_points_device"](self._h, _box3(origin, "origin"), _box3(dims, "dims"),
                                                    C.byref(params), points, int(capacity), count),
               "surface_points_device")
        total = self._read_back(d_count, np.int64)
        return None if total is None else int(total[0])

    @staticmethod
    def _exposure_params(occupied_below, max_range, min_irradiance, p_cutoff, unknown_occupied, accumulate):
        flags = (EXPOSURE_UNKNOWN_OCCUPIED if unknown_occupied else 0) | (EXPOSURE_ACCUMULATE if accumulate else 0)
        return ExposureParams(float(occupied_below), float(max_range), float(min_irradiance), float(p_cutoff), flags,
                              (C.c_uint32 * 3)(0, 0, 0))

    def exposure(self, origin, dims, points, lamps, occupied_below=0.0, max_range=np.inf, min_irradiance=0.0,
                 p_cutoff=0.5, unknown_occupied=False, dose=None, with_mask=False):
        """exposure of surface points to lamps through a box of voxels (ratsdf_exposure, include/ratsdf_surface.h):
        `points` SURFACE_DTYPE records (surface_points' output), `lamps` LAMP_DTYPE records (at most
        EXPOSURE_MAX_LAMPS: position in metres, power).  A lamp lights a point that faces it, within max_range, when
        the integer voxel walk from the point's start voxel (one voxel along its normal) to the lamp's voxel meets no
        OCCUPIED voxel of the box (nor an UNKNOWN one with unknown_occupied).  Returns (dose, [mask,] table, summary):
        dose float32 [n], the sum of P cos(theta) / 4 pi r^2 over the visible lamps in ascending lamp order -- on top
        of `dose` when one is given (the chain for more than 64 lamps), else from 0; mask uint64 [n], bit k for lamp k;
        table LAMP_RECORD_DTYPE [n_lamps] (accepted, points lit with at least min_irradiance, those of them with
        prob >= p_cutoff); summary an EXPOSURE_SUMMARY_DTYPE record."""
        o, d = _box3(origin, "origin"), _box3(dims, "dims")
        pts = np.ascontiguousarray(np.asarray(points, dtype=SURFACE_DTYPE).reshape(-1))
        lmp = np.ascontiguousarray(np.asarray(lamps, dtype=LAMP_DTYPE).reshape(-1))
        out = np.zeros(max(len(pts), 1), dtype=np.float32)[:len(pts)]   # (never a null pointer: an empty list too)
        if dose is not None:
            if np.size(dose) != len(pts):
                raise ValueError("dose must hold one float per point")
            out[:] = np.asarray(dose, dtype=np.float32).reshape(-1)
        mask = np.zeros(len(pts), dtype=np.uint64) if with_mask else None
        table = np.zeros(len(lmp), dtype=LAMP_RECORD_DTYPE)
        summary = np.zeros(1, dtype=EXPOSURE_SUMMARY_DTYPE)
        params = self._exposure_params(occupied_below, max_range, min_irradiance, p_cutoff, unknown_occupied,
                                       dose is not None)
        _check(self.lib.fn["exposure"](self._h, o, d, C.byref(params), pts.ctypes.data if len(pts) else None, len(pts),
                                       lmp.ctypes.data if len(lmp) else None, len(lmp),
                                       out.ctypes.data,
                                       mask.ctypes.data if with_mask and len(pts) else None,
                                       table.ctypes.data if len(lmp) else None, summary.ctypes.data), "exposure")
        return (out, mask, table, summary[0]) if with_mask else (out, table, summary[0])

    def exposure_device(self, origin, dims, d_points, n_points, d_lamps, n_lamps, d_dose, d_mask, d_lamp_table,
                        d_summary, occupied_below=0.0, max_range=np.inf, min_irradiance=0.0, p_cutoff=0.5,
                        unknown_occupied=False, accumulate=False):
        """exposure() on DEVICE buffers, asynchronous on the engine's stream: n_points 32-byte records at d_points and
        n_lamps 16-byte records at d_lamps (16-byte aligned); the doses to d_dose (float32, in/out with accumulate),
        the masks to d_mask (uint64, 0 for none), the lamp table to d_lamp_table (n_lamps 16-byte records, 0 for none)
        and the 32-byte summary to d_summary (8-byte aligned).  Each buffer: a torch tensor, a devmem.DeviceArray or a
        raw pointer.  Returns the summary record (this waits for the stream)."""
        params = self._exposure_params(occupied_below, max_range, min_irradiance, p_cutoff, unknown_occupied,
                                       accumulate)
        points, lamps, dose, mask, table, summary = _device_ptrs(d_points, d_lamps, d_dose, d_mask, d_lamp_table,
                                                                 d_summary)
        _check(self.lib.fn["exposure_device"](self._h, _box3(origin, "origin"), _box3(dims, "dims"), C.byref(params),
                                              points, int(n_points), lamps, int(n_lamps), dose, mask, table, summary),
               "exposure_device")
        record = self._read_back(d_summary, EXPOSURE_SUMMARY_DTYPE)
        return None if record is None else record[0]

    def surface_exposure(self, origin, dims, lamps, min_weight=1, min_prob=0.0, **exposure_kw):
        """surface_points_device() and then exposure_device() of the same box, the points staying on the device in
        between: (points, dose, mask) as numpy arrays -- SURFACE_DTYPE records, float32, uint64 -- plus the lamp table
        and the summary record.  exposure_kw: exposure_device's keywords but accumulate."""
        from .devmem import DeviceArray
        dev = self.device
        lmp = np.ascontiguousarray(np.asarray(lamps, dtype=LAMP_DTYPE).reshape(-1))
        d_count = DeviceArray(np.zeros(1, dtype=np.int64), dev)
        n = self.surface_points_device(origin, dims, 0, 0, d_count, min_weight=min_weight, min_prob=min_prob)
        d_points = DeviceArray(np.zeros(max(n, 1), dtype=SURFACE_DTYPE), dev)
        self.surface_points_device(origin, dims, d_points, n, d_count, min_weight=min_weight, min_prob=min_prob)
        d_lamps = DeviceArray(lmp if len(lmp) else np.zeros(1, dtype=LAMP_DTYPE), dev)
        d_dose = DeviceArray(np.zeros(max(n, 1), dtype=np.float32), dev)   # (OUTSIDE points keep it: a defined 0)
        d_mask = DeviceArray(np.zeros(max(n, 1), dtype=np.uint64), dev)
        d_table = DeviceArray(np.zeros(max(len(lmp), 1), dtype=LAMP_RECORD_DTYPE), dev)
        d_summary = DeviceArray(np.zeros(1, dtype=EXPOSURE_SUMMARY_DTYPE), dev)
        summary = self.exposure_device(origin, dims, d_points if n else 0, n, d_lamps if len(lmp) else 0, len(lmp),
                                       d_dose, d_mask, d_table if len(lmp) else 0, d_summary, **exposure_kw)
        return (d_points.numpy()[:n], d_dose.numpy()[:n], d_mask.numpy()[:n], d_table.numpy()[:len(lmp)], summary)

    def _mesh(self, symbol, origin, dims, params):
        """surface_mesh() and cluster_mesh(): `symbol` with its params struct"""
        pv, pt, nv, nt = C.c_void_p(), C.c_void_p(), C.c_size_t(), C.c_size_t()
        _check(self.lib.fn[symbol](self._h, _box3(origin, "origin"), _box3(dims, "dims"), C.byref(params),
                                   C.byref(pv), C.byref(nv), C.byref(pt), C.byref(nt)), symbol)
        return self._take(pv, nv.value, SURFACE_DTYPE), self._take(pt, nt.value * 3, np.dtype("<i4")).reshape(-1, 3)

    def _mesh_device(self, symbol, origin, dims, params, d_vertices, vertex_capacity, d_triangles, triangle_capacity,
                     d_counts):
        """surface_mesh_device() and cluster_mesh_device(): `symbol` with its params struct"""
        vertices, triangles, counts = _device_ptrs(d_vertices, d_triangles, d_counts)
        _check(self.lib.fn[symbol](self._h, _box3(origin, "origin"), _box3(dims, "dims"), C.byref(params), vertices,
                                   int(vertex_capacity), triangles, int(triangle_capacity), counts), symbol)
        totals = self._read_back(d_counts, np.int64, 2)
        return None if totals is None else tuple(int(v) for v in totals)

    def surface_mesh(self, origin, dims, min_weight=1):
        """welded triangle mesh of a box of voxels (ratsdf_surface_mesh, include/ratsdf_surface_mesh.h): (vertices,
        triangles).  The vertices are SURFACE_DTYPE records, the surface points that the triangles of the box's
        complete cells use, each once, in surface_points' order; the triangles are int32 [n, 3] indices into them,
        wound so that their normal points into free space, in the order of their cell's voxel."""
        return self._mesh("surface_mesh", origin, dims, SurfaceMeshParams(int(min_weight), 0, 0, 0))

    def surface_mesh_device(self, origin, dims, d_vertices, vertex_capacity, d_triangles, triangle_capacity, d_counts,
                            min_weight=1):
        """surface_mesh() into DEVICE buffers, asynchronous on the engine's stream: the first min(total, capacity)
        32-byte vertex records to d_vertices (16-byte aligned) and index triples to d_triangles (0 with capacity 0
        for a pure count), and the true totals as two int64 (vertices, triangles) to d_counts.  A triangle written
        while one of its vertices fell beyond vertex_capacity keeps its true index.  Each buffer: a torch tensor, a
        devmem.DeviceArray or a raw pointer.  Returns the two totals (this waits for the stream)."""
        return self._mesh_device("surface_mesh_device", origin, dims, SurfaceMeshParams(int(min_weight), 0, 0, 0),
                                 d_vertices, vertex_capacity, d_triangles, triangle_capacity, d_counts)

    def cluster_mesh(self, origin, dims, factor=4, min_weight=1):
        """clustered mesh of a box of voxels (ratsdf_cluster_mesh, include/ratsdf_cluster_mesh.h): (vertices,
        triangles).  surface_mesh() of the same box with its vertices merged per lattice-aligned cluster of factor^3
        voxels (factor 2, 4 or 8): one SURFACE_DTYPE record per non-empty cluster -- the mean of its members -- in
        block order, then cluster order within the block; the triangles are int32 [n, 3] indices into them, those with
        two vertices in one cluster dropped, the smallest index first, each once."""
        return self._mesh("cluster_mesh", origin, dims, ClusterMeshParams(int(min_weight), int(factor), 0, 0))

    def cluster_mesh_device(self, origin, dims, d_vertices, vertex_capacity, d_triangles, triangle_capacity, d_counts,
                            factor=4, min_weight=1):
        """cluster_mesh() into DEVICE buffers, asynchronous on the engine's stream: the arguments, the capacity rule
        and the result of surface_mesh_device()."""
        return self._mesh_device("cluster_mesh_device", origin, dims,
                                 ClusterMeshParams(int(min_weight), int(factor), 0, 0), d_vertices, vertex_capacity,
                                 d_triangles, triangle_capacity, d_counts)

    def regions(self, origin, dims, states=1 << ESDF_STATE_FREE, occupied_below=0.0, min_prob=0.0, with_labels=True):
        """connected regions of a box of voxels (ratsdf_regions, include/ratsdf_regions.h): the voxels whose
        ESDF_STATE_* is admitted by the bit mask `states` and whose probability is not below min_prob, grouped by face
        adjacency inside the box.  Returns (labels, table): labels is an int32 array of shape (dims[2], dims[1],
        dims[0]), -1 for a non-member and otherwise the smallest box index x + X * (y + Y * z) of the voxel's region;
        table is REGION_DTYPE records, one per region, ascending in root (size, voxels that border UNKNOWN ones, box
        faces reached, bounding box in absolute voxel indices).  Without with_labels only the table."""
        o, d = _box3(origin, "origin"), _box3(dims, "dims")
        labels = np.empty(_box_shape(d), dtype=np.int32) if with_labels else None
        params = RegionsParams(float(occupied_below), float(min_prob), int(states), 0)
        table = self._call_owned("regions", REGION_DTYPE, o, d, C.byref(params),
                                 labels.ctypes.data if with_labels else None)
        return (labels, table) if with_labels else table

    def regions_device(self, origin, dims, d_labels, d_regions, capacity, d_count, states=1 << ESDF_STATE_FREE,
                       occupied_below=0.0, min_prob=0.0):
        """regions() into DEVICE buffers, asynchronous on the engine's stream: the labels to d_labels (dims[0] * dims[1]
        * dims[2] int32, 16-byte aligned, or 0 for none), the first min(total, capacity) 32-byte records to d_regions
        (16-byte aligned; 0 with capacity 0 for a pure count) and the total as an int64 to d_count.  Each buffer: a
        torch tensor, a devmem.DeviceArray or a raw pointer.  Returns the total (this waits for the stream)."""
        params = RegionsParams(float(occupied_below), float(min_prob), int(states), 0)
        labels, regions, count = _device_ptrs(d_labels, d_regions, d_count)
        _check(self.lib.fn["regions_device"](self._h, _box3(origin, "origin"), _box3(dims, "dims"), C.byref(params),
                                             labels, regions, int(capacity), count), "regions_device")
        total = self._read_back(d_count, np.int64)
        return None if total is None else int(total[0])

    @staticmethod
    def _cost_flags(unknown_occupied, through_unknown, faces_only, resume=False):
        return ((COST_UNKNOWN_OCCUPIED if unknown_occupied else 0) | (COST_THROUGH_UNKNOWN if through_unknown else 0) |
                (COST_FACES_ONLY if faces_only else 0) | (COST_CONTINUE if resume else 0))

    def cost_to_go(self, origin, dims, goals, clearance=0.0, occupied_below=0.0, unknown_occupied=False,
                   through_unknown=False, faces_only=False, with_next=False):
        """cost-to-go field of a box of voxels (ratsdf_cost_to_go, include/ratsdf_cost.h): for every traversable voxel
        -- FREE (or UNKNOWN with through_unknown), outside the ESDF's obstacle set and not closer to it than `clearance`
        metres -- the least chamfer length (10 / 14 / 17 a face / edge / corner move; faces_only: face moves only) of a
        path through traversable voxels to one of `goals` ([n, 3] absolute voxel indices; those outside the box or not
        traversable are ignored).  Returns (cost, [next,] summary): cost uint32 of shape (dims[2], dims[1], dims[0]),
        COST_NONE where no goal is reached; with with_next the uint8 direction codes (COST_AT_GOAL, COST_NO_STEP or
        (dx + 1) + 3 * (dy + 1) + 9 * (dz + 1): see descend()); summary a COST_SUMMARY_DTYPE record."""
        o, d = _box3(origin, "origin"), _box3(dims, "dims")
        shape = _box_shape(d)
        g = np.ascontiguousarray(np.asarray(goals, dtype=np.int32).reshape(-1, 3))
        cost = np.empty(shape, dtype=np.uint32)
        nxt = np.empty(shape, dtype=np.uint8) if with_next else None
        summary = np.zeros(1, dtype=COST_SUMMARY_DTYPE)
        params = CostParams(float(occupied_below), float(clearance),
                            self._cost_flags(unknown_occupied, through_unknown, faces_only), 0)
        _check(self.lib.fn["cost_to_go"](self._h, o, d, C.byref(params), g.ctypes.data if len(g) else None, len(g),
                                         cost.ctypes.data, nxt.ctypes.data if with_next else None,
                                         summary.ctypes.data), "cost_to_go")
        return (cost, nxt, summary[0]) if with_next else (cost, summary[0])

    def cost_to_go_device(self, origin, dims, d_goals, n_goals, d_cost, d_next, d_summary, rounds, clearance=0.0,
                          occupied_below=0.0, unknown_occupied=False, through_unknown=False, faces_only=False,
                          resume=False):
        """cost_to_go() into DEVICE buffers, asynchronous on the engine's stream, with exactly `rounds` (1 .. 4096)
        relaxation rounds: the goals from d_goals (n_goals int32 triples, 16-byte aligned), the cost words to d_cost
        (16-byte aligned), the direction bytes to d_next (0 for none) and the 32-byte summary to d_summary (8-byte
        aligned).  summary["pending"] != 0: not converged yet -- the field is an upper bound that `next` still
        descends to a goal; call again with resume=True and the same arguments to go on from it.  Each buffer: a torch
        tensor, a devmem.DeviceArray or a raw pointer.  Returns the summary record (this waits for the stream)."""
        params = CostParams(float(occupied_below), float(clearance),
                            self._cost_flags(unknown_occupied, through_unknown, faces_only, resume), int(rounds))
        goals, cost, nxt, summary = _device_ptrs(d_goals, d_cost, d_next, d_summary)
        _check(self.lib.fn["cost_to_go_device"](self._h, _box3(origin, "origin"), _box3(dims, "dims"), C.byref(params),
                                                goals, int(n_goals), cost, nxt, summary), "cost_to_go_device")
        record = self._read_back(d_summary, COST_SUMMARY_DTYPE)
        return None if record is None else record[0]

    def label_set(self, points, labels, cell=0.0):
        """a LabelSet of n labelled points (ratsdf_labelset_create, include/ratsdf_score.h): points [n, 3] float32
        metres, labels [n] uint8 of LABEL_IGNORE / LABEL_LOW / LABEL_HIGH.  cell: the edge of the search grid's cells,
        0 for 8 voxel sizes of this engine.  With `points` and `labels` on the device (torch tensors or
        devmem.DeviceArray: float32 [n, 3] and uint8 [n], contiguous) it is built from them in place."""
        return self._labelled(LabelSet, "point", cell, (points, np.float32, (-1, 3)), (labels, np.uint8, (-1,)))

    def _labelled(self, cls, what, cell, xyz, *more):
        """label_set() and label_mesh(): a `cls` from (array, dtype, shape) triples, the positions first, then every
        further array, which goes to the library as a (pointer, items) pair.  Arrays on the device -- the positions
        have a data_ptr() -- are taken in place, others as contiguous host arrays of that dtype and shape."""
        h = C.c_void_p()
        if hasattr(xyz[0], "data_ptr"):
            symbol = cls._prefix + "_create_device"
            arrays = [a for a, _, _ in (xyz,) + more]
            counts = [int(a.shape[0]) if hasattr(a, "shape") else int(len(a)) for a in arrays[1:]]
            ptrs = [a.data_ptr() or None for a in arrays]
        else:
            symbol = cls._prefix + "_create"
            arrays = [np.ascontiguousarray(a, dtype=dtype).reshape(shape) for a, dtype, shape in (xyz,) + more]
            if arrays[1].shape[0] != arrays[0].shape[0]:
                raise ValueError(f"one label per {what}")
            counts = [len(a) for a in arrays[1:]]
            ptrs = [a.ctypes.data if len(a) else None for a in arrays]
        pairs = [v for pair in zip(ptrs[1:], counts) for v in pair]
        _check(self.lib.fn[symbol](self._h, ptrs[0], *pairs, C.c_float(float(cell)), C.byref(h)), symbol)
        return cls(self.lib, h)

    def score_labels(self, label_set, tsdf_below=0.1, max_dist=None, p_cutoff=0.5, min_weight=0, per_voxel=False):
        """the map scored against a LabelSet (ratsdf_score_labels): every voxel with |tsdf| < tsdf_below and weight >=
        min_weight takes the label of its nearest point within max_dist (default: 4 cells of the set) and counts by
        prob > p_cutoff against it.  Returns a LabelScore, with per_voxel also VOXEL_LABEL_DTYPE records in the order
        of gather_valid_semantic()."""
        return self._score("score_labels", label_set, tsdf_below, max_dist, p_cutoff, min_weight, per_voxel)

    def score_labels_device(self, label_set, d_score, d_per_voxel, capacity, d_count, tsdf_below=0.1, max_dist=None,
                            p_cutoff=0.5, min_weight=0):
        """score_labels() into DEVICE buffers, asynchronous on the engine's stream: the 4160-byte score to d_score, at
        most `capacity` 8-byte per-voxel records to d_per_voxel (0 for none) and the number of voxels as an int64 to
        d_count; all 8-byte aligned.  Each buffer: a torch tensor, a devmem.DeviceArray or a raw pointer.  Returns
        nothing: synchronize() before reading."""
        self._score_device("score_labels_device", label_set, d_score, d_per_voxel, capacity, d_count, tsdf_below,
                           max_dist, p_cutoff, min_weight)

    def _score(self, symbol, labelled, tsdf_below, max_dist, p_cutoff, min_weight, per_voxel):
        """score_labels() and score_mesh(): `symbol` against the LabelSet or LabelMesh `labelled`"""
        if max_dist is None:
            max_dist = 4.0 * labelled.info["cell"]
        params = ScoreParams(float(tsdf_below), float(max_dist), float(p_cutoff), int(min_weight), 0)
        rec = np.zeros((), dtype=LABEL_SCORE_DTYPE)
        records = self._call_owned(symbol, VOXEL_LABEL_DTYPE, labelled._h, C.byref(params), rec.ctypes.data,
                                   wanted=per_voxel)
        return (LabelScore(rec), records) if per_voxel else LabelScore(rec)

    def _score_device(self, symbol, labelled, d_score, d_per_voxel, capacity, d_count, tsdf_below, max_dist, p_cutoff,
                      min_weight):
        """score_labels_device() and score_mesh_device(): `symbol` against the LabelSet or LabelMesh `labelled`"""
        if max_dist is None:
            max_dist = 4.0 * labelled.info["cell"]
        params = ScoreParams(float(tsdf_below), float(max_dist), float(p_cutoff), int(min_weight), 0)
        score, records, count = _device_ptrs(d_score, d_per_voxel, d_count)
        _check(self.lib.fn[symbol](self._h, labelled._h, C.byref(params), score, records, int(capacity), count), symbol)

    def label_mesh(self, vertices, labels, triangles, cell=0.0):
        """a LabelMesh (ratsdf_labelmesh_create, include/ratsdf_score_mesh.h): vertices [n, 3] float32 metres, labels
        [n] uint8 of LABEL_IGNORE / LABEL_LOW / LABEL_HIGH, triangles [m, 3] int32 vertex indices; a triangle carries
        the label of its first vertex.  cell: the edge of the search grid's cells, 0 for 8 voxel sizes of this engine.
        With the three arrays on the device (torch tensors or devmem.DeviceArray: float32 [n, 3], uint8 [n] and
        int32 [m, 3], contiguous) it is built from them in place."""
        return self._labelled(LabelMesh, "vertex", cell, (vertices, np.float32, (-1, 3)), (labels, np.uint8, (-1,)),
                              (triangles, np.int32, (-1, 3)))

    def score_mesh(self, label_mesh, tsdf_below=0.1, max_dist=None, p_cutoff=0.5, min_weight=0, per_voxel=False):
        """the map scored against a LabelMesh (ratsdf_score_mesh): every voxel with |tsdf| < tsdf_below and weight >=
        min_weight takes the label of its nearest triangle within max_dist (default: 4 cells of the set) and counts
        by prob > p_cutoff against it.  Returns a LabelScore, with per_voxel also VOXEL_LABEL_DTYPE records (nearest:
        the triangle's index) in the order of gather_valid_semantic()."""
        return self._score("score_mesh", label_mesh, tsdf_below, max_dist, p_cutoff, min_weight, per_voxel)

    def score_mesh_device(self, label_mesh, d_score, d_per_voxel, capacity, d_count, tsdf_below=0.1, max_dist=None,
                          p_cutoff=0.5, min_weight=0):
        """score_mesh() into DEVICE buffers, asynchronous on the engine's stream, with the buffers of
        score_labels_device().  Returns nothing: synchronize() before reading."""
        self._score_device("score_mesh_device", label_mesh, d_score, d_per_voxel, capacity, d_count, tsdf_below,
                           max_dist, p_cutoff, min_weight)

    def gather_valid_mesh(self):
        """TSDFGrid::GatherValidMesh (voxel_tsdf.cu:736-845): (vertices [n,3] f32 metres,
        triangles [m,3] i32, per-vertex probability [n] f32)."""
        pv, pi, pp = C.c_void_p(), C.c_void_p(), C.c_void_p()
        nv, nt = C.c_size_t(), C.c_size_t()
        _check(self.lib.fn["gather_valid_mesh"](self._h, C.byref(pv), C.byref(nv), C.byref(pi),
                                                C.byref(nt), C.byref(pp)), "gather_valid_mesh")
        v = self._take(pv, nv.value * 3, np.dtype("<f4")).reshape(-1, 3)
        i = self._take(pi, nt.value * 3, np.dtype("<i4")).reshape(-1, 3)
        p = self._take(pp, nv.value, np.dtype("<f4"))
        return v, i, p

    def download_all_mesh(self, vertices_path, indices_path, prob_path):
        _check(self.lib.fn["download_all_mesh"](self._h, str(vertices_path).encode(),
                                                str(indices_path).encode(),
                                                str(prob_path).encode()), "download_all_mesh")

    def export_directory_device(self, d_blocks, capacity, d_count):
        _check(self.lib.fn["export_directory_device"](self._h, d_blocks, capacity, d_count),
               "export_directory_device")

    def export_directory_delta_device(self, d_payload, capacity, d_counts):
        """added / changed entries, then deleted positions, since the previous call; d_payload = 0: forget them"""
        _check(self.lib.fn["export_directory_delta_device"](self._h, d_payload or None, capacity, d_counts or None),
               "export_directory_delta_device")

    def import_blocks(self, block_pos, tsdf, rgbw, prob):
        """blocks copied in from another map (a neighbour rank's subvolume): positions [n, 3] int16 and the three
        voxel arrays [n, 512] in dump_voxels()'s layout; inserted whatever the shard filter says"""
        a, n = self._s3(block_pos)
        t = np.ascontiguousarray(tsdf, dtype=np.float32).reshape(n, BLOCK_VOLUME)
        c = np.ascontiguousarray(rgbw, dtype=RGBW_DTYPE).reshape(n, BLOCK_VOLUME)
        p = np.ascontiguousarray(prob, dtype=np.float32).reshape(n, BLOCK_VOLUME)
        _check(self.lib.fn["import_blocks"](self._h, n, a.ctypes.data, t.ctypes.data, c.ctypes.data, p.ctypes.data),
               "import_blocks")

    def export_blocks_device(self, n, d_block_pos, d_voxels, d_missing):
        """record i of d_voxels (1536 words: tsdf | rgbw | prob) = the voxels of the block at position i of d_block_pos
        (n x 3 int16); all three are device pointers; *d_missing (int32) counts listed blocks the map does not hold.
        Asynchronous on the engine's stream."""
        _check(self.lib.fn["export_blocks_device"](self._h, int(n), d_block_pos or None, d_voxels or None, d_missing),
               "export_blocks_device")

    def import_blocks_device(self, n, d_block_pos, d_voxels):
        """import_blocks() from device buffers in export_blocks_device()'s layout (read on the engine's stream)"""
        _check(self.lib.fn["import_blocks_device"](self._h, int(n), d_block_pos or None, d_voxels or None),
               "import_blocks_device")

    # -- map fusion (include/ratsdf_fuse.h) ------------------------------------------------
    def _fuse(self, name, *args):
        """calls a fusion entry point; returns its statistics as a dict (filled in even when the call fails: the
        blocks fused before an error stay fused) -- raises RatsdfError carrying them as ``.fuse_stats``"""
        st = np.zeros(1, dtype=FUSE_STATS)
        rc = self.lib.fn[name](self._h, *args, st.ctypes.data)
        stats = {k: int(st[0][k]) for k in FUSE_STATS.names}
        if rc != 0:
            err = RatsdfError(rc, name)
            err.fuse_stats = stats
            raise err
        return stats

    def fuse_map(self, src):
        """merges the map of ``src`` (an Engine on the same device, same voxel size and truncation) into this map with
        the weighted-average voxel update; ``src`` is only read.  Returns the statistics."""
        return self._fuse("fuse_map", src._h)

    def fuse_blocks(self, block_pos, tsdf, rgbw, prob):
        """fuses blocks given as import_blocks() takes them (positions must be distinct)"""
        a, n = self._s3(block_pos)
        t = np.ascontiguousarray(tsdf, dtype=np.float32).reshape(n, BLOCK_VOLUME)
        c = np.ascontiguousarray(rgbw, dtype=RGBW_DTYPE).reshape(n, BLOCK_VOLUME)
        p = np.ascontiguousarray(prob, dtype=np.float32).reshape(n, BLOCK_VOLUME)
        return self._fuse("fuse_blocks", n, a.ctypes.data, t.ctypes.data, c.ctypes.data, p.ctypes.data)

    def fuse_blocks_device(self, n, d_block_pos, d_voxels):
        """fuse_blocks() from device buffers in export_blocks_device()'s layout (positions must be distinct)"""
        return self._fuse("fuse_blocks_device", int(n), d_block_pos or None, d_voxels or None)

    def fuse_map_file(self, path):
        """fuses a checkpoint written by save_map() into this map (only voxel size and truncation must agree)"""
        return self._fuse("fuse_map_file", os.fsencode(path))

    # -- transformed map fusion (include/ratsdf_resample.h) --------------------------------
    def fuse_map_transformed(self, src, dst_T_src):
        """resamples the map of ``src`` onto this map's lattice under ``dst_T_src`` (qx, qy, qz, qw, tx, ty, tz as
        ratsdf.pose builds it: p_dst = R(q) p_src + t in metres, a map-to-map pose) and fuses it; ``src`` is only
        read.  Returns the statistics (raises like the other fusion calls)."""
        p = _as_pose(dst_T_src)
        return self._fuse("fuse_map_transformed", src._h, C.byref(p))

    def resample_blocks_device(self, dst_T_src, n, d_block_pos, d_voxels, d_contrib=0):
        """blocks of the DESTINATION lattice (d_block_pos: n x 3 int16) filled from this map seen through
        ``dst_T_src``: d_voxels gets n records in export_blocks_device()'s layout, d_contrib (or 0) one int32 per
        block, the number of contributing voxels.  Device pointers; asynchronous on this engine's stream."""
        p = _as_pose(dst_T_src)
        _check(self.lib.fn["resample_blocks_device"](self._h, C.byref(p), int(n), d_block_pos or None,
                                                     d_voxels or None, d_contrib or None), "resample_blocks_device")

    # -- map coarsening (include/ratsdf_coarsen.h) -----------------------------------------
    def fuse_map_coarsened(self, src):
        """coarsens the map of ``src`` (an Engine on the same device, of HALF this map's voxel size and the same
        truncation) by two and fuses it into this map; ``src`` is only read.  Returns the statistics (raises like the
        other fusion calls)."""
        return self._fuse("fuse_map_coarsened", src._h)

    def coarsen_blocks_device(self, n, d_block_pos, d_voxels, d_contrib=0):
        """blocks of the lattice of TWICE this map's voxel size (d_block_pos: n x 3 int16) filled from this map:
        d_voxels gets n records in export_blocks_device()'s layout, d_contrib (or 0) one int32 per block, the number of
        contributing voxels.  Device pointers; asynchronous on this engine's stream."""
        _check(self.lib.fn["coarsen_blocks_device"](self._h, int(n), d_block_pos or None, d_voxels or None,
                                                    d_contrib or None), "coarsen_blocks_device")

    def coarsened(self, levels=1, **create_kw):
        """a new engine of the same library, device and truncation holding this map at float32(voxel_size) *
        2**levels: `levels` coarsenings by two in a chain (1 .. 8), each temporary level destroyed as soon as the next
        one exists.  ``create_kw`` (block_bits, bucket_bits, ...) goes to every engine of the chain.  The caller closes
        the result."""
        levels = int(levels)
        if not 1 <= levels <= 8:
            raise ValueError("levels must lie in 1 .. 8")
        create_kw.setdefault("device", self.device)
        cur = self
        try:
            for _ in range(levels):
                vs = float(np.float32(2.0) * np.float32(cur.voxel_size))
                nxt = object.__new__(type(self))  # (a TSDFGrid stays a TSDFGrid: it adds no state of its own)
                Engine.__init__(nxt, self.lib, vs, self.truncation, **create_kw)
                try:
                    nxt.fuse_map_coarsened(cur)
                except Exception:
                    nxt.close()
                    raise
                if cur is not self:
                    cur.close()
                cur = nxt
        except Exception:
            if cur is not self:
                cur.close()
            raise
        return cur

    # -- test hooks ------------------------------------------------------------------------
    @staticmethod
    def _s3(a):
        a = np.ascontiguousarray(a, dtype=np.int16).reshape(-1, 3)
        return a, a.shape[0]

    def test_allocate(self, block_pos):
        a, n = self._s3(block_pos)
        _check(self.lib.fn["test_allocate"](self._h, a.ctypes.data, n), "test_allocate")

    def test_delete(self, block_pos):
        a, n = self._s3(block_pos)
        _check(self.lib.fn["test_delete"](self._h, a.ctypes.data, n), "test_delete")

    def test_retrieve(self, points):
        a, n = self._s3(points)
        rgbw = np.zeros(n, dtype=RGBW_DTYPE)
        tsdf = np.zeros(n, dtype=np.float32)
        prob = np.zeros(n, dtype=np.float32)
        blocks = np.zeros(n, dtype=BLOCK_DTYPE)
        _check(self.lib.fn["test_retrieve"](self._h, a.ctypes.data, n, rgbw.ctypes.data,
                                            tsdf.ctypes.data, prob.ctypes.data,
                                            blocks.ctypes.data), "test_retrieve")
        return rgbw, tsdf, prob, blocks

    def test_assign_rgbw(self, points, values):
        a, n = self._s3(points)
        v = np.ascontiguousarray(values, dtype=RGBW_DTYPE).reshape(-1)
        if v.shape[0] != n:
            raise ValueError("values must match points")
        _check(self.lib.fn["test_assign_rgbw"](self._h, a.ctypes.data, v.ctypes.data, n),
               "test_assign_rgbw")

    def dump_directory(self):
        pe, pb, n = C.c_void_p(), C.c_void_p(), C.c_size_t()
        _check(self.lib.fn["dump_directory"](self._h, C.byref(pe), C.byref(pb), C.byref(n)),
               "dump_directory")
        return (self._take(pe, n.value, np.dtype("<i4")), self._take(pb, n.value, BLOCK_DTYPE))

    def dump_voxels(self, pool_idx):
        idx = np.ascontiguousarray(pool_idx, dtype=np.int32).reshape(-1)
        n = idx.shape[0]
        tsdf = np.zeros((n, BLOCK_VOLUME), dtype=np.float32)
        rgbw = np.zeros((n, BLOCK_VOLUME), dtype=RGBW_DTYPE)
        prob = np.zeros((n, BLOCK_VOLUME), dtype=np.float32)
        _check(self.lib.fn["dump_voxels"](self._h, idx.ctypes.data, n, tsdf.ctypes.data,
                                          rgbw.ctypes.data, prob.ctypes.data), "dump_voxels")
        return tsdf, rgbw, prob

    def dump_heap(self):
        nf = C.c_int32()
        heap = np.zeros(1 << self.block_bits, dtype=np.int32)
        _check(self.lib.fn["dump_heap"](self._h, C.byref(nf), heap.ctypes.data), "dump_heap")
        return nf.value, heap


class Group:
    """Several engines of one GPU stepped together (ratsdf_group_*): frame f of every member stream
    goes through one launch triple.  Members stay usable on their own between group calls."""

    def __init__(self, engines):
        self.engines = list(engines)
        self.lib = self.engines[0].lib
        arr = (C.c_void_p * len(self.engines))(*[e._h for e in self.engines])
        h = C.c_void_p()
        _check(self.lib.fn["group_create"](arr, len(self.engines), C.byref(h)), "group_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self.lib.fn["group_destroy"](self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def make_batch(self, d_rgb, d_depth, d_ht, d_lt, height, width, max_depth, intrinsics, poses):
        """Arguments are lists over frames of lists over members (raw device pointers, intrinsics,
        poses); returns an opaque tuple for integrate_device_batch."""
        n, s = len(d_rgb), len(self.engines)
        flat = lambda rows: [v for row in rows for v in row]
        arr = lambda rows: (C.c_void_p * (n * s))(*flat(rows)) if rows is not None else None
        ks = (Intrinsics * (n * s))(*[_as_intr(k) for k in flat(intrinsics)])
        ps = (Pose * (n * s))(*[_as_pose(p) for p in flat(poses)])
        return (n, arr(d_rgb), arr(d_depth), arr(d_ht), arr(d_lt), int(height), int(width),
                float(max_depth), ks, ps)

    def integrate_device_batch(self, batch):
        n, rgb, depth, ht, lt, h, w, md, ks, ps = batch
        _check(self.lib.fn["group_integrate_device_batch"](self._h, n, rgb, depth, ht, lt, h, w, md,
                                                           ks, ps), "group_integrate_device_batch")

    def synchronize(self):
        _check(self.lib.fn["group_synchronize"](self._h), "group_synchronize")

    def profile_enable(self, on=True):
        _check(self.lib.fn["group_profile_enable"](self._h, 1 if on else 0), "group_profile_enable")

    def profile_read(self):
        ms, n = C.c_double(), C.c_int64()
        _check(self.lib.fn["group_profile_read"](self._h, C.byref(ms), C.byref(n)),
               "group_profile_read")
        return ms.value, n.value
