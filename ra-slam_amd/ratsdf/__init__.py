"""ratsdf -- Python host binding of the MI355X-native TSDF engine (libratsdf.so, HIP / gfx950).

The binding loads the in-tree C-ABI library built from ``ra-slam_amd/csrc`` and nothing else: there
is no CPU fallback.  If the HIP library has not been built the import of an engine fails loudly.
"""
import os
from pathlib import Path

from . import _abi
from ._abi import (BLOCK_DTYPE, ESDF_STATE_FREE, ESDF_STATE_OCCUPIED, ESDF_STATE_UNKNOWN, ESDF_UNKNOWN_OCCUPIED,
                   REGION_DTYPE, RGBW_DTYPE, SAMPLE_DTYPE, SURFACE_DTYPE, VOXEL_SEGM_DTYPE, VOXEL_TSDF_DTYPE, Bounds,
                   Engine, Group, Intrinsics, Library, Pose, RatsdfError, RegionsParams, voxel_box)
from ._abi import (LABEL_HIGH, LABEL_IGNORE, LABEL_LOW, LABEL_SCORE_DTYPE, VOXEL_LABEL_DTYPE, LabelScore, LabelSet,
                   ScoreParams)
from ._abi import LabelMesh, LabelMeshInfo
from ._abi import ClusterMeshParams
from ._abi import (COST_AT_GOAL, COST_CONTINUE, COST_FACES_ONLY, COST_NO_STEP, COST_NONE, COST_SUMMARY_DTYPE,
                   COST_THROUGH_UNKNOWN, COST_UNKNOWN_OCCUPIED, CostParams, cost_direction, descend)
from ._abi import (EXPOSURE_ACCUMULATE, EXPOSURE_MAX_LAMPS, EXPOSURE_SUMMARY_DTYPE, EXPOSURE_UNKNOWN_OCCUPIED, LAMP_DTYPE,
                   LAMP_RECORD_DTYPE, ExposureParams)
from .pose import compose, identity_pose, invert, pose_from_matrix

_PKG_ROOT = Path(__file__).resolve().parent.parent
LIB_PATH = _PKG_ROOT / "csrc" / "build" / "libratsdf.so"
_lib = None


def library():
    """The HIP engine library; raises if it has not been built (no fallback exists)."""
    global _lib
    if _lib is None:
        path = Path(os.environ.get("RATSDF_LIB", LIB_PATH))
        if not path.exists():
            raise ImportError(
                f"{path} not found: build the HIP engine first "
                f"(python -c 'import __graft_entry__ as g; g.build()' or make -C ra-slam_amd/csrc)")
        _lib = Library(path, "ratsdf_")
    return _lib


def map_file_info(path):
    """Validates a map checkpoint on the host (no device needed) and returns its configuration and the number of live
    blocks: ``{voxel_size, truncation, block_bits, bucket_bits, shard_rank, shard_count, shard_slab_bits,
    n_blocks}``.  Raises RatsdfError (status 1) for a malformed or corrupted file."""
    return library().map_file_info(path)


class TSDFGrid(Engine):
    """``TSDFGrid(voxel_size, truncation)`` of utils/tsdf/voxel_tsdf.cuh:47 on one MI355X."""

    def __init__(self, voxel_size, truncation, device=0, **kw):
        super().__init__(library(), voxel_size, truncation, device=device, **kw)


__all__ = ["TSDFGrid", "Engine", "Group", "Library", "library", "Intrinsics", "Pose", "Bounds",
           "RatsdfError", "map_file_info", "pose_from_matrix", "compose", "invert", "identity_pose", "BLOCK_DTYPE",
           "RGBW_DTYPE", "SAMPLE_DTYPE", "VOXEL_TSDF_DTYPE", "VOXEL_SEGM_DTYPE", "LIB_PATH", "voxel_box",
           "ESDF_UNKNOWN_OCCUPIED", "ESDF_STATE_UNKNOWN", "ESDF_STATE_FREE", "ESDF_STATE_OCCUPIED",
           "SURFACE_DTYPE", "REGION_DTYPE", "RegionsParams", "LABEL_SCORE_DTYPE", "VOXEL_LABEL_DTYPE", "ScoreParams",
           "LabelSet", "LabelScore", "LABEL_IGNORE", "LABEL_LOW", "LABEL_HIGH", "LabelMesh", "LabelMeshInfo",
           "ClusterMeshParams", "CostParams", "COST_SUMMARY_DTYPE", "COST_NONE", "COST_AT_GOAL", "COST_NO_STEP",
           "COST_UNKNOWN_OCCUPIED", "COST_THROUGH_UNKNOWN", "COST_FACES_ONLY", "COST_CONTINUE",
           "cost_direction", "descend", "ExposureParams", "LAMP_DTYPE", "LAMP_RECORD_DTYPE",
           "EXPOSURE_SUMMARY_DTYPE", "EXPOSURE_UNKNOWN_OCCUPIED", "EXPOSURE_ACCUMULATE", "EXPOSURE_MAX_LAMPS"]
