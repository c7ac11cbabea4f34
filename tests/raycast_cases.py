"""Crafted maps and views for the ray cast (k_raycast / k_occupancy_build, ra-slam_amd/csrc/kernels_raycast.h),
written once and run against the CPU oracle (tests/test_raycast_cases.py, no GPU) and the HIP engine
(tests/test_gpu_raycast.py).  Same role as kat_cases.py / mixed_cases.py: no GPU and no torch at import.

The maps are written voxel by voxel (import_blocks), never integrated from frames: a plane or a sphere with a signed
distance known in closed form, a colour that is a function of the voxel's integer coordinates (a wrong voxel shows) and a
probability on either side of 0.5 (both alpha branches of voxel_tsdf.cu:350 occur).  Voxel v sits at v * VS metres; a
block b holds voxels 8b .. 8b + 7 per axis, in dump_voxels() order (x + 8y + 64z).
"""
import functools
import math
from typing import Callable, NamedTuple

import numpy as np

from ratsdf import pose as se3
from ratsdf._abi import RGBW_DTYPE

VS = 0.02
TRUNC = 6 * VS
TRUNC_VOXELS = 6.0            # TRUNC / VS
KEEP_VOXELS = 13.0            # a block is kept when its centre is this close to the surface
WEIGHT = 40
F = np.float32


class BlockSet(NamedTuple):
    """what import_blocks() takes"""
    pos: np.ndarray    # [n, 3] int16
    tsdf: np.ndarray   # [n, 512] float32
    rgbw: np.ndarray   # [n, 512] RGBW_DTYPE
    prob: np.ndarray   # [n, 512] float32

    def __len__(self):
        return len(self.pos)

    def take(self, rows):
        return BlockSet(*(a[rows] for a in self))


def concat(*sets):
    return BlockSet(*(np.concatenate([s[i] for s in sets]) for i in range(4)))


def block_keys(pos):
    """one int64 per block position"""
    p = np.asarray(pos).astype(np.int64) & 0xFFFF
    return p[..., 0] | (p[..., 1] << 16) | (p[..., 2] << 32)


def block_voxels(pos):
    """integer voxel coordinates [n, 512, 3] of the blocks at `pos`, in dump_voxels() order"""
    i = np.arange(512)
    local = np.stack([i & 7, (i >> 3) & 7, i >> 6], axis=1)
    return np.asarray(pos, dtype=np.int64)[:, None, :] * 8 + local[None]


def _from_distance(pos, dist):
    """the block set whose voxels lie `dist` voxels in front of (+) / behind (-) the surface"""
    v = block_voxels(pos)
    nd = dist / TRUNC_VOXELS                       # signed distance * vs / truncation
    rgbw = np.zeros(nd.shape, dtype=RGBW_DTYPE)
    rgbw["r"] = (37 * v[..., 0]) & 255
    rgbw["g"] = (59 * v[..., 1]) & 255
    rgbw["b"] = (83 * v[..., 2]) & 255
    rgbw["weight"] = np.where(np.abs(nd) <= 1, WEIGHT, 0)
    prob = 0.3 + 0.5 * ((v[..., 0] + v[..., 1]) & 15) / 15
    return BlockSet(np.asarray(pos, dtype=np.int16), np.clip(nd, -1, 1).astype(F), rgbw, prob.astype(F))


def _cube(lo, hi):
    """all integer points of [lo, hi) per axis, [n, 3]"""
    ax = [np.arange(int(a), int(b)) for a, b in zip(lo, hi)]
    return np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, 3)


def block_centre(block):
    return np.asarray(block, dtype=np.float64) * 8 + 3.5


def plane_patch(normal, centre_block, half_blocks, cube_block=None):
    """A plane through the centre of `centre_block`, `normal` pointing to its front (tsdf > 0) side: the blocks of the
    cube centre_block - half_blocks .. centre_block + half_blocks - 1 whose centre lies within KEEP_VOXELS of it.
    cube_block: the cube's centre block where it is not the plane's (a further piece of the same plane)."""
    n = np.asarray(normal, dtype=np.float64)
    n = n / np.linalg.norm(n)
    cb = np.asarray(centre_block, dtype=np.int64)
    mid = cb if cube_block is None else np.asarray(cube_block, dtype=np.int64)
    lo, hi = np.maximum(mid - half_blocks, -4096), np.minimum(mid + half_blocks, 4096)
    pos = _cube(lo, hi)
    c = block_centre(cb)
    pos = pos[np.abs((block_centre(pos) - c) @ n) <= KEEP_VOXELS]
    return _from_distance(pos, (block_voxels(pos) - c) @ n)


def sphere_shell(centre_voxel, radius_voxels):
    """The same for a sphere (front = outside): a silhouette against empty space, all normal directions."""
    c = np.asarray(centre_voxel, dtype=np.float64)
    reach = int(math.ceil((radius_voxels + KEEP_VOXELS) / 8)) + 1
    cb = np.floor(c / 8).astype(np.int64)
    pos = _cube(cb - reach, cb + reach + 1)
    pos = pos[np.abs(np.linalg.norm(block_centre(pos) - c, axis=1) - radius_voxels) <= KEEP_VOXELS]
    return _from_distance(pos, np.linalg.norm(block_voxels(pos) - c, axis=2) - radius_voxels)


def wall_patch(x_block=0):
    """the `far` wall: blocks x in [x_block - 2, x_block + 2), y in [-6, 6), z in [6, 9), its face at z = 60.3 voxels;
    weight 40 everywhere, green varying with y"""
    pos = _cube((x_block - 2, -6, 6), (x_block + 2, 6, 9))
    v = block_voxels(pos)
    s = _from_distance(pos, 60.3 - v[..., 2].astype(np.float64))
    s.rgbw["weight"] = WEIGHT
    s.rgbw["g"] = (11 * v[..., 1]) & 255
    return s


# ---------------------------------------------------------------------------------------------------------------------
# The hashes of the occupancy filter.  KEEP IN STEP WITH ra-slam_amd/csrc/kernels_raycast.h (occ_bit, occ_bit2,
# cell_bit, kOccWords, kCellWords, kCellVoxelBits): __umul24 multiplies the low 24 bits and keeps the low 32 of the product.
OCC_BITS = 4096 * 32
CELL_BITS = 1024 * 32
CELL_BLOCK_SHIFT = 2          # kCellVoxelBits - 3: a super-cell is 4^3 blocks


def _mad3(p, kx, ky, kz):
    q = np.asarray(p).astype(np.int64) & 0xFFFF
    m = 0xFFFFFFFF
    return (((q[..., 0] * kx) & m) + ((q[..., 1] * ky) & m) + ((q[..., 2] * kz) & m)) & m


def occ_bit(blocks):
    return _mad3(blocks, 0x9E5, 0x1F35B, 0x6A7C1) & (OCC_BITS - 1)


def occ_bit2(blocks):
    return (_mad3(blocks, 0x2C1B3, 0x5D3, 0x1B873) >> 3) & (OCC_BITS - 1)


def cell_bit(cells):
    return _mad3(cells, 0x9E5, 0x1F35B, 0x6A7C1) & (CELL_BITS - 1)


def cells_of(blocks):
    return np.asarray(blocks).astype(np.int64) >> CELL_BLOCK_SHIFT


DECOY_REGION = ((1000, 1000, 1000), 96)


def filter_decoys(targets, region=DECOY_REGION):
    """Blocks of `region` (a cube of blocks: (offset, side), well outside every view) that set, between them, both Bloom
    bits of every block of `targets` and the cell bit of its super-cell: with them in the map a sample in a target block
    finds its cell bit set and both block bits set, and has to learn from the directory that the block is absent.  The
    cell bit hashes the CELL's coordinates, so cells are searched: side^3 cells from the region's first cell on, each
    represented by its first block.  Decoys carry tsdf 1, weight 0: nothing to render."""
    targets = np.unique(np.asarray(targets, dtype=np.int64).reshape(-1, 3), axis=0)
    off, side = np.asarray(region[0], dtype=np.int64), int(region[1])
    cand = _cube(off, off + side)
    cand_cells = _cube(off >> CELL_BLOCK_SHIFT, (off >> CELL_BLOCK_SHIFT) + side)

    def first_match(cand_hash, want):
        order = np.argsort(cand_hash, kind="stable")
        at = np.searchsorted(cand_hash[order], want)
        ok = (at < len(order)) & (cand_hash[order][np.minimum(at, len(order) - 1)] == want)
        assert ok.all(), f"{int((~ok).sum())} of {len(want)} bits have no decoy in the region"
        return order[at]

    picked = [cand[first_match(occ_bit(cand), occ_bit(targets))],
              cand[first_match(occ_bit2(cand), occ_bit2(targets))],
              cand_cells[first_match(cell_bit(cand_cells), cell_bit(cells_of(targets)))] << CELL_BLOCK_SHIFT]
    decoys = np.unique(np.concatenate(picked), axis=0)
    # the coverage this builder promises, by the decoys alone
    assert not np.isin(block_keys(decoys), block_keys(targets)).any()
    assert np.isin(occ_bit(targets), occ_bit(decoys)).all() and np.isin(occ_bit2(targets), occ_bit2(decoys)).all()
    assert np.isin(cell_bit(cells_of(targets)), cell_bit(cells_of(decoys))).all()
    n = len(decoys)
    return BlockSet(decoys.astype(np.int16), np.ones((n, 512), F), np.zeros((n, 512), RGBW_DTYPE),
                    np.full((n, 512), 0.5, F))


# ---------------------------------------------------------------------------------------------------------------------
# views
class View(NamedTuple):
    name: str
    build: Callable        # () -> BlockSet (memoised: the CPU and the GPU test share one map per case)
    K: tuple               # fx, fy, cx, cy
    H: int
    W: int
    pose: tuple            # cam_T_world (qx, qy, qz, qw, tx, ty, tz)
    max_depth: float
    hit_share: tuple       # (lo, hi) the oracle's share of rendered pixels must lie in
    surface: tuple = None  # ("plane", unit normal, point) / ("sphere", centre, radius), voxels: closed-form shading


def centred(f, H, W):
    return (float(f), float(f), (W - 1) / 2.0, (H - 1) / 2.0)


def look(position_voxels, yaw_deg=0.0):
    """cam_T_world of a camera at `position_voxels` looking along +z turned by `yaw_deg` about y (towards +x)"""
    a = math.radians(yaw_deg)
    m = np.eye(4)
    m[:3, :3] = [[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]]  # world_R_cam
    m[:3, 3] = np.asarray(position_voxels, dtype=np.float64) * VS
    if yaw_deg == 0.0:
        return (0.0, 0.0, 0.0, 1.0) + tuple(float(-v) for v in m[:3, 3])
    return se3.invert(se3.pose_from_matrix(m))


PLANE_NORMAL = (0.2, -0.3, -1.0)


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v)


def on_plane(centre_block, dx=0.0, dy=0.0, normal=PLANE_NORMAL):
    """the point of the patch's plane at lateral offset (dx, dy) voxels from the centre of centre_block"""
    n = _unit(normal)
    c = block_centre(centre_block)
    return c + np.array([dx, dy, -(n[0] * dx + n[1] * dy) / n[2]])


@functools.lru_cache(maxsize=None)
def patch(centre_block):
    return plane_patch(PLANE_NORMAL, centre_block, 6)


def _plane_view(name, centre_block, dx=0.0, yaw=0.0, H=50, W=77, max_depth=3.0, hit_share=(0.9, 1.0), back=50.0):
    at = on_plane(centre_block, dx)
    a = math.radians(yaw)
    cam = at - back * np.array([math.sin(a), 0.0, math.cos(a)])
    return View(name, functools.partial(patch, tuple(centre_block)), centred(80, H, W), H, W, look(cam, yaw), max_depth,
                hit_share, ("plane", _unit(PLANE_NORMAL), block_centre(centre_block)))


ORIGIN, NEGATIVE, EDGE_HI, EDGE_LO = (0, 0, 0), (-300, -200, -250), (4090, 0, 0), (-4090, 0, 0)
SIZES = ((1, 1), (1, 16), (33, 17), (50, 77), (120, 160))
SPHERE_CENTRE, SPHERE_RADIUS = (3.0, -5.0, 110.0), 40.0


@functools.lru_cache(maxsize=None)
def sphere():
    return sphere_shell(SPHERE_CENTRE, SPHERE_RADIUS)


def octants_view():
    return _plane_view("octants", ORIGIN)


def rim_view():
    # turned 35 degrees towards +x and aimed at the patch's -x rim (voxel x = -48): the patch fills the right half
    return _plane_view("rim", ORIGIN, dx=-51.5, yaw=35.0, max_depth=6.0, hit_share=(0.2, 0.8))


def plane_views():
    """octants, negative, edge_hi, edge_lo, rim"""
    return [octants_view(),
            _plane_view("negative", NEGATIVE),
            # the camera 22 voxels inside the end of the voxel range: the patch's rim there, and the rays that pass it
            # (their voxel x wraps round to the other end of the range), take the image's last columns
            _plane_view("edge_hi", EDGE_HI, dx=32745 - block_centre(EDGE_HI)[0]),
            _plane_view("edge_lo", EDGE_LO, dx=-32749 - block_centre(EDGE_LO)[0]),
            rim_view()]


def sphere_views():
    """from outside (1.2 m from the surface; f = 60 so that the silhouette and empty space share the image), and from
    inside the shell's band of voxels: 4 voxels in front of the surface, turned 60 degrees so that some rays miss"""
    c = np.asarray(SPHERE_CENTRE)
    surf = ("sphere", c, SPHERE_RADIUS)
    return [View("sphere", sphere, centred(60, 50, 77), 50, 77, look(c - [0, 0, SPHERE_RADIUS + 60]), 4.0, (0.2, 0.8),
                 surf),
            View("sphere_inside", sphere, centred(60, 50, 77), 50, 77, look(c - [0, 0, SPHERE_RADIUS + 4], 60.0), 4.0,
                 (0.2, 0.8), surf)]


def size_views():
    return [_plane_view(f"sizes_{H}x{W}", ORIGIN, H=H, W=W, hit_share=(0.0, 1.0)) for H, W in SIZES]


def row_ranges(H):
    """(0,H), (1,2), (H-3,H), (k,k), cut to the image"""
    k = H // 2
    want = [(0, H), (1, 2), (H - 3, H), (k, k)]
    return sorted({(max(min(a, H), 0), max(min(b, H), 0)) for a, b in want})


def short_views():
    """max_step 1 and 2 (the loop is not entered / runs once), and the last max_step at which no ray of the octants view
    has reached its crossing sample"""
    v = octants_view()
    first = int(march(v.build(), v)["cross_i"].min())
    assert first > 8
    step = float(F(TRUNC) / F(2))
    return [v._replace(name=f"short_{n}", max_depth=(n - 0.5) * step, hit_share=(0.0, 0.0), surface=None)
            for n in (1, 2, first)]


def _far_tx(voxels):
    """a float32 tx with (-tx) / vs == `voxels` in float32 (what the march starts from)"""
    t = F(voxels) * F(VS)
    for _ in range(64):
        q = F(t) / F(VS)
        if q == F(voxels) or (voxels >= 2.0 ** 31 and q >= F(2.0 ** 31)):   # (beyond int32 the conversion saturates)
            return -float(t)
        t = np.nextafter(F(t), F(np.inf) if q < F(voxels) else F(-np.inf))
    raise AssertionError(f"no float32 tx reaches {voxels} voxels")


def wrapped_voxel(v):
    """(short)roundf(v) as both implementations evaluate it: saturating conversion to int32, then the low 16 bits"""
    i = int(np.clip(np.round(np.float64(F(v))), -2 ** 31, 2 ** 31 - 1))
    return ((i + 32768) & 0xFFFF) - 32768


FAR_START = (2.0 ** 30, 2.0 ** 30 + 3 * 65536, 3e9)
FAR_MIXED_START = 999999936.0   # the last float32 but one below 1e9: see far_views()


def far_views():
    """Ray origins whose voxel x is beyond the short form of (short)roundf (`small == false` in k_raycast).  The step is
    absorbed by such an x, so every ray keeps the wrapped voxel x it starts with: 0, 0 and -1 (saturated).  The fourth
    view starts 64 voxels below 1e9: `|p.x| + reach * |step.x| < 1e9` then holds for the lanes whose reach * |step.x|
    stays below 32 (it rounds back down) and fails for the others, inside one 16x4-pixel wave."""
    H, W = 40, 50
    out = []
    for i, start in enumerate(FAR_START + (FAR_MIXED_START,)):
        x = wrapped_voxel(start)
        assert x % 8 == 0 or x == -1
        build = functools.partial(far_wall, x >> 3)
        name = f"far_{i}" if start != FAR_MIXED_START else "far_mixed"
        out.append(View(name, build, centred(60, H, W), H, W, (0.0, 0.0, 0.0, 1.0, _far_tx(start), 0.0, 0.0), 3.0,
                        (1.0, 1.0)))
    return out


@functools.lru_cache(maxsize=None)
def far_wall(x_block):
    return wall_patch(x_block)


def far_mixed_lanes(v):
    """per pixel: does the lane's own term of k_raycast's `small` test hold (float32, as the kernel evaluates it)"""
    d = ray_directions(v).astype(F)
    reach = F(math.ceil(F(v.max_depth) / (F(TRUNC) / F(2))))
    full_x = d[..., 0] * (F(TRUNC) / F(2)) / F(VS)
    return np.abs(F(-v.pose[4]) / F(VS)) + reach * np.abs(full_x) < F(1e9)


@functools.lru_cache(maxsize=None)
def collisions_map():
    v = octants_view()
    m = v.build()
    return concat(m, filter_decoys(march(m, v, full_step_only=True)["absent"]))


def collisions_view():
    return octants_view()._replace(name="collisions", build=collisions_map)


def views():
    """every named case's views (the `edited` and `chains` sequences are driven by the GPU test on octants / rim)"""
    return plane_views() + sphere_views() + size_views() + short_views() + [collisions_view()] + far_views()


def extension(m, count=50):
    """`count` blocks that extend the octants patch: the next slab of its plane in +x (blocks x = 6, 7)"""
    more = plane_patch(PLANE_NORMAL, ORIGIN, 6, cube_block=(12, 0, 0))
    new = more.take(~np.isin(block_keys(more.pos), block_keys(m.pos)))
    new = new.take(np.argsort(block_keys(new.pos[:, [1, 2, 0]]), kind="stable")[:count])   # x slowest: a connected slab
    assert len(new) == count
    return new


# ---------------------------------------------------------------------------------------------------------------------
# the march in numpy (voxel_tsdf.cu:278-374 as the oracle restates it), for designing cases and for re-marching the rays
# of differing pixels -- float32 like the implementations, though not promised bit-equal to them
class Lookup:
    def __init__(self, m):
        self.m = m
        k = block_keys(m.pos)
        self.order = np.argsort(k)
        self.keys = k[self.order]

    def rows(self, vox):
        """block row of integer voxels [..., 3] (int16 range), -1 where the block is absent"""
        k = block_keys(np.asarray(vox).astype(np.int64) >> 3)
        at = np.minimum(np.searchsorted(self.keys, k), len(self.keys) - 1)
        return np.where(self.keys[at] == k, self.order[at], -1)

    def fetch(self, vox):
        """(tsdf, weight, block present) at integer voxels [..., 3]"""
        vox = np.asarray(vox).astype(np.int64)
        r = self.rows(vox)
        i = (vox[..., 0] & 7) + (vox[..., 1] & 7) * 8 + (vox[..., 2] & 7) * 64
        ok = r >= 0
        rr = np.where(ok, r, 0)
        return (np.where(ok, self.m.tsdf[rr, i], F(-10)), np.where(ok, self.m.rgbw["weight"][rr, i], 0), ok)


def ray_directions(v, dtype=np.float64):
    """world directions [H, W, 3] of the view's pixel rays (unit) in float64"""
    fx, fy, cx, cy = v.K
    x, y = np.meshgrid(np.arange(v.W, dtype=np.float64), np.arange(v.H, dtype=np.float64))
    d = np.stack([(x - cx) / fx, (y - cy) / fy, np.ones_like(x)], axis=-1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    q = np.asarray(se3.invert(v.pose)[:4], dtype=np.float64)
    qv, w = q[:3], q[3]
    uv = 2 * np.cross(np.broadcast_to(qv, d.shape), d)
    return d + w * uv + np.cross(np.broadcast_to(qv, d.shape), uv)


def camera_voxels(v):
    return np.asarray(se3.invert(v.pose)[4:], dtype=np.float64) / VS


def _round16(p):
    p = p.astype(np.float64)
    i = np.clip(np.copysign(np.floor(np.abs(p) + 0.5), p), -2 ** 31, 2 ** 31 - 1).astype(np.int64)   # roundf, saturated
    return ((i + 32768) & 0xFFFF) - 32768


def march(m, v, full_step_only=False):
    """Marches every pixel's ray.  Returns cross_i [H, W] (the sample index of the zero crossing, max_step where there is
    none), hit, and `absent`: the absent blocks that samples fell into ([n, 3]).  full_step_only: never change to the fine
    step, stop a ray at its first weighted voxel (the samples between the camera and the surface)."""
    look_up = Lookup(m)
    step = F(TRUNC) / F(2)
    max_step = int(math.ceil(F(v.max_depth) / step))
    full = (ray_directions(v).astype(F) * step / F(VS)).reshape(-1, 3)
    fine = full / F(10)
    n = len(full)
    p = np.broadcast_to((np.asarray(se3.invert(v.pose)[4:], dtype=F) / F(VS)), (n, 3)).copy()
    stepv = full.copy()
    prev, _, _ = look_up.fetch(_round16(p))
    p += stepv
    alive = np.ones(n, dtype=bool)
    cross = np.full(n, max_step, dtype=np.int64)
    absent = []
    for i in range(1, max_step):
        g = _round16(p)
        cur, w, present = look_up.fetch(g)
        absent.append((g[alive & ~present] >> 3))
        weighted = w >= 10
        crossing = alive & weighted & (prev > 0) & (cur <= 0) & (prev - cur <= 2)
        if full_step_only:
            crossing = alive & weighted
        cross[crossing] = i
        alive &= ~crossing
        prev = np.where(alive, cur, prev)
        stepv = np.where((weighted & (cur < F(0.5)) & (not full_step_only))[:, None], fine,
                         np.where(weighted[:, None], full, stepv))
        p = np.where(alive[:, None], p + stepv, p)
    absent = np.unique(np.concatenate(absent), axis=0) if absent else np.zeros((0, 3), np.int64)
    return dict(cross_i=cross.reshape(v.H, v.W), hit=(cross < max_step).reshape(v.H, v.W), absent=absent)


# ---------------------------------------------------------------------------------------------------------------------
# what the tests assert

# Closed-form shading: the ORACLE's own error on these views, (largest, mean), measured with shading_error().  It is
# byte quantisation plus central differences on a clipped field (and, on the sphere, the meeting point's error turning
# the normal).  The tests allow SHADING_MARGIN times these figures, for the oracle and for the engine alike.
SHADING_ORACLE = {"octants": (0.0073, 0.0024), "negative": (0.0073, 0.0024), "edge_hi": (0.0073, 0.0024),
                  "edge_lo": (0.0073, 0.0024), "rim": (0.0073, 0.0024), "collisions": (0.0073, 0.0024),
                  "sphere": (0.0761, 0.0116), "sphere_inside": (0.0378, 0.0113)}
SHADING_MARGIN = 1.7
SPHERE_MIN_COS = 0.35   # sphere views: rays that meet the surface at more than ~70 degrees from its normal are left out


def assert_shading(m, v, normal_img, rgba):
    worst, mean, n = shading_error(m, v, normal_img, rgba, SPHERE_MIN_COS if v.surface[0] == "sphere" else 0.0)
    print(f"raycast {v.name}: closed-form shading: largest error {worst:.4f}, mean {mean:.4f} over {n} pixels")
    assert n >= 0.2 * v.H * v.W, f"{v.name}: only {n} pixels judged"
    ref_worst, ref_mean = SHADING_ORACLE[v.name]
    assert worst <= SHADING_MARGIN * ref_worst, f"{v.name}: shading off by {worst} (oracle: {ref_worst})"
    assert mean <= SHADING_MARGIN * ref_mean, f"{v.name}: mean shading error {mean} (oracle: {ref_mean})"


def assert_hit_share(v, rgba):
    share = hit_share(rgba)
    assert v.hit_share[0] <= share <= v.hit_share[1], f"{v.name}: the oracle rendered {share} of the pixels"
    return share

def hit_share(rgba):
    return float((rgba[..., 3] == 255).mean())


def byte_differences(got, want):
    """(largest byte difference, number of differing bytes, share of differing bytes)"""
    d = np.abs(got.astype(np.int16) - want.astype(np.int16))
    return int(d.max()) if d.size else 0, int((d > 0).sum()), float((d > 0).mean()) if d.size else 0.0


def assert_matches_oracle(got, want, what, exact=False):
    """The bar of test_raycast_matches_oracle for both images (largest byte difference <= 1, fewer than 1e-3 of the
    bytes differing), pixels the oracle leaves empty exactly empty.  Prints the observed count.  exact: the images are
    equal (the crafted maps' probabilities are imported, not computed: both sides hold the same floats)."""
    counts = []
    for g, w, name in ((got[0], want[0], "rgba"), (got[1], want[1], "normal")):
        assert g.shape == w.shape
        worst, count, share = byte_differences(g, w)
        counts.append(count)
        print(f"raycast {what}: {name}: {count} of {g.size} bytes differ, largest difference {worst}")
        assert worst <= 1, f"{what}: {name}: max byte difference {worst}"
        assert share < 1e-3, f"{what}: {name}: {count} bytes differ"
        if exact:
            assert count == 0, f"{what}: {name}: {count} bytes differ"
    empty = want[0][..., 3] == 0
    assert not got[0][empty].any() and not got[1][empty].any(), f"{what}: a pixel the oracle leaves empty is not empty"
    return counts


def interior(m, v):
    """[H, W] bool: the ray meets the surface in front of the camera where every voxel within 2 of the meeting point
    lies in a block of the map (the crossing's eight trilinear corners and six normal neighbours exist), and the
    meeting point [H, W, 3]"""
    d, c = ray_directions(v), camera_voxels(v)
    if v.surface[0] == "plane":
        _, n, pt = v.surface
        with np.errstate(divide="ignore", invalid="ignore"):
            s = ((pt - c) @ n) / (d @ n)
    else:
        _, centre, r = v.surface
        b = d @ (c - centre)
        disc = b * b - ((c - centre) @ (c - centre) - r * r)
        s = np.where(disc > 0, -b - np.sqrt(np.maximum(disc, 0)), np.nan)
    ok = np.isfinite(s) & (s > 0)
    x = c + np.where(ok, s, 0)[..., None] * d
    look_up = Lookup(m)
    base = np.round(x).astype(np.int64)
    for off in _cube((-1, -1, -1), (2, 2, 2)) * 2:
        ok &= look_up.rows(base + off) >= 0
    return ok, x


def shading_error(m, v, normal_img, rgba, min_cos=0.0):
    """Closed-form shading on the view's interior pixels with alpha < 0.5: |diff - max(-d.n, 0)| with alpha and diff
    recovered from the normal image (n0 = alpha*255 + (1-alpha)*diff*255, n1 = (1-alpha)*diff*255).  Returns
    (largest error, mean error, pixels judged); every interior pixel must have been rendered.  min_cos: only pixels
    whose ray meets the surface at max(-d.n, 0) >= min_cos (a grazing ray's meeting point, and on a sphere with it the
    normal, moves far for a small error along the ray)."""
    ok, x = interior(m, v)
    assert (rgba[..., 3][ok] == 255).all(), f"{v.name}: {int((rgba[..., 3][ok] != 255).sum())} interior pixels are empty"
    d = ray_directions(v)
    if v.surface[0] == "plane":
        n = np.broadcast_to(v.surface[1], d.shape)
    else:
        n = x - v.surface[1]
        n = n / np.linalg.norm(n, axis=-1, keepdims=True)
    want = np.maximum(-(d * n).sum(-1), 0)
    n0, n1 = normal_img[..., 0].astype(np.float64), normal_img[..., 1].astype(np.float64)
    alpha = (n0 - n1) / 255
    use = ok & (alpha < 0.5) & (want >= min_cos)
    diff = n1[use] / ((1 - alpha[use]) * 255)
    err = np.abs(diff - want[use])
    return float(err.max()), float(err.mean()), int(use.sum())
