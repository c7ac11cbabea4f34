"""Crafted poses, intrinsics and image borders for the projection at the head of the frame update (integrate_block in
ra-slam_amd/csrc/kernels_integrate.h: voxel -> camera -> pixel, the two quotients, the pixel pick) and for the
visibility test that feeds it (block_visible<false> / voxel_visible in device_math.h).  Written once, checked without a
GPU in tests/test_proj_cases.py (every case reaches what it is named for, and the restatement here is pinned to the
oracle) and run against the HIP engine in tests/test_gpu_proj_cases.py and, at one and four voxels per lane, in
tests/diagnostic_build_cases.py.  Same role as update_cases.py and cand_cases.py: no engine, no GPU and no torch at
import.

A case is a set of imported blocks and two or three frames, each frame with its own pose and intrinsics.  Poses are
(qx, qy, qz, qw, tx, ty, tz), world -> camera as in the reference.  Images are 160 x 120 or 161 x 121:
  colour    of pixel (u, v) is (u & 255, v, a seeded hash of both): it names the pixel, adjacent pixels differ, and so do
            the two pixels of a pair mirrored about the principal point
  depth     a wall with seeded per-pixel noise, valid in every pixel (so that a wrong pick at a border finds a texel)
  ht / lt   ordinary and seeded
Most imported voxels have weight 0: one update then leaves exactly the picked pixel's colour in them, and a wrong pick
shows in the colour bytes.  The others have a weight of 1 .. 40, and every voxel a seeded tsdf and probability, so the
blend and the carve predicate run too.

The blocks of a case are the crafted ones, then "guard" blocks: every block that frame 0's candidate pass would
allocate (cand_cases.chain, the full-frustum test) is imported beforehand with ordinary words, so that frame 0
allocates nothing and the oracle's visible_blocks / updated_voxels can be counted against the restatement over the
imported blocks alone.  Later frames may allocate.

The numpy restatement (`project`, `corners`, `visible`, `predict`) is float32 operation by operation after the oracle's
integrate_block head and block_visible<false>, on cand_cases' qrot / se3_apply / roundf.  It is used ONLY to show that a
case reaches what it is named for; expected maps always come from the oracle.

Families:
  halves    voxel size 2^-6, K = (128, 128, 79.5, 59.5): every quotient on the plane 1 m ahead is 2 g + 79.5, an exact
            half; voxels exactly at -0.5 and W - 0.5, and inside (-0.5, 0) and [W - 1, W - 0.5).  The same camera-space
            lattice under the six float-exact rotations (identity, half turns about x, y, z, the third of a turn about
            (1, 1, 1) and its inverse), so that every cross-product term sees a non-zero operand
  borders   block corners exactly on u = 0, u = W - 1, v = 0, v = H - 1 as a block's only corner in view; the same
            blocks with the camera moved by 2^-18 m, the corner 2^-11 pixel outside; corners in the camera plane; a
            block that fills the image while all eight corners miss it
  plane     the camera plane cuts through imported blocks: voxels behind the camera update through the point-mirrored
            pixel; lane pairs with one voxel at pc.z == 0; the voxel at the camera centre (0 / 0, pixel 0)
  oblique   general poses and intrinsics (fx != fy, principal point near a corner and outside the image, 37 degree
            rotations about each axis, a quarter roll, a quaternion of norm 1.001), the ends of the block grid
  far       t.z = 1e19 and both sides of 1e18: the divisor on either side of the shared-reciprocal guard
"""
import functools
from typing import NamedTuple

import numpy as np

import cand_cases as cc
from cand_cases import F, f2i, intr_mul, roundf, se3, se3_apply, to_short
from ratsdf._abi import RGBW_DTYPE
from update_cases import align, bits, by_position, words  # (what the comparisons of a case module need beside `predict`)

U32 = np.uint32
CFG = dict(block_bits=12, bucket_bits=12)
MD = 4.0
VI = np.arange(512)
IDENTITY = (0.0, 0.0, 0.0, 1.0)


class Frame(NamedTuple):
    rgb: np.ndarray
    depth: np.ndarray
    ht: np.ndarray
    lt: np.ndarray
    md: float
    intr: tuple
    pose: tuple
    vs: float
    trunc: float

    def args(self):
        return (self.rgb, self.depth, self.ht, self.lt, self.md, self.intr, self.pose)

    @property
    def shape(self):
        return self.depth.shape


class Case(NamedTuple):
    name: str
    family: str
    vs: float
    trunc: float
    blocks: tuple      # (positions [n, 3], tsdf, rgbw, prob): the crafted blocks first, then the guard blocks
    frames: tuple
    n_crafted: int

    @property
    def pool(self):    # (the name tests/test_gpu_update_cases.py prints)
        return self.name


# ---------------------------------------------------------------------------------------------------------------------
# the restatement (the oracle's voxel_visible / block_visible<false> and the head of its integrate_block)
def _project(g, fr):
    """voxel coordinates g (three int arrays) -> (pc, ph, qu, qv) in float32, in the oracle's order"""
    pw = tuple(c.astype(F) * F(fr.vs) for c in g)
    pc = se3_apply(se3(fr.pose), pw)
    ph = intr_mul(fr.intr, pc)
    with np.errstate(all="ignore"):
        return pc, ph, ph[0] / ph[2], ph[1] / ph[2]


class Corners(NamedTuple):
    u: np.ndarray      # [n, 8] float32 quotients of the eight corners
    v: np.ndarray
    z: np.ndarray      # [n, 8] ph.z
    inview: np.ndarray  # [n, 8] voxel_visible


def corners(pos, fr):
    pos = np.asarray(pos).astype(np.int64).reshape(-1, 3)
    H, W = fr.shape
    base = to_short(pos << 3)
    i = np.arange(8)
    g = [to_short(base[:, a, None] + (((i >> a) & 1) * 7)[None, :]) for a in range(3)]
    _, ph, u, v = _project(g, fr)
    with np.errstate(invalid="ignore"):
        inview = (u >= 0) & (u <= F(W - 1)) & (v >= 0) & (v <= F(H - 1)) & (ph[2] >= 0)
    return Corners(u, v, np.broadcast_to(ph[2], u.shape), inview)


def visible(pos, fr):
    """block_visible<false>: any of the eight corners in view"""
    return corners(pos, fr).inview.any(axis=1)


class Projection(NamedTuple):
    pcz: np.ndarray    # [n, 512] float32
    qu: np.ndarray     # the two quotients
    qv: np.ndarray
    iu: np.ndarray     # [n, 512] int64: f2i(roundf(q))
    iv: np.ndarray
    inb: np.ndarray    # the pick lies in the image
    k: np.ndarray      # the picked pixel (0 where it does not)


def project(pos, fr):
    pos = np.asarray(pos).astype(np.int64).reshape(-1, 3)
    H, W = fr.shape
    base = to_short(pos << 3)
    g = [to_short(base[:, a, None] + ((VI >> s) & 7)[None, :]) for a, s in ((0, 0), (1, 3), (2, 6))]
    pc, _, qu, qv = _project(g, fr)
    iu, iv = f2i(roundf(qu)), f2i(roundf(qv))
    inb = (iu >= 0) & (iu < W) & (iv >= 0) & (iv < H)
    return Projection(np.broadcast_to(pc[2], qu.shape), qu, qv, iu, iv, inb, np.where(inb, iv * W + iu, 0))


def range_image(fr):
    """img_depth_to_range: |K^-1 (x, y, 1)|, float32 in the oracle's order"""
    H, W = fr.shape
    Ki = cc.intr_inverse(fr.intr)
    y, x = np.meshgrid(np.arange(H, dtype=F), np.arange(W, dtype=F), indexing="ij")
    one = np.ones((H, W), dtype=F)
    px, py, pz = Ki[0] * x + Ki[2] * one, Ki[1] * y + Ki[3] * one, one
    return np.sqrt(px * px + (py * py + pz * pz)).astype(F)


class Prediction(NamedTuple):
    upd: np.ndarray    # [n, 512] bool: the frame updates the voxel
    k: np.ndarray      # [n, 512] the picked pixel
    ts: np.ndarray     # [n, 512] float32 truncated signed distance of the update (where upd)
    wn: np.ndarray     # [n, 512] float32 w_new (where upd)
    proj: Projection
    vis: np.ndarray    # [n] bool: block_visible<false>


def predict(pos, fr):
    """which voxels of the blocks at `pos` the frame updates, and with which pixel, ts and w_new"""
    pr, vis = project(pos, fr), visible(pos, fr)
    with np.errstate(all="ignore"):
        d = fr.depth.reshape(-1)[pr.k]
        ok = vis[:, None] & pr.inb & ~((d == 0) | (d > F(fr.md)))
        sdf = (range_image(fr).reshape(-1)[pr.k] * (d - pr.pcz)).astype(F)
        upd = ok & (sdf > -F(fr.trunc))
        ts = np.minimum(F(1), sdf / F(fr.trunc)).astype(F)
        wn = ((F(1) - d / F(fr.md)) * F(4)).astype(F)
    return Prediction(upd, pr.k, ts, wn, pr, vis)


def partner(a):
    """a[n, 512] seen from each voxel's lane partner (the x-neighbour of the pair 2k, 2k + 1)"""
    return a[:, VI ^ 1]


# ---------------------------------------------------------------------------------------------------------------------
# images
def pixel_colours(W, H, seed):
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    h = (u * 73856093 + v * 19349669 + seed * 83492791) & 0xFFFFFFFF
    h = ((h ^ (h >> 13)) * 1274126177) & 0xFFFFFFFF
    return np.stack([u & 255, v & 255, (h >> 16) & 255], axis=-1).astype(np.uint8)


def make_frame(seed, W, H, intr, pose, vs, trunc, depth_m, noise=0.01):
    """a wall at depth_m metres (a number or an [H, W] array) with `noise` metres of seeded noise in every pixel"""
    rng = np.random.default_rng(seed)
    depth = (np.broadcast_to(np.asarray(depth_m, dtype=np.float64), (H, W)) + rng.uniform(-noise, noise, (H, W))).astype(F)
    ht = rng.uniform(0.05, 0.95, (H, W)).astype(F)
    lt = (F(1) - ht).astype(F)
    out = (pixel_colours(W, H, seed), depth, ht, lt)
    for a in out:
        a.setflags(write=False)
    return Frame(*out, MD, tuple(float(x) for x in intr), tuple(float(x) for x in pose), float(vs), float(trunc))


# ---------------------------------------------------------------------------------------------------------------------
# blocks
def keys(pos):
    return cc.block_key(np.asarray(pos).reshape(-1, 3))


def unique_blocks(pos):
    pos = np.asarray(pos, dtype=np.int64).reshape(-1, 3)
    _, first = np.unique(keys(pos), return_index=True)
    return pos[np.sort(first)]


def guard_blocks(pos, fr):
    """the blocks frame `fr` would allocate beside the blocks `pos`: distinct blocks of its ray samples that are
    absent and pass the full-frustum test (whether a directory bucket's lock would let them in or not)"""
    H, W = fr.shape
    ch = cc.chain(fr.depth, fr.md, fr.intr, fr.pose, fr.vs, fr.trunc)
    cand = unique_blocks(ch.block)
    cand = cand[~np.isin(keys(cand), keys(pos))]
    if not len(cand):
        return cand
    return cand[cc.fully_visible(cand, H, W, fr.intr, fr.pose, fr.vs)]


def ordinary_words(rng, n, zero_share=0.7):
    """seeded tsdf in [-1, 1], colours, probabilities in (0.02, 0.98); weight 0 in `zero_share` of the voxels, 1 .. 40 in
    the others"""
    t = rng.uniform(-1, 1, (n, 512)).astype(F)
    p = rng.uniform(0.02, 0.98, (n, 512)).astype(F)
    c = np.zeros((n, 512), dtype=RGBW_DTYPE)
    for ch in ("r", "g", "b"):
        c[ch] = rng.integers(0, 256, (n, 512))
    c["weight"] = np.where(rng.uniform(0, 1, (n, 512)) < zero_share, 0, rng.integers(1, 41, (n, 512)))
    return t, c, p


def make_case(name, family, vs, trunc, crafted, frames, words=None):
    """crafted: block positions [n, 3]; words: (tsdf, rgbw, prob) overrides for the first len(words[0]) blocks"""
    crafted = unique_blocks(crafted)
    guard = guard_blocks(crafted, frames[0])
    pos = np.concatenate([crafted, guard]).astype(np.int16)
    rng = np.random.default_rng(sum(map(ord, name)))
    t, c, p = ordinary_words(rng, len(pos))
    if words is not None:
        m = len(words[0])
        t[:m], c[:m], p[:m] = words
    blocks = (pos, t, c, p)
    for a in blocks:
        a.setflags(write=False)
    return Case(name, family, float(vs), float(trunc), blocks, tuple(frames), len(crafted))


def rotation_matrix(q):
    """the integer matrix of a float-exact rotation (columns: the images of the axes under cand_cases.qrot)"""
    qf = tuple(F(x) for x in q)
    cols = [cc.qrot(qf, tuple(F(v) for v in e)) for e in ((1, 0, 0), (0, 1, 0), (0, 0, 1))]
    R = np.array(cols, dtype=np.float64).T
    assert np.array_equal(R, np.round(R)) and abs(np.linalg.det(R) - 1) < 1e-9
    return R.astype(np.int64)


def block_voxels(pos):
    """[n * 512, 3] voxel coordinates of blocks"""
    pos = np.asarray(pos, dtype=np.int64).reshape(-1, 3)
    off = np.stack([VI & 7, (VI >> 3) & 7, VI >> 6], axis=1)
    return (pos[:, None, :] * 8 + off[None, :, :]).reshape(-1, 3)


def blocks_in_view(fr, zlo, zhi, margin=6.0, step=0.4):
    """blocks with a voxel near a point that projects within `margin` pixels of the image at a camera depth in
    [zlo, zhi] (float64; only chooses the scene)"""
    H, W = fr.shape
    fx, fy, cx, cy = fr.intr
    q, t = np.array(fr.pose[:4], dtype=np.float64), np.array(fr.pose[4:], dtype=np.float64)
    Rm = np.array([cc.qrot(tuple(q), e) for e in ((1, 0, 0), (0, 1, 0), (0, 0, 1))], dtype=np.float64).T
    z = np.arange(zlo, zhi + 1e-9, step * fr.vs)
    du = max(1.0, step * fr.vs * fx / zhi)
    dv = max(1.0, step * fr.vs * fy / zhi)
    u = np.arange(-margin, W - 1 + margin + du, du)
    v = np.arange(-margin, H - 1 + margin + dv, dv)
    uu, vv, zz = np.meshgrid(u, v, z, indexing="ij")
    pc = np.stack([(uu - cx) / fx * zz, (vv - cy) / fy * zz, zz], axis=-1).reshape(-1, 3)
    pw = np.linalg.solve(Rm, (pc - t).T).T
    return unique_blocks(np.round(pw / fr.vs).astype(np.int64) >> 3)


# ---------------------------------------------------------------------------------------------------------------------
# what a case reaches
def exact_halves(q):
    """quotients that are exactly n + 0.5"""
    with np.errstate(invalid="ignore"):
        return np.isfinite(q) & (np.abs(q - np.trunc(q)) == F(0.5))


def border_classes(pr, W, H):
    """voxels per border class of the halves family"""
    with np.errstate(invalid="ignore"):
        return {"u == -0.5": int((pr.qu == F(-0.5)).sum()), "u == W - 0.5": int((pr.qu == F(W - 0.5)).sum()),
                "u in (-0.5, 0)": int(((pr.qu > F(-0.5)) & (pr.qu < 0)).sum()),
                "u in [W - 1, W - 0.5)": int(((pr.qu >= F(W - 1)) & (pr.qu < F(W - 0.5))).sum()),
                "v == -0.5": int((pr.qv == F(-0.5)).sum()), "v == H - 0.5": int((pr.qv == F(H - 0.5)).sum())}


def near_borders(pr, W, H):
    """voxels whose other quotient picks a pixel and whose quotient lies in (-0.5, 0) or [W - 1, W - 0.5) on some axis:
    inside the image only by rounding"""
    with np.errstate(invalid="ignore"):
        bu = ((pr.qu > F(-0.5)) & (pr.qu < 0)) | ((pr.qu >= F(W - 1)) & (pr.qu < F(W - 0.5)))
        bv = ((pr.qv > F(-0.5)) & (pr.qv < 0)) | ((pr.qv >= F(H - 1)) & (pr.qv < F(H - 0.5)))
    return int(((bu | bv) & pr.inb).sum())


def mixed_pairs(pr):
    """lane pairs (voxel ^ 1) with exactly one member at pc.z == 0"""
    z0 = pr.pcz == 0
    return int((z0 != partner(z0)).sum()) // 2


def mirrored_pixel(pr, fr):
    """[n, 512] the pixel a voxel's pick is the point mirror of: (2 cx - qu, 2 cy - qv) rounded; -1 outside the image"""
    H, W = fr.shape
    with np.errstate(all="ignore"):
        mu = f2i(roundf(F(2) * F(fr.intr[2]) - pr.qu))
        mv = f2i(roundf(F(2) * F(fr.intr[3]) - pr.qv))
    inb = (mu >= 0) & (mu < W) & (mv >= 0) & (mv < H)
    return np.where(inb, mv * W + mu, -1)


# ---------------------------------------------------------------------------------------------------------------------
# halves
VS6 = 2.0 ** -6
HALVES_K = (128.0, 128.0, 79.5, 59.5)
HALVES_ROT = {"identity": IDENTITY, "turn-x": (1.0, 0.0, 0.0, 0.0), "turn-y": (0.0, 1.0, 0.0, 0.0),
              "turn-z": (0.0, 0.0, 1.0, 0.0), "third": (0.5, 0.5, 0.5, 0.5), "third-back": (-0.5, -0.5, -0.5, 0.5)}
HALVES_CAMERA_BLOCKS = np.array([(x, y, 8) for y in range(-4, 4) for x in range(-6, 6)], dtype=np.int64)


def lattice_shift(q):
    """the translation, in voxels, that goes with a float-exact rotation: -1 along every camera axis the rotation
    reverses, so that whole camera-space blocks (voxels 8 b .. 8 b + 7) come from whole world blocks"""
    return (rotation_matrix(q).sum(axis=1) < 0) * -1


def rotated_blocks(camera_blocks, q):
    """the world blocks whose voxels the rotation q and lattice_shift(q) take onto the voxels of `camera_blocks`"""
    R = rotation_matrix(q)
    return unique_blocks(((block_voxels(camera_blocks) - lattice_shift(q)[None, :]) @ R) >> 3)   # rows: R^-1 (c - t)


def lattice_pose(q, vs, extra=(0.0, 0.0, 0.0)):
    return tuple(q) + tuple(float(s) * vs + e for s, e in zip(lattice_shift(q), extra))


@functools.lru_cache(maxsize=None)
def halves(rot):
    q = HALVES_ROT[rot]
    pos = rotated_blocks(HALVES_CAMERA_BLOCKS, q)
    assert len(pos) == len(HALVES_CAMERA_BLOCKS)
    seed = 8100 + 10 * list(HALVES_ROT).index(rot)
    mk = lambda i, d: make_frame(seed + i, 160, 120, HALVES_K, lattice_pose(q, VS6), VS6, 6 * VS6, d)
    # a wall behind the slab (every voxel in the image updates, ts on both sides of 1), then one inside it
    return make_case(f"halves/{rot}", "halves", VS6, 6 * VS6, pos, (mk(0, 1.13), mk(1, 1.06)))


# ---------------------------------------------------------------------------------------------------------------------
# borders
# side: (rotation, intrinsics, W, H, the two blocks whose one corner in view lies on the bound, the camera's move)
NUDGE = 2.0 ** -18   # metres; at 1 m and f = 128 it moves a corner by 2^-11 pixel
BORDER_SIDES = {
    "u0": ((0.0, 1.0, 0.0, 0.0), (128.0, 128.0, 80.0, 60.0), 161, 121, ((5, 3, -8), (5, -4, -8)), (-NUDGE, 0.0, 0.0)),
    "uW": ((1.0, 0.0, 0.0, 0.0), (128.0, 128.0, 80.0, 60.0), 161, 121, ((5, 3, -8), (5, -4, -8)), (NUDGE, 0.0, 0.0)),
    "v0": ((1.0, 0.0, 0.0, 0.0), (128.0, 128.0, 90.0, 64.0), 160, 120, ((4, 4, -8), (-6, 4, -8)), (0.0, -NUDGE, 0.0)),
    "vH": ((0.0, 1.0, 0.0, 0.0), (128.0, 128.0, 90.0, 56.0), 161, 121, ((-5, 4, -8), (5, 4, -8)), (0.0, NUDGE, 0.0)),
}
BORDER_BOUND = {"u0": ("u", 0.0), "uW": ("u", 160.0), "v0": ("v", 0.0), "vH": ("v", 120.0)}


def _border_scene(q):
    """a few blocks in the middle of the view, 1 m ahead under the half turn q"""
    return rotated_blocks([(x, y, 7) for y in (-1, 0) for x in (-1, 0)], q)


@functools.lru_cache(maxsize=None)
def borders(side, moved):
    """moved False: the corner on the bound; True: the camera 2^-18 m aside, the corner 2^-11 pixel outside"""
    q, K, W, H, edge, nudge = BORDER_SIDES[side]
    pos = np.concatenate([np.array(edge, dtype=np.int64), _border_scene(q)])
    t0, t1 = ((0.0, 0.0, 0.0), nudge)[::-1 if moved else 1]
    seed = 8300 + 10 * list(BORDER_SIDES).index(side) + 5 * moved
    mk = lambda i, t: make_frame(seed + i, W, H, K, q + t, VS6, 6 * VS6, 1.12)
    return make_case(f"borders/{side}/{'moved' if moved else 'on'}", "borders", VS6, 6 * VS6, pos, (mk(0, t0), mk(1, t1)))


@functools.lru_cache(maxsize=None)
def borders_camera_plane():
    """blocks whose far face lies in the camera plane (pc.z == 0: quotients of +-inf, and 0 / 0 at the corner on the
    axis), every other corner behind the camera; beside them blocks in the middle of the view"""
    K = (128.0, 128.0, 80.0, 60.0)
    pos = np.array([(0, 0, -1), (-1, 0, -1), (0, -1, -1), (2, 1, -1)] + [(x, y, 7) for y in (-1, 0) for x in (-1, 0)])
    # (gz = -1 is the far face of bz = -1: t.z = vs puts it at pc.z = 0; the corner (0, 0, -1) lies on the axis)
    mk = lambda i, t: make_frame(8400 + i, 160, 120, K, IDENTITY + t, VS6, 6 * VS6, 1.12)
    return make_case("borders/camera-plane", "borders", VS6, 6 * VS6, pos,
                     (mk(0, (0.0, 0.0, VS6)), mk(1, (VS6, 0.0, VS6)), mk(2, (0.0, 0.0, 0.0))))


FILL_BLOCK = (0, 0, 0)


@functools.lru_cache(maxsize=None)
def borders_fill():
    """a block that fills the image: the camera stands one voxel before the middle of its near face (f = 138), so its
    near corners project far outside and its far ones, eight voxels ahead, 0.4 and 1.4 pixel outside the rows of the image,
    while well over a hundred of its voxels project inside.  Not visible, so nothing in it changes; the blocks
    behind it are visible"""
    K = (138.0, 138.0, 80.0, 60.0)
    pos = np.array([FILL_BLOCK, (0, 0, 1), (0, 0, 2)])
    t = (-3.5 * VS6, -3.5 * VS6, VS6)
    mk = lambda i, d: make_frame(8450 + i, 160, 120, K, IDENTITY + t, VS6, 6 * VS6, d)
    return make_case("borders/fill", "borders", VS6, 6 * VS6, pos, (mk(0, 10 * VS6), mk(1, 20 * VS6)))


# ---------------------------------------------------------------------------------------------------------------------
# plane
PLANE_K = (40.0, 40.0, 80.0, 60.0)   # 127 degrees across: corners 3 voxels ahead of the camera are in view
VS2 = 0.02


def _t(x):
    return float(F(x))


@functools.lru_cache(maxsize=None)
def plane(sub):
    if sub == "a":
        # identity rotation; the camera half a voxel off the corner shared by four blocks, in the middle of layer bz
        vs, bz = VS2, 3
        q, t = IDENTITY, (_t(0.5 * vs), _t(0.5 * vs), -_t(F(8 * bz + 4) * F(vs)))
        pos = [(x, y, z) for z in (bz - 1, bz, bz + 1) for y in range(-2, 2) for x in range(-2, 2)]
    elif sub == "b":
        # the camera's z is the world's x: the camera plane is x = 8 bx + 4, and lane pairs straddle it.  The camera
        # stands ON the voxel (8 bx + 4, 0, 0): 0 / 0 there.  Voxel size 2^-6: the rotation is exact
        vs, bx = VS6, 3
        q = next(r for r in (HALVES_ROT["third"], HALVES_ROT["third-back"])
                 if np.array_equal(rotation_matrix(r) @ np.array([1, 0, 0]), [0, 0, 1]))
        # Frame 0 has the plane at the ODD x = 8 bx + 5 (the pair's second voxel is the one at pc.z == 0, its first
        # lies a voxel behind the camera), frame 1 at the even x = 8 bx + 4 (the first at 0, the second a voxel ahead)
        t = (0.0, 0.0, -_t(F(8 * bx + 5) * F(vs)))
        t1 = (0.0, 0.0, -_t(F(8 * bx + 4) * F(vs)))
        pos = [(x, y, z) for x in (bx - 1, bx, bx + 1) for y in range(-2, 2) for z in range(-2, 2)]
    else:
        # ten degrees of tilt about an oblique axis and a translation that is no dyadic number
        vs, bz = VS2, 3
        q, t = cc.quat((1.0, 0.3, 0.0), 10.0), (0.013, -0.027, -((8 * bz + 4) * vs) + 0.003)
        pos = [(x, y, z) for z in (bz - 1, bz, bz + 1) for y in range(-2, 2) for x in range(-2, 2)]
    seed = 8500 + 10 * "abc".index(sub)
    mk = lambda i, d, t: make_frame(seed + i, 160, 120, PLANE_K, tuple(q) + tuple(t), vs, 6 * vs, d, noise=0.1 * vs)
    # walls 10 and 6 voxels ahead: in front of them and just behind, the voxels of the layer before the camera
    return make_case(f"plane/{sub}", "plane", vs, 6 * vs, np.array(pos),
                     (mk(0, 10 * vs, t), mk(1, 6 * vs, t1 if sub == "b" else t)))


# ---------------------------------------------------------------------------------------------------------------------
# oblique
def _scaled(q, s):
    return tuple(float(F(c) * F(s)) for c in q)


OBLIQUE = {  # name: (intrinsics, rotation, translation)
    "corner-x37": ((140.3, 97.7, 3.3, 4.7), cc.quat((1, 0, 0), 37.0), (0.11, -0.07, 0.05)),
    "outside-y37": ((140.3, 97.7, -20.5, 60.2), cc.quat((0, 1, 0), 37.0), (-0.21, 0.04, 0.02)),
    "z37": ((140.3, 97.7, 79.3, 59.1), cc.quat((0, 0, 1), 37.0), (0.03, 0.05, -0.04)),
    "roll90": ((97.7, 140.3, 80.6, 60.4), cc.quat((0, 0, 1), 90.0), (0.01, -0.02, 0.03)),
    "norm1.001": ((140.3, 97.7, 81.7, 58.2), _scaled(cc.quat((1, 1, 0), 20.0), 1.001), (-0.05, 0.02, 0.06)),
    # the ends of the block grid: bx = 4095 is 32 760 .. 32 767 voxels out, bx = -4096 -32 768 .. -32 761.  (The third
    # entry is the camera's centre in the world here: `oblique` turns it into the translation)
    "grid-end+": ((140.3, 97.7, 79.3, 59.1), cc.quat((0, 1, 0), 4.0), ((4095 * 8 - 4) * VS2, 0.01, -0.5)),
    "grid-end-": ((140.3, 97.7, 79.3, 59.1), cc.quat((0, 1, 0), -4.0), ((-4096 * 8 + 12) * VS2, -0.01, -0.5)),
}
OBLIQUE_Z = (0.42, 0.6)   # camera depths of the scene


@functools.lru_cache(maxsize=None)
def oblique(name):
    K, q, t = OBLIQUE[name]
    grid_end = name.startswith("grid-end")
    if grid_end:   # t = -R c
        t = tuple(-float(x) for x in cc.qrot(tuple(np.float64(c) for c in q), tuple(np.float64(c) for c in t)))
    seed = 8700 + 10 * list(OBLIQUE).index(name)
    mk = lambda i, d, dt=0.0: make_frame(seed + i, 160, 120, K, tuple(q) + (t[0] + dt, t[1], t[2]), VS2, 6 * VS2, d)
    frames = (mk(0, 0.62), mk(1, 0.5, 0.004))
    pos = blocks_in_view(frames[0], *OBLIQUE_Z)
    if grid_end:   # (what lies past the end of the grid is no block)
        pos = pos[(pos[:, 0] <= 4095) & (pos[:, 0] >= -4096)]
    return make_case(f"oblique/{name}", "oblique", VS2, 6 * VS2, pos, frames)


# ---------------------------------------------------------------------------------------------------------------------
# far
F1E18 = F(1e18)
FAR_TZ = {"1e19": 1e19, "below": float(np.nextafter(F1E18, F(0))), "above": float(F1E18)}
FAR_ORDER = {"1e19": ("1e19", "below", "above"), "below": ("below", "above"), "above": ("above", "below")}
FAR_CARVE = ("full 0.95", "0.95 with one 0.5", "full -0.9f", "-1 with one -0.89")   # carved, kept, carved, kept


@functools.lru_cache(maxsize=None)
def far(which):
    """recip_safe is |z| < 1e18f: 1e19 and 1e18f itself take the IEEE quotients, the float below 1e18f the shared
    reciprocal.  Nothing updates (sdf = range * (d - 1e18) < -trunc), every block is visible (every corner projects on
    the principal point), and four blocks stand for the carve verdict, which falls on the priors alone"""
    K = (140.0, 140.0, 80.0, 60.0)
    pos = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0)] + [(x, y, z) for z in (5, 6) for y in (-2, -1, 0, 1)
                                                                  for x in (-2, -1, 0, 1)])
    rng = np.random.default_rng(8900)
    t, c, p = ordinary_words(rng, 4)
    c["weight"] = 5
    t[0], t[1], t[2], t[3] = 0.95, 0.95, -F(0.9), -1.0
    t[1, 77], t[3, 300] = 0.5, -0.89
    mk = lambda i, w: make_frame(8900 + i, 160, 120, K, IDENTITY + (0.0, 0.0, FAR_TZ[w]), VS2, 6 * VS2, 1.0)
    return make_case(f"far/{which}", "far", VS2, 6 * VS2, pos, tuple(mk(i, w) for i, w in enumerate(FAR_ORDER[which])),
                     words=(t, c, p))


# ---------------------------------------------------------------------------------------------------------------------
# one map under three different cameras (for batches: an engine has one voxel size, here 2^-6)
@functools.lru_cache(maxsize=None)
def batch_case():
    """the blocks of halves/third and plane/b and a scene for an oblique camera, all at 2^-6 m; the frames: halves/third
    frame 0, plane/b frame 0 and the camera of oblique/corner-x37 -- three poses and three sets of intrinsics"""
    h, p = halves("third"), plane("b")
    K, q, t = OBLIQUE["corner-x37"]
    third = make_frame(8990, 160, 120, K, tuple(q) + tuple(t), VS6, 6 * VS6, 0.6)
    pos = np.concatenate([h.blocks[0][:h.n_crafted], p.blocks[0][:p.n_crafted], blocks_in_view(third, 0.45, 0.55)])
    return make_case("batch", "batch", VS6, 6 * VS6, pos, (h.frames[0], p.frames[0], third))


# ---------------------------------------------------------------------------------------------------------------------
FAMILIES = {
    "halves": tuple((halves, (r,)) for r in HALVES_ROT),
    "borders": tuple((borders, (s, m)) for s in BORDER_SIDES for m in (False, True))
               + ((borders_camera_plane, ()), (borders_fill, ())),
    "plane": tuple((plane, (s,)) for s in "abc"),
    "oblique": tuple((oblique, (n,)) for n in OBLIQUE),
    "far": tuple((far, (w,)) for w in FAR_TZ),
}
ALL = tuple((fam, fn, a) for fam, members in FAMILIES.items() for fn, a in members)
IDS = tuple("-".join([fn.__name__] + [str(x) for x in a]) for _, fn, a in ALL)


def family(name):
    return [fn(*a) for fn, a in FAMILIES[name]]
