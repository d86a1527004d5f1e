"""Inputs shared by test_frames_carve_host.py and test_gpu_frames_carve.py: tests/frames_cases.py's synthetic frames and
points, the scene rendered again without its box, and a handful of probes constructed so that every float32 value of the
rule is exact.  Every case is built once per process and must not be modified."""
import functools

import numpy as np
import torch

from geoformer_amd import frames, render, scene
from tests import frames_cases as fc

# Sizes, each next to the constant it straddles (csrc/frames_carve.hip):
WAVE = 64                    # the lanes of a wave: n = 63, 64, 65
THREADS = 256                # FC_THREADS = frames.CARVE_THREADS: the points of one workgroup; n = 257 is one workgroup + 1
STAGE = 16                   # FC_STAGE = frames.CARVE_STAGE: the frame records a workgroup stages at a time; F = 16 is one
#                              full round, F = 17 a second round of one record
SIZES = (0, 1, WAVE - 1, WAVE, WAVE + 1, THREADS + 1)
FIRST_ROWS = 1024            # the first capacity of a Carver's state: dense(4)'s first frame alone brings more cells
RANDOM = fc.CELL_POINTS      # 20000 random points = 78 workgroups + 32 points: most outside or occluded, lanes diverge
CELL = 0.02                  # metres: the cells of the maps below
EDGE = 0.05
BAND = 3.0 * float(np.float32(CELL))   # a Carver's default band: three cells, as the constructor computes it

assert THREADS == frames.CARVE_THREADS and STAGE == frames.CARVE_STAGE and FIRST_ROWS == frames._CARVE_MIN_ROWS

OUTSIDE, UNKNOWN, OCCLUDED, SEEN, FREE = 0, 1, 2, 3, 4
assert (OUTSIDE, UNKNOWN, OCCLUDED, SEEN, FREE) == (frames.OUTSIDE, frames.UNKNOWN, frames.OCCLUDED, frames.SEEN, frames.FREE)


def f32(v):
    return np.float32(v)


@functools.lru_cache(maxsize=None)
def narrow_points():
    """float32 [n + 200, 3]: the fused points of narrow() at 2 cm and 200 random points in the scene's bounding box."""
    fused = frames.fuse_host(fc.make(fc.narrow()), cell=CELL)
    xyz, _ = fc.small_scene()
    lo, hi = xyz.min(0), xyz.max(0)
    rnd = (lo + np.random.default_rng(11).random((200, 3)) * (hi - lo)).astype(np.float32)
    out = np.concatenate([fused.xyz.numpy(), rnd])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def scene_random_points(n=RANDOM):
    """frames_cases.random_points(n) moved to the scene's lower corner: in and around the cameras' frusta."""
    xyz, _ = fc.small_scene()
    out = (fc.random_points(n)[0] + xyz.min(0) - np.float32(0.2)).astype(np.float32)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def many_frames(F):
    """F frames of NARROW around the scene as uint16 Frames: F = STAGE and STAGE + 1."""
    return fc.make(fc.rendered(F, fc.NARROW, 40.0, 2))


def sheared(fr):
    """fr with every pose's 3 x 3 block multiplied by a shear and a scale: not orthonormal, still invertible."""
    F = fr.depth.shape[0]
    pose = np.zeros((F, 4, 4))
    pose[:, :3, :] = fr.table[:, 4:].astype(np.float64).reshape(F, 3, 4)
    pose[:, 3, 3] = 1
    S = np.array([[1.25, 0.5, 0.0], [0.0, 0.75, 0.25], [0.0, 0.0, 1.5]])
    pose[:, :3, :3] = pose[:, :3, :3] @ S
    return frames.make(fr.depth, fr.table[0, :4].astype(np.float64), pose, fr.color, fr.depth_shift)


@functools.lru_cache(maxsize=None)
def no_box(n=fc.DENSE_FRAMES_TOP):
    """(depth_m float32 [n, H, W]) of dense(n)'s cameras on the scene without its box, the background at FAR_FILL."""
    xyz, rgb = fc.small_scene()
    box = scene.make_small_scene(8192, 7)["instance"] == 0
    case = fc.dense(n)
    W, H = fc.DENSE
    keys = render.splat_host(np.ascontiguousarray(xyz[~box]), None, render.camera_table(case.cams, 1, 2), W, H, 2)
    _, index = render.resolve_host(keys, 1, np.ascontiguousarray(rgb[~box]), shade=render.NO_SHADE, background=(0, 0, 0))
    depth = np.where(index >= 0, render.depth_of_keys(keys), np.float32(fc.FAR_FILL)).astype(np.float32)
    depth.setflags(write=False)
    return depth


@functools.lru_cache(maxsize=None)
def box_gone():
    """(with_box Frames, without_box Frames, is_box bool [H W n]): dense(4) as float32 frames with every background pixel
    at FAR_FILL, the same cameras on the scene without the box, and per pixel of the first whether its source point
    (the case's index) is a box point."""
    case = fc.dense(fc.DENSE_FRAMES_TOP)
    d = np.array(case.depth_m)
    d[case.index < 0] = fc.FAR_FILL
    box = scene.make_small_scene(8192, 7)["instance"] == 0
    is_box = (case.index >= 0) & box[np.maximum(case.index, 0)]
    return fc.make(case, "f32", True, depth=d), fc.make(case, "f32", True, depth=no_box()), is_box


def box_cells(cells, is_box, M):
    """bool [M]: the cells most of whose pixels came from box points (cells: what add returned)."""
    c = cells.numpy().reshape(-1)
    on = c >= 0
    total = np.bincount(c[on], minlength=M)
    of_box = np.bincount(c[on], weights=is_box.reshape(-1)[on].astype(np.float64), minlength=M)
    return 2 * of_box > total


# ---- probes whose every float32 value is exact --------------------------------------------------------------------------
# One frame of 8 x 4 pixels, the camera at the origin looking along +z with the identity pose, fx = fy = 4, cx = 4,
# cy = 2, every depth 2.0 m (float32, depth_shift 1); near = 0.5, rel = 0, band = 0.25: tol = 0.25 exactly, u = 4 x / z + 4.
B_NEAR, B_FAR, B_BAND, B_REL = 0.5, 10.0, 0.25, 0.0
B_W, B_H = 8, 4


def boundary_frames():
    depth = np.full((1, B_H, B_W), 2.0, np.float32)
    return frames.make(depth, [4.0, 4.0, 4.0, 2.0], np.eye(4)[None], None, 1.0)


def _below(v):
    return np.nextafter(f32(v), f32(-np.inf))


def _above(v):
    return np.nextafter(f32(v), f32(np.inf))


BOUNDARY = (  # (point, the class the rule gives, why)
    ((0, 0, 0.5), FREE, "zc == near is inside the range; 0.5 < 2 - 0.25"),
    ((0, 0, _below(0.5)), OUTSIDE, "zc just below near"),
    ((1, 0, 1), OUTSIDE, "u = 4 / 1 + 4 == W exactly"),
    ((f32(1) - f32(2.0 ** -21), 0, 1), FREE, "u = 8 - 2^-19, just below W: pixel 7"),
    ((-1, 0, 1), FREE, "u == 0 exactly: pixel 0"),
    ((_below(-1), 0, 1), OUTSIDE, "u just below 0"),
    ((0, 0.5, 1), OUTSIDE, "v = 4 * 0.5 + 2 == H exactly"),
    ((0, 0, 1.75), SEEN, "zc == z - tol"),
    ((0, 0, _below(1.75)), FREE, "zc just below z - tol"),
    ((0, 0, 2.25), SEEN, "zc == z + tol"),
    ((0, 0, _above(2.25)), OCCLUDED, "zc just above z + tol"),
    ((0, 0, 2), SEEN, "on the surface"),
    ((0, 0, -1), OUTSIDE, "behind the camera"),
    ((np.nan, 0, 1), OUTSIDE, "NaN x"), ((0, 0, np.nan), OUTSIDE, "NaN z"), ((np.inf, 0, 1), OUTSIDE, "inf x"),
    ((0, 0, np.inf), OUTSIDE, "inf z: u is NaN"), ((0, -np.inf, 1), OUTSIDE, "-inf y"),
)


def boundary_points():
    return np.array([p for p, _, _ in BOUNDARY], np.float32)


def boundary_codes():
    return np.array([[c for _, c, _ in BOUNDARY]], np.uint8)


# ---- comparisons --------------------------------------------------------------------------------------------------------
def h(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def same(a, b):
    """Two arrays or tensors equal in dtype, shape and every value."""
    a, b = h(a), h(b)
    return a.dtype == b.dtype and a.shape == b.shape and bool((a == b).all())


def same_vis(a, b):
    return all(same(x, y) and h(x).dtype == np.int32 for x, y in zip(a, b))


def loop_statement(xyz, fr, near, far, edge, band, rel):
    """The rule restated as a plain loop over probes with np.float32 scalars: (codes uint8 [F, n], counts int32 [3, n])."""
    d = fr.depth.numpy()
    F, H, W = d.shape
    inv = frames.inverse_records(fr)
    near, far, edge, band, rel, shift = f32(near), f32(far), f32(edge or 0), f32(band), f32(rel), f32(fr.depth_shift)

    def depth_at(f, j, i):
        return f32(d[f, j, i]) / shift

    def valid(f, j, i):
        z = depth_at(f, j, i)
        if not (near <= z <= far):
            return False
        if edge > 0:
            for jj, ii in ((j, i - 1), (j, i + 1), (j - 1, i), (j + 1, i)):
                if 0 <= jj < H and 0 <= ii < W:
                    zn = depth_at(f, jj, ii)
                    if near <= zn <= far and abs(zn - z) > edge * z:
                        return False
        return True

    codes = np.zeros((F, xyz.shape[0]), np.uint8)
    with np.errstate(all="ignore"):
        for f in range(F):
            fx, fy, cx, cy = (f32(v) for v in fr.table[f, :4])
            m, t = inv[f, :9].reshape(3, 3), inv[f, 9:]
            for p in range(xyz.shape[0]):
                dd = [f32(xyz[p, a]) - t[a] for a in range(3)]
                c = [(m[a, 0] * dd[0] + m[a, 1] * dd[1]) + m[a, 2] * dd[2] for a in range(3)]
                zc = c[2]
                if not (zc >= near):
                    continue
                u, v = ((c[0] * fx) / zc) + cx, ((c[1] * fy) / zc) + cy
                assert type(u) is np.float32 and type(v) is np.float32
                i, j = np.floor(u), np.floor(v)
                if not (0 <= i < W and 0 <= j < H):
                    continue
                i, j = int(i), int(j)
                if not valid(f, j, i):
                    codes[f, p] = UNKNOWN
                    continue
                z = depth_at(f, j, i)
                tol = (rel * z) + band
                codes[f, p] = FREE if zc < z - tol else OCCLUDED if zc > z + tol else SEEN
    counts = np.stack([(codes == k).sum(0) for k in (SEEN, FREE, OCCLUDED)]).astype(np.int32)
    return codes, counts
