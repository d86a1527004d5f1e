"""Synthetic posed depth frames shared by test_frames_host.py and test_gpu_frames.py: scene.make_small_scene seen by a few
render.look_at perspective cameras, the depth taken from render.splat_host's keys (depth_of_keys, supersample 1) and the
colours from render.resolve_host with NO_SHADE.  Every case is built once per process and must not be modified."""
import functools

import numpy as np

from geoformer_amd import frames, render, scene

# Sizes, each next to the constant it straddles (csrc/frames.hip):
WAVE = 64                    # one ballot / one mask word
ROUND = 256                  # FR_THREADS: the pixels of one round of a workgroup
CHUNK = 2048                 # FR_CHUNK = frames.DEFAULT_CHUNK: the pixels of one workgroup
SMALL_CHUNK = 64             # the smallest chunk: a workgroup per mask word
TOP = 256                    # SCAN_THREADS: the chunk counts k_fr_top scans before it carries
NARROW = (67, 5)             # W x H: 67 = WAVE + 3, no multiple of the wave or of strides 2 and 3; 3 frames = 1005 pixels
#                              = 3 ROUNDs + 237, one workgroup at CHUNK and 16 at SMALL_CHUNK (the last one 45 pixels)
DENSE = (80, 60)             # W x H: 4800 pixels per frame = 2 CHUNKs + 704; 3 frames = 14400 = 7 CHUNKs + 64 pixels (8
#                              workgroups), 225 SMALL_CHUNKs (< TOP: the scan's first regime)
DENSE_FRAMES_TOP = 4         # 4 frames = 19200 pixels = 300 SMALL_CHUNKs > TOP: the scan's carry
CELL_POINTS = 20000          # random points alone in their cells: 20000 cells = 313 SMALL_CHUNKs > TOP, 10 CHUNKs
FAR_FILL = 3.0               # metres: the depth put behind the scene where a frame must have no invalid pixel

assert CHUNK == frames.DEFAULT_CHUNK
assert -(-DENSE[0] * DENSE[1] * 3 // SMALL_CHUNK) < TOP < -(-DENSE[0] * DENSE[1] * DENSE_FRAMES_TOP // SMALL_CHUNK)
assert CELL_POINTS // SMALL_CHUNK > TOP


@functools.lru_cache(maxsize=None)
def small_scene():
    """(xyz float32 [N, 3], rgb uint8 [N, 3]) of scene.make_small_scene(8192, 7)."""
    sc = scene.make_small_scene(8192, 7)
    rgb = np.clip(np.rint((sc["rgb"].astype(np.float64) + 1) * 127.5), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(sc["xyz"], np.float32), rgb


def cameras(n, size, focal):
    """n perspective cameras on a circle around the scene, 2.2 m from its centre, looking at it; fx = fy = focal."""
    xyz, _ = small_scene()
    c = (xyz.min(0).astype(np.float64) + xyz.max(0)) / 2
    W, H = size
    cams = []
    for k in range(n):
        az = 0.4 + 2 * np.pi * k / max(n, 3)
        eye = c + 2.2 * np.array([np.cos(az) * np.cos(0.5), np.sin(az) * np.cos(0.5), np.sin(0.5)])
        cams.append(render.Camera(tuple(eye), tuple(render.look_at(eye, c).reshape(9)), "persp", float(focal), W / 2.0,
                                  H / 2.0, 0.05))
    return cams


def pose_of(cam):
    """The camera-to-world pose float64 [4, 4] of a render.Camera: R = P[:3, :3]^T, eye = P[:3, 3]."""
    P = np.eye(4)
    P[:3, :3] = np.asarray(cam.R, np.float64).reshape(3, 3).T
    P[:3, 3] = cam.eye
    return P


class Case(dict):
    """depth_m float32 [F, H, W] (0 = nothing seen), depth_mm uint16, color uint8 [F, H, W, 3], index int32 [F, H, W] (the
    source point of every pixel, -1 background), K float64 [4], pose float64 [F, 4, 4], cams."""
    __getattr__ = dict.__getitem__


@functools.lru_cache(maxsize=None)
def rendered(n, size, focal, radius):
    xyz, rgb = small_scene()
    W, H = size
    cams = cameras(n, size, focal)
    keys = render.splat_host(xyz, None, render.camera_table(cams, 1, radius), W, H, radius)
    color, index = render.resolve_host(keys, 1, rgb, shade=render.NO_SHADE, background=(0, 0, 0))
    depth = np.where(index >= 0, render.depth_of_keys(keys), np.float32(0)).astype(np.float32)
    assert depth.max() < 10 and (depth[index >= 0] > 0.5).all()
    mm = np.rint(depth.astype(np.float64) * 1000).astype(np.uint16)
    for a in (depth, mm, color, index):
        a.setflags(write=False)
    return Case(depth_m=depth, depth_mm=mm, color=color, index=index, K=np.array([focal, focal, W / 2.0, H / 2.0]),
                pose=np.stack([pose_of(c) for c in cams]), cams=cams)


def narrow():
    """3 frames of NARROW, discs of radius 2."""
    return rendered(3, NARROW, 40.0, 2)


def dense(n=3):
    """n frames of DENSE, discs of radius 2 (nearly every pixel of the scene's outline is covered)."""
    return rendered(n, DENSE, 50.0, 2)


def round_trip():
    """3 frames of DENSE at radius 0: a pixel holds exactly the one point that projects into it."""
    return rendered(3, DENSE, 50.0, 0)


def make(case, kind="u16", color=True, depth=None):
    """frames.Frames of a case: kind "u16" (millimetres, depth_shift 1000) or "f32" (metres, depth_shift 1)."""
    d = depth if depth is not None else (case.depth_mm if kind == "u16" else case.depth_m)
    return frames.make(np.array(d), case.K, case.pose, np.array(case.color) if color else None,
                       1000.0 if d.dtype == np.uint16 else 1.0)


@functools.lru_cache(maxsize=None)
def gaps(n=3):
    """(depth_m float32 [n, H, W]) of dense(n) with frame 1 all zeros -- its workgroups keep no pixel -- and the last
    frame's background at FAR_FILL metres -- its workgroups keep every pixel."""
    d = np.array(dense(n).depth_m)
    d[1] = 0
    d[n - 1][d[n - 1] == 0] = FAR_FILL
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def nasty():
    """depth_m of dense() with NaN, +-inf, 0 and negative values sown over a fifth of the pixels."""
    d = np.array(dense().depth_m)
    rng = np.random.default_rng(3)
    pick = rng.random(d.shape)
    for lo, v in ((0.00, np.nan), (0.04, np.inf), (0.08, -np.inf), (0.12, 0.0), (0.16, -1.5)):
        d[(pick >= lo) & (pick < lo + 0.04)] = v
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def random_points(n=CELL_POINTS, seed=5):
    """(xyz float32 [n, 3] in [0, 2)^3, rgb uint8 [n, 3])."""
    rng = np.random.default_rng(seed)
    xyz = (rng.random((n, 3)) * 2).astype(np.float32)
    rgb = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    xyz.setflags(write=False)
    rgb.setflags(write=False)
    return xyz, rgb
