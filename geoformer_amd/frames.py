"""Scenes from posed depth frames: the step in front of every other entry point of the package when there is no
reconstructed cloud yet, only a stream of depth images with intrinsics and camera-to-world poses (an RGB-D sensor, a
phone, a headset).

    fr = frames.make(depth, K, pose, color)            # depth uint16 [F, H, W] (millimetres) or float32
    fused = frames.fuse(fr, cell=0.02, edge=0.05)      # one point per 2 cm cell: xyz, rgb, count, point_of
    raw, shift = fused.raw_scene()                     # float64 [n, 8], what batch_eval.* takes
    (name, labels), = batch_eval.label_batches(model, [("scan", raw)], 1)
    ids = frames.gather(fused, labels.ids, fill=0)     # int32 [F, Hs, Ws]: the instance id of every depth pixel
    sem, inst = frames.lift_scene(fused, label_images, instance_images, ignore=0)   # pixel labels onto the points, by vote
    raw, shift = fused.raw_scene(semantic=sem, instance=inst)                       # ... a scene with its ground truth

The hot path is csrc/frames.hip: gf_frames_backproject (pixel validity, the edge filter, the world point, an ordered
compaction as count / scan / write), pointops.grid_subsample for the cells, and gf_frames_cell_means (fixed-point
integer sums per cell, the mean, the cells seen often enough renumbered in order).  backproject_host, cell_means_host
and fuse_host are the numpy statement -- the same operations in the same order -- and the kernels are tested bit for
bit against them.  Conventions are render.py's: camera axes x right, y down, z forward, pixel i covers [i, i + 1), so
its centre is i + 0.5; pose is camera to world, R = pose[:3, :3]^T, eye = pose[:3, 3].

While the sensor is still moving (csrc/frames_stream.hip): a map that persists between calls.

    fuser = frames.Fuser(cell=0.02, edge=0.05)         # the grid and the integer sums of fuse, kept between calls
    cells = [fuser.add(chunk) for chunk in chunks]     # int32 [F, Hs, Ws] per chunk; a cell keeps its number
    fused = fuser.snapshot(1, torch.cat(cells))        # what fuse(concat(chunks), origin=fuser.origin) returns, as bits

... and its labels with it (csrc/frames_vote_stream.hip): the votes persist as the cells do, nothing is kept.

    sem_v, ins_v = frames.Voter(ignore=0), frames.Voter(ignore=0)
    for chunk, labels, instances in stream:
        cells = fuser.add(chunk); sem_v.add(cells, labels); ins_v.add(cells, instances)
    sem, inst = frames.lift_scene_stream(fuser, sem_v, ins_v)   # lift_scene over every frame so far, as bits

... and the model's instances keep their ids from one snapshot to the next (csrc/frames_track.hip).

    tracker = frames.Tracker(iou=0.3, max_misses=2)
    tracked = frames.track_scene(tracker, fuser, labels)        # labels: label_batches on fuser.snapshot()'s scene
    ids = frames.gather(fused, tracked.ids)                     # the persistent id of every depth pixel

... and cells that later frames look through are dropped (csrc/frames_carve.hip): free-space evidence.

    carver = frames.Carver(fuser)
    for chunk in chunks:
        cells = fuser.add(chunk); carver.observe(chunk)         # seen / free counts and a clamped score per cell
    fused = fuser.snapshot(1, cells, keep=carver.keep())        # ... lift_scene_stream and track_scene take keep= too
    vis = frames.visibility(points, chunk)                      # on its own: in how many frames is a point seen
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

RECORD_FLOATS = 16        # gf_frames_record_floats(): {fx, fy, cx, cy, P[12]}; asserted against the library in limits()
MAX_FRAMES = 1 << 16      # gf_frames_max_frames()
MAX_SIDE = 1 << 13        # gf_frames_max_side()
DEFAULT_CHUNK = 2048      # gf_frames_default_chunk(): elements one workgroup compacts
MAX_CHUNK = 1 << 16
MAX_POINTS = 1 << 29      # gf_resample_max_points()
UNITS = 1048576.0         # fixed-point units per metre of the cell sums
REACH = 16384.0           # metres from the origin the integer sums are proven for
AGGREGATE = True          # runs of equal cells among adjacent lanes are added in the wave before the atomics
IGNORE_LABEL = -100
VOTE_MAX_PROBES = 128     # gf_frames_vote_max_probes(): the probes of a thread in a table of fewer than 2 T slots
VOTE_MIN_SLOTS, VOTE_MAX_SLOTS = 64, 1 << 30
VOTE_AGGREGATE = True     # runs of equal (group, value) pairs among adjacent lanes add once
STREAM_REACH = 4096.0     # gf_frames_map_reach(): metres from the origin a Fuser's integer sums are proven for
STREAM_MAX_PIXELS = 2 ** 31 - 1   # gf_frames_map_max_pixels(): the valid pixels a Fuser takes in all
STREAM_MAX_PROBES = 128   # gf_frames_map_max_probes(): the probes of a thread in a table of fewer than 2 (M + n) slots
STREAM_MIN_SLOTS, STREAM_MAX_SLOTS = 64, 1 << 31
STREAM_AGGREGATE = True   # runs of equal cells among adjacent lanes are added in the wave before the atomics
STREAM_MARGIN = 64.0      # metres below the first chunk's minimum a Fuser puts its origin when none is given
VOTER_MAX_PROBES = 128    # gf_frames_votes_max_probes(): the probes of a thread in a table of fewer than 2 (P + T) slots
VOTER_MAX_ELEMENTS = 2 ** 31 - 1  # gf_frames_votes_max_elements(): the elements a Voter takes in all, counted as offered
VOTER_MIN_SLOTS, VOTER_MAX_SLOTS = 64, 1 << 31   # (a slot is recorded as a non-negative int32)
VOTER_MAX_GROUPS = 2 ** 31 - 1    # the n of a snapshot
VOTER_AGGREGATE = True    # runs of equal (group, value) pairs among adjacent lanes record one add
TRACK_MAX_ROWS = 4096     # gf_frames_track_max_rows(): the rows (instances) of one Tracker update
TRACK_MAX_PROBES = 128    # gf_frames_track_max_probes(): the probes of a thread in a pair table of fewer than 2 m slots
TRACK_MAX_TRACKS = 1 << 30   # gf_frames_track_max_tracks(): the ids a Tracker hands out in all
TRACK_MIN_SLOTS, TRACK_MAX_SLOTS = 64, 1 << 30
TRACK_AGGREGATE = True    # runs of equal (row, track) pairs among adjacent lanes add once
_TRACK_WORDS = 16         # gf_frames_track_words()
_TRACK_MIN_MAP, _TRACK_MIN_TABLE = 1024, 64   # the first capacities of a Tracker's map and table, doubled as needed
CARVE_STAGE = 16          # gf_frames_carve_stage_frames(): the frame records a workgroup holds in LDS at a time
CARVE_THREADS = 256       # gf_frames_carve_threads(): the points of one workgroup
CARVE_VARIANT = 0         # the launch shape: 0 a thread per point over the frames, 1 a thread per probe
_CARVE_MIN_ROWS = 1024    # the first capacity of a Carver's state, doubled as needed


class Frames(NamedTuple):
    """What make() checked: depth uint16 or float32 [F, H, W] and color uint8 [F, H, W, 3] or None as torch tensors (on
    any device), table float32 [F, RECORD_FLOATS] on the host, the divisor that takes a depth value to metres."""
    depth: torch.Tensor
    color: object
    table: np.ndarray
    depth_shift: float


class Fused(NamedTuple):
    """xyz fp32 [n, 3], rgb uint8 [n, 3], count int32 [n] (the pixels that saw the point) and point_of int32 [F, Hs, Ws]:
    the fused point of every sampled pixel, -1 for an invalid pixel or a dropped cell."""
    xyz: torch.Tensor
    rgb: torch.Tensor
    count: torch.Tensor
    point_of: torch.Tensor

    def raw_scene(self, center=True, semantic=None, instance=None):
        """(raw float64 [n, 8], shift float64 [3]): the scene as data/scannetv2/prepare_data_inst.py stores one --
        coordinates minus their float64 mean (the shift; zeros with center=False), colours / 127.5 - 1, both labels
        -100 -- which every batch_eval entry point takes as it is.  raw[:, :3] + shift are the fused coordinates.
        semantic, instance: per-point labels [n] (lift_scene's) for columns 6 and 7, which then hold a ground truth."""
        xyz = self.xyz.detach().cpu().numpy().astype(np.float64)
        shift = xyz.mean(0) if center and xyz.shape[0] else np.zeros(3)
        raw = np.empty((xyz.shape[0], 8), np.float64)
        raw[:, :3] = xyz - shift
        raw[:, 3:6] = self.rgb.detach().cpu().numpy().astype(np.float64) / 127.5 - 1
        raw[:, 6:] = IGNORE_LABEL
        for col, lab, name in ((6, semantic, "semantic"), (7, instance, "instance")):
            if lab is not None:
                lab = lab.detach().cpu().numpy() if torch.is_tensor(lab) else np.asarray(lab)
                if lab.shape != (xyz.shape[0],) or lab.dtype.kind not in "iu":
                    raise ValueError(f"raw_scene: {name}: expected integers [{xyz.shape[0]}], got {lab.dtype} {lab.shape}")
                raw[:, col] = lab
        return raw, shift


class Lifted(NamedTuple):
    """What a vote leaves per group (per fused point): label int32 [n] (the value most of the group's votes hold, the
    smallest of them on a tie, `fill` without a vote), votes int32 [n] (the votes for it) and total int32 [n] (the
    group's votes), as torch tensors on one device."""
    label: torch.Tensor
    votes: torch.Tensor
    total: torch.Tensor

    def where(self, min_votes=1, min_share=None, fill=IGNORE_LABEL):
        """label, with `fill` where votes < min_votes or (with min_share) votes.double() < min_share * total.double():
        one float64 multiplication and one comparison per point, the same result on every device."""
        bad = self.votes < int(min_votes)
        if min_share is not None:
            bad = bad | (self.votes.double() < float(min_share) * self.total.double())
        return torch.where(bad, torch.full_like(self.label, int(fill)), self.label)


def _tensor(a, name):
    if torch.is_tensor(a):
        return a
    if isinstance(a, np.ndarray):
        return torch.from_numpy(np.ascontiguousarray(a))
    raise ValueError(f"frames.make: {name}: expected a numpy array or a torch tensor, got {type(a).__name__}")


def make(depth, K, pose, color=None, depth_shift=1000.0):
    """Frames of depth [F, H, W] (uint16, or float32), K [4] or [F, 4] = (fx, fy, cx, cy) in pixels, pose [F, 4, 4]
    camera to world, color uint8 [F, H, W, 3] aligned with the depth or None; a depth value d is d / depth_shift metres
    (ScanNet: 1000; 1 for metres).  ValueError for wrong shapes or dtypes, a record that is not finite, fx or fy <= 0, or
    a pose whose last row is not (0, 0, 0, 1).  Records are computed in float64 and rounded to float32 once."""
    depth = _tensor(depth, "depth")
    if depth.dim() != 3 or depth.dtype not in (torch.uint16, torch.float32) or 0 in depth.shape:
        raise ValueError(f"frames.make: depth: expected uint16 or float32 [F, H, W], got {depth.dtype} {tuple(depth.shape)}")
    F, H, W = depth.shape
    if not (1 <= F <= MAX_FRAMES and H <= MAX_SIDE and W <= MAX_SIDE):
        raise ValueError(f"frames.make: {F} frames of {W} x {H} pixels (1 to {MAX_FRAMES} frames, each side 1 to {MAX_SIDE})")
    if color is not None:
        color = _tensor(color, "color")
        if color.dtype != torch.uint8 or tuple(color.shape) != (F, H, W, 3):
            raise ValueError(f"frames.make: color: expected uint8 {(F, H, W, 3)}, got {color.dtype} {tuple(color.shape)}")
        if color.device != depth.device:
            raise ValueError(f"frames.make: color on {color.device}, depth on {depth.device}")
        color = color.contiguous()
    K = np.asarray(K.detach().cpu() if torch.is_tensor(K) else K)
    pose = np.asarray(pose.detach().cpu() if torch.is_tensor(pose) else pose)
    if K.dtype.kind not in "fiu" or K.shape not in ((4,), (F, 4)):
        raise ValueError(f"frames.make: K: expected numbers [4] or [{F}, 4], got {K.dtype} {K.shape}")
    if pose.dtype.kind not in "fiu" or pose.shape != (F, 4, 4):
        raise ValueError(f"frames.make: pose: expected numbers [{F}, 4, 4], got {pose.dtype} {pose.shape}")
    ds = np.float32(depth_shift)
    if not (ds > 0 and np.isfinite(ds)):
        raise ValueError(f"frames.make: depth_shift must be positive and finite in float32, got {depth_shift!r}")
    t = np.empty((F, RECORD_FLOATS), np.float64)
    t[:, :4] = np.broadcast_to(K.astype(np.float64), (F, 4))
    t[:, 4:] = pose.astype(np.float64)[:, :3, :].reshape(F, 12)
    if not np.isfinite(t).all() or not np.isfinite(pose.astype(np.float64)).all():
        raise ValueError("frames.make: K or pose holds a value that is not finite")
    if not (t[:, :2] > 0).all():
        raise ValueError("frames.make: fx and fy must be positive")
    if not (pose[:, 3, :] == np.array([0, 0, 0, 1])).all():
        raise ValueError("frames.make: the last row of every pose must be (0, 0, 0, 1)")
    with np.errstate(over="ignore"):
        table = t.astype(np.float32)
    if not np.isfinite(table).all() or not (table[:, :2] > 0).all():
        raise ValueError("frames.make: a record is not finite (or fx, fy not positive) in float32")
    return Frames(depth.contiguous(), color, table, float(ds))


def camera(fr, f, size=None):
    """The render.Camera of frame f, for images of size = (W, H) pixels (default: the frame's own size; another size
    scales the intrinsics): predictions drawn with it are seen from the frame's own viewpoint.  ValueError unless
    fx == fy (render's cameras have one focal length)."""
    from . import render

    F, H, W = fr.depth.shape
    if not 0 <= int(f) < F:
        raise ValueError(f"frames.camera: frame {f} of {F}")
    fx, fy, cx, cy = (float(v) for v in fr.table[int(f), :4])
    if fx != fy:
        raise ValueError(f"frames.camera: frame {f}: fx = {fx} and fy = {fy} differ")
    Wo, Ho = (W, H) if size is None else (int(s) for s in size)
    sx, sy = Wo / W, Ho / H
    if abs(sx - sy) > 1e-9 * max(sx, sy):
        raise ValueError(f"frames.camera: size {Wo} x {Ho} does not keep the frame's aspect {W} x {H}")
    P = fr.table[int(f), 4:].astype(np.float64).reshape(3, 4)
    return render.Camera(tuple(P[:, 3]), tuple(P[:, :3].T.reshape(9)), "persp", fx * sx, cx * sx, cy * sy)


# ---- the host statement -----------------------------------------------------------------------------------------------
def _args(fr, stride, near, far, edge, who):
    if not isinstance(fr, Frames):
        raise ValueError(f"{who}: expected the Frames of frames.make")
    stride = int(stride)
    if stride < 1:
        raise ValueError(f"{who}: stride = {stride} (>= 1)")
    e = np.float32(0.0 if edge is None else edge)
    if not (e >= 0 and np.isfinite(e)):
        raise ValueError(f"{who}: edge must be None or >= 0 and finite in float32, got {edge!r}")
    F, H, W = fr.depth.shape
    Hs, Ws = -(-H // stride), -(-W // stride)
    if F * Hs * Ws > MAX_POINTS:
        raise ValueError(f"{who}: {F * Hs * Ws} sampled pixels (at most {MAX_POINTS})")
    return stride, np.float32(near), np.float32(far), e, Hs, Ws


def _chunk(chunk, who):
    c = 0 if chunk is None else int(chunk)
    if c and not (64 <= c <= MAX_CHUNK and c % 64 == 0):
        raise ValueError(f"{who}: chunk = {chunk} (None, or a multiple of 64 from 64 to {MAX_CHUNK})")
    return c


def _shift2(a, dx, dy, fill):
    """out[f, y, x] = a[f, y + dy, x + dx] inside the image, fill outside."""
    from .render import _shifted

    return _shifted(a, dx, dy, fill)


def backproject_host(fr, stride=1, near=0.1, far=10.0, edge=None):
    """The statement of gf_frames_backproject, float32 with every operation rounded on its own: (xyz fp32 [n, 3], rgb
    uint8 [n, 3], pixel_of int32 [n], point_of int32 [F, Hs, Ws], flag).  The sampled pixel (i0, j0) is the pixel
    (i0 stride, j0 stride); z = d / depth_shift; a pixel is valid when near <= z <= far and, with edge, none of its four
    neighbours at one full-resolution pixel that is inside the image and itself in range has |zn - z| > edge z;
    xc = (((i + 0.5) - cx) z) / fx, yc likewise; X = ((P0 xc + P1 yc) + P2 z) + P3.  Valid pixels in ascending order of
    (f, j0, i0); flag: some coordinate is not finite."""
    stride, near, far, edge, Hs, Ws = _args(fr, stride, near, far, edge, "backproject_host")
    f32 = np.float32
    d = fr.depth.detach().cpu().numpy()
    F, H, W = d.shape
    with np.errstate(all="ignore"):
        z = d.astype(np.float32) / f32(fr.depth_shift)
        assert z.dtype == np.float32
        inr = (z >= near) & (z <= far)
        ok = inr.copy()
        if edge > 0:
            lim = edge * z
            for dx, dy in ((-1, 0), (1, 0), (0, -1), (0, 1)):
                zn = _shift2(z, dx, dy, f32(0))
                ok &= ~(_shift2(inr, dx, dy, False) & (np.abs(zn - z) > lim))
        ok, z = ok[:, ::stride, ::stride], z[:, ::stride, ::stride]
        t = fr.table
        i = (np.arange(Ws, dtype=np.int64) * stride).astype(np.float32)[None, None, :]
        j = (np.arange(Hs, dtype=np.int64) * stride).astype(np.float32)[None, :, None]
        col = lambda k: t[:, k][:, None, None]  # noqa: E731
        xc = (((i + f32(0.5)) - col(2)) * z) / col(0)
        yc = (((j + f32(0.5)) - col(3)) * z) / col(1)
        world = [((col(4 + 4 * a) * xc + col(5 + 4 * a) * yc) + col(6 + 4 * a) * z) + col(7 + 4 * a) for a in range(3)]
        assert all(w.dtype == np.float32 for w in world)
    sel = ok.reshape(-1)
    pixel_of = np.nonzero(sel)[0].astype(np.int32)
    xyz = np.stack([w.reshape(-1)[sel] for w in world], axis=1) if pixel_of.size else np.zeros((0, 3), np.float32)
    if fr.color is not None:
        rgb = fr.color.detach().cpu().numpy()[:, ::stride, ::stride].reshape(-1, 3)[sel]
    else:
        rgb = np.zeros((pixel_of.size, 3), np.uint8)
    point_of = np.full(sel.shape, -1, np.int32)
    point_of[sel] = np.arange(pixel_of.size, dtype=np.int32)
    return (np.ascontiguousarray(xyz, np.float32), np.ascontiguousarray(rgb), pixel_of, point_of.reshape(F, Hs, Ws),
            int(not np.isfinite(xyz).all()))


def cell_means_host(xyz, rgb, cell_of, count, origin, min_obs=1):
    """The statement of gf_frames_cell_means: (xyz_out fp32 [m, 3], rgb_out uint8 [m, 3], count_out int32 [m], new_id
    int32 [M], flag).  Per point and axis, float64: q = (int64)floor((x - o) 1048576) -- units of 2^-20 m, the
    multiplication exact; per cell the int64 sum of q, mean = (float)(o + (sum / count) 2^-20); colour per channel the
    integer (sum + count // 2) // count.  Cells with count >= min_obs keep their order and are renumbered densely;
    new_id is -1 for the others.  Integer sums: no result depends on the order of the points.  flag: a point with
    !(0 <= x - o < 16384), beyond what the sums are proven for."""
    h = lambda a: a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)  # noqa: E731
    xyz, rgb, cell_of, count, origin = h(xyz), h(rgb), h(cell_of), h(count), h(origin)
    n, M = xyz.shape[0], count.shape[0]
    if not (xyz.dtype == np.float32 and xyz.shape == (n, 3) and rgb.dtype == np.uint8 and rgb.shape == (n, 3)
            and cell_of.dtype == np.int32 and cell_of.shape == (n,) and count.dtype == np.int32 and count.ndim == 1
            and origin.dtype == np.float32 and origin.shape == (3,)):
        raise ValueError("cell_means_host: expected xyz float32 [n, 3], rgb uint8 [n, 3], cell_of int32 [n], count int32 [M] "
                         "and origin float32 [3]")
    if int(min_obs) < 1:
        raise ValueError(f"cell_means_host: min_obs = {min_obs} (>= 1)")
    if n and not (cell_of.min() >= 0 and cell_of.max() < M):
        raise ValueError("cell_means_host: cell_of outside [0, M)")
    if not (count >= 1).all():
        raise ValueError("cell_means_host: every count must be at least 1")
    o = origin.astype(np.float64)
    with np.errstate(all="ignore"):
        e = xyz.astype(np.float64) - o
        good = ((e >= 0) & (e < REACH)).all(1)
        q = np.floor(np.where(good[:, None], e, 0.0) * UNITS).astype(np.int64)
    vals = np.concatenate([q, rgb.astype(np.int64)], axis=1)
    order = np.argsort(cell_of[good], kind="stable")
    csum = np.zeros((int(good.sum()) + 1, 6), np.int64)
    np.cumsum(vals[good][order], axis=0, out=csum[1:])
    start = np.searchsorted(cell_of[good][order], np.arange(M + 1))
    sums = csum[start[1:]] - csum[start[:-1]]  # [M, 6]
    keep = count >= int(min_obs)
    new_id = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
    cnt = count[keep].astype(np.int64)
    mean = (sums[keep, :3].astype(np.float64) / cnt[:, None].astype(np.float64)) * (1.0 / UNITS)
    xyz_out = (o + mean).astype(np.float32)
    rgb_out = ((sums[keep, 3:] + (cnt // 2)[:, None]) // cnt[:, None]).astype(np.uint8)
    return xyz_out, rgb_out, count[keep].astype(np.int32), new_id, int(not good.all())


def _origin_arg(origin, who):
    if origin is None:
        return None
    o = origin.detach().cpu().numpy() if torch.is_tensor(origin) else np.asarray(origin)
    o = o.astype(np.float32).reshape(-1)
    if o.shape != (3,) or not np.isfinite(o).all():
        raise ValueError(f"{who}: origin: three finite numbers")
    return o


def _fuse_args(cell, min_obs, who):
    from . import postprocess

    c = postprocess._grid_args(cell, "first", who)
    if int(min_obs) < 1:
        raise ValueError(f"{who}: min_obs = {min_obs} (>= 1)")
    return c, int(min_obs)


_NOT_FINITE = "a back-projected coordinate is not finite (depth, intrinsics and pose give a value beyond float32)"
_BEYOND = f"a point lies {int(REACH)} m or more from the grid's origin"


def fuse_host(fr, cell=0.02, stride=1, near=0.1, far=10.0, edge=None, min_obs=1, origin=None):
    """The statement of fuse, on the host: backproject_host, postprocess.grid_subsample_host (mode "first"; origin: the
    caller's, or the per-axis float32 minimum of the points), cell_means_host, and point_of composed through cell_of
    and new_id.  Returns a Fused of CPU tensors."""
    from . import postprocess

    c, min_obs = _fuse_args(cell, min_obs, "fuse_host")
    origin = _origin_arg(origin, "fuse_host")
    xyz, rgb, _, point_of, flag = backproject_host(fr, stride, near, far, edge)
    if flag:
        raise ValueError(f"fuse_host: {_NOT_FINITE}")
    if xyz.shape[0] == 0:
        return _empty(point_of.shape, "cpu")
    if origin is None:
        origin = xyz.min(0)
    _, cell_of, count = postprocess.grid_subsample_host(xyz, c, "first", origin)
    xyz_out, rgb_out, count_out, new_id, flag = cell_means_host(xyz, rgb, cell_of, count, origin, min_obs)
    if flag:
        raise ValueError(f"fuse_host: {_BEYOND}")
    fused_of = np.where(point_of >= 0, new_id[cell_of[np.maximum(point_of, 0)]], -1).astype(np.int32)
    return Fused(*(torch.from_numpy(np.ascontiguousarray(a)) for a in (xyz_out, rgb_out, count_out, fused_of)))


def _empty(shape, device):
    return Fused(torch.zeros((0, 3), dtype=torch.float32, device=device), torch.zeros((0, 3), dtype=torch.uint8, device=device),
                 torch.zeros(0, dtype=torch.int32, device=device), torch.full(tuple(shape), -1, dtype=torch.int32, device=device))


# ---- device wrappers --------------------------------------------------------------------------------------------------
def limits():
    """(record floats, frames, side, default chunk, points) of the library, asserted against this module's constants."""
    from . import _lib

    lib = _lib.load()
    got = (lib.gf_frames_record_floats(), lib.gf_frames_max_frames(), lib.gf_frames_max_side(), lib.gf_frames_default_chunk(),
           lib.gf_resample_max_points())
    if got != (RECORD_FLOATS, MAX_FRAMES, MAX_SIDE, DEFAULT_CHUNK, MAX_POINTS):
        raise RuntimeError(f"frames: the library's limits {got} are not this module's")
    return got


def backproject(fr, stride=1, near=0.1, far=10.0, edge=None, chunk=None, return_origin=False):
    """(xyz fp32 [n, 3], rgb uint8 [n, 3], pixel_of int32 [n], point_of int32 [F, Hs, Ws]) on fr.depth's device: the valid
    pixels of the frames as world points, in ascending order of the sampled pixel (gf_frames_backproject on the current
    stream: three launches, bit-identical to backproject_host and from call to call).  The two words {n, not finite}
    are read back once (the only synchronisation); a coordinate that is not finite is a ValueError.  chunk: the pixels
    one workgroup compacts (None: the default).  return_origin: also the per-axis minimum of xyz, float32 [3] on the
    device (found by the kernel that writes the points; meaningless when n == 0) -- the default origin of fuse's grid.
    Frames on the CPU run the statement."""
    stride, near, far, e, Hs, Ws = _args(fr, stride, near, far, edge, "frames.backproject")
    chunk = _chunk(chunk, "frames.backproject")
    if not fr.depth.is_cuda:
        xyz, rgb, pixel_of, point_of, flag = backproject_host(fr, stride, near, far, edge)
        out = tuple(torch.from_numpy(a) for a in (xyz, rgb, pixel_of, point_of))
        lo = torch.from_numpy(xyz.min(0) if xyz.shape[0] else np.zeros(3, np.float32))
    else:
        from . import _lib
        from ._lib import check, ptr, stream_ptr

        lib = _lib.load()
        dev = fr.depth.device
        F, H, W = fr.depth.shape
        T = F * Hs * Ws
        with torch.cuda.device(dev):
            table = torch.from_numpy(fr.table).to(dev, non_blocking=True)
            xyz = torch.empty((T, 3), dtype=torch.float32, device=dev)
            rgb = torch.empty((T, 3), dtype=torch.uint8, device=dev)
            pixel_of = torch.empty(T, dtype=torch.int32, device=dev)
            point_of = torch.empty((F, Hs, Ws), dtype=torch.int32, device=dev)
            words = torch.empty(2, dtype=torch.int32, device=dev)
            lo = torch.empty(3, dtype=torch.float32, device=dev)
            ws = torch.empty(lib.gf_frames_backproject_scratch_bytes(T, chunk) // 8 + 1, dtype=torch.int64, device=dev)
            check(lib.gf_frames_backproject(ptr(fr.depth), int(fr.depth.dtype == torch.float32), fr.depth_shift, ptr(fr.color),
                                            ptr(table), F, W, H, stride, float(near), float(far), float(e), chunk, ptr(ws),
                                            ptr(xyz), ptr(rgb), ptr(pixel_of), ptr(point_of), ptr(lo), ptr(words), stream_ptr()),
                  "gf_frames_backproject")
            n, flag = words.tolist()
        out = xyz[:n], rgb[:n], pixel_of[:n], point_of
    if flag:
        raise ValueError(f"frames.backproject: {_NOT_FINITE}")
    return out + (lo,) if return_origin else out


def cell_means(xyz, rgb, cell_of, count, origin, min_obs=1, chunk=None, aggregate=None):
    """(xyz_out fp32 [m, 3], rgb_out uint8 [m, 3], count_out int32 [m], new_id int32 [M]) on xyz's device: one fused
    point per cell with at least min_obs points, from the cell_of and count of pointops.grid_subsample(xyz, cell,
    mode="first", origin=origin) (gf_frames_cell_means on the current stream: integer atomics only, bit-identical to
    cell_means_host and from call to call).  origin: float32 [3] tensor on the same device.  The two words {m, beyond}
    are read back once; a point 16384 m or more from the origin (or below it) is a ValueError.  aggregate: whether
    adjacent lanes of one cell add up in the wave before the atomics (None: AGGREGATE; the result is the same).  CPU
    tensors run the statement."""
    if not (torch.is_tensor(xyz) and xyz.dtype == torch.float32 and xyz.dim() == 2 and xyz.shape[1] == 3 and xyz.is_contiguous()):
        raise ValueError("frames.cell_means: xyz: expected a contiguous float32 tensor [n, 3]")
    n, M, dev = xyz.shape[0], count.shape[0] if torch.is_tensor(count) else -1, xyz.device
    for t, dt, shape, name in ((rgb, torch.uint8, (n, 3), "rgb"), (cell_of, torch.int32, (n,), "cell_of"),
                               (count, torch.int32, (M,), "count"), (origin, torch.float32, (3,), "origin")):
        if not (torch.is_tensor(t) and t.dtype == dt and tuple(t.shape) == shape and t.is_contiguous() and t.device == dev):
            raise ValueError(f"frames.cell_means: {name}: expected a contiguous {dt} tensor {shape} on {dev}")
    if int(min_obs) < 1:
        raise ValueError(f"frames.cell_means: min_obs = {min_obs} (>= 1)")
    chunk = _chunk(chunk, "frames.cell_means")
    if n == 0 or M == 0:
        if n or M:
            raise ValueError(f"frames.cell_means: {n} points in {M} cells")
        e = _empty((0,), dev)
        return e.xyz, e.rgb, e.count, e.point_of
    if not xyz.is_cuda:
        *out, flag = cell_means_host(xyz, rgb, cell_of, count, origin, min_obs)
        out = tuple(torch.from_numpy(a) for a in out)
    else:
        from . import _lib
        from ._lib import check, ptr, stream_ptr

        lib = _lib.load()
        with torch.cuda.device(dev):
            xyz_out = torch.empty((M, 3), dtype=torch.float32, device=dev)
            rgb_out = torch.empty((M, 3), dtype=torch.uint8, device=dev)
            out_i = torch.empty((2, M), dtype=torch.int32, device=dev)
            words = torch.empty(2, dtype=torch.int32, device=dev)
            ws = torch.empty(lib.gf_frames_cell_means_scratch_bytes(M, chunk) // 8 + 1, dtype=torch.int64, device=dev)
            check(lib.gf_frames_cell_means(ptr(xyz), ptr(rgb), ptr(cell_of), ptr(count), n, M, ptr(origin), int(min_obs),
                                           int(AGGREGATE if aggregate is None else aggregate), chunk, ptr(ws), ptr(xyz_out),
                                           ptr(rgb_out), ptr(out_i[0]), ptr(out_i[1]), ptr(words), stream_ptr()),
                  "gf_frames_cell_means")
            m, flag = words.tolist()
        out = xyz_out[:m], rgb_out[:m], out_i[0, :m], out_i[1]
    if flag:
        raise ValueError(f"frames.cell_means: {_BEYOND}")
    return out


def fuse(fr, cell=0.02, stride=1, near=0.1, far=10.0, edge=None, min_obs=1, origin=None, device="cuda"):
    """Fused: the frames as one point per occupied cell of `cell` metres -- the mean position and colour of the pixels
    that fell into it, the number of those pixels, and for every sampled pixel the point it went into.  stride: every
    stride-th pixel of every stride-th row; near, far: the depth range in metres; edge: drop a pixel whose depth
    differs from an in-range neighbour's by more than edge times its own (flying pixels at depth edges; None: off);
    min_obs: cells seen by fewer pixels are dropped; origin: the grid's corner, three numbers no point lies below (None:
    the per-axis minimum of the points).  Cells are numbered in order of their first pixel.  On the GPU: the frames are
    moved to `device` when they are elsewhere, then gf_frames_backproject (which also finds the points' per-axis
    minimum), pointops.grid_subsample, gf_frames_cell_means and gf_frames_compose on the current stream, with three small
    read-backs ({n, flag}, {M, invalid}, {m, flag}) as the only synchronisations; bit-identical to fuse_host and from
    call to call.  device "cpu" runs fuse_host."""
    from . import pointops

    c, min_obs = _fuse_args(cell, min_obs, "frames.fuse")
    o = _origin_arg(origin, "frames.fuse")
    _args(fr, stride, near, far, edge, "frames.fuse")
    dev = torch.device(device)
    if dev.type != "cuda":
        return fuse_host(fr, c, stride, near, far, edge, min_obs, o)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    if fr.depth.device != dev:
        fr = fr._replace(depth=fr.depth.to(dev), color=None if fr.color is None else fr.color.to(dev))
    from ._lib import check, ptr, stream_ptr
    from . import _lib

    with torch.cuda.device(dev):
        xyz, rgb, _, point_of, lo = backproject(fr, stride, near, far, edge, return_origin=True)
        if xyz.shape[0] == 0:
            return _empty(point_of.shape, dev)
        xyz, rgb = xyz.contiguous(), rgb.contiguous()  # (leading rows of the buffers: already contiguous)
        org = lo if o is None else torch.from_numpy(o).to(dev)
        try:
            _, cell_of, count = pointops.grid_subsample(xyz, c, mode="first", origin=org)
        except ValueError as e:
            raise ValueError(f"frames.fuse: {e}") from None
        xyz_out, rgb_out, count_out, new_id = cell_means(xyz, rgb, cell_of.contiguous(), count.contiguous(), org, min_obs)
        check(_lib.load().gf_frames_compose(ptr(point_of), point_of.numel(), ptr(cell_of), ptr(new_id), stream_ptr()),
              "gf_frames_compose")
    return Fused(xyz_out, rgb_out, count_out, point_of)


def gather(fused, values, fill=-1):
    """Per-point values [n] or [n, C] (a tensor or an array: label ids, classes, panoptic ids, colours) as images
    [F, Hs, Ws] or [F, Hs, Ws, C] on fused.point_of's device: every pixel takes the value of its fused point, `fill`
    where it has none.  Exact: a pixel's point is the one it was fused into, nothing is projected or occluded."""
    p = fused.point_of
    v = torch.as_tensor(values).to(p.device)
    n = fused.xyz.shape[0]
    if v.dim() not in (1, 2) or v.shape[0] != n:
        raise ValueError(f"frames.gather: values: expected [{n}] or [{n}, C], got {tuple(v.shape)}")
    out = torch.full(tuple(p.shape) + tuple(v.shape[1:]), fill, dtype=v.dtype, device=p.device)
    on = p >= 0
    out[on] = v[p[on].long()]
    return out


# ---- labels of the pixels onto the fused points: a vote ---------------------------------------------------------------
_VALUE_KINDS = {torch.uint8: 0, torch.uint16: 1, torch.int32: 2}


def vote_slots(T, n):
    """(default, proven) table sizes of a vote of T elements into n groups: the smallest power of two at or above
    2 min(T, 8 n) -- a few MB that stay in cache for the usual one or two labels per point -- and at or above 2 T, which
    no input overflows; both at least 64 (gf_frames_vote_default_slots)."""
    def pow2(v):
        p = VOTE_MIN_SLOTS
        while p < v:
            p <<= 1
        return p

    return pow2(2 * min(int(T), 8 * int(n))), pow2(2 * int(T))


def _vote_args(group, value, n, ignore, fill, who):
    def h(a):  # (a read-only or strided array is copied: a tensor wants writable, contiguous memory)
        return a if torch.is_tensor(a) else torch.from_numpy(a if a.flags.writeable and a.flags.c_contiguous else np.array(a, order="C"))

    if not (torch.is_tensor(group) or isinstance(group, np.ndarray)) or not (torch.is_tensor(value) or isinstance(value, np.ndarray)):
        raise ValueError(f"{who}: group and value: numpy arrays or torch tensors")
    group, value = h(group), h(value)
    if group.dtype != torch.int32:
        raise ValueError(f"{who}: group: expected int32, got {group.dtype}")
    if value.dtype not in _VALUE_KINDS:
        raise ValueError(f"{who}: value: expected uint8, uint16 or int32, got {value.dtype}")
    n = int(n)
    if not 0 <= n <= MAX_POINTS:
        raise ValueError(f"{who}: n = {n} groups (0 to {MAX_POINTS})")
    if group.numel() > MAX_POINTS:
        raise ValueError(f"{who}: {group.numel()} elements (at most {MAX_POINTS})")
    if ignore is not None and int(ignore) != ignore:
        raise ValueError(f"{who}: ignore must be None or an integer, got {ignore!r}")
    if not -2 ** 31 <= int(fill) < 2 ** 31:
        raise ValueError(f"{who}: fill = {fill} is no int32")
    return group, value, n, None if ignore is None else int(ignore), int(fill)


def vote_host(group, value, n, ignore=None, fill=IGNORE_LABEL):
    """(Lifted of CPU tensors, pairs): the statement of gf_frames_vote.  group int32 and value uint8, uint16 or int32
    of one shape, flattened to T elements.  Element t votes when 0 <= group[t] < n, value[t] >= 0 and value[t] != ignore
    (an int or None; ScanNet's label-filt and instance-filt images use 0 for "unannotated": lift them with ignore=0).
    group[t] >= n is a ValueError; group[t] < 0 is no vote (point_of's -1).  Per group g: total[g] = its votes; among
    its distinct values the one with the largest count wins, ties go to the smallest value; label[g] = the winner, or
    fill without a vote; votes[g] = the winner's count, or 0.  pairs: the distinct (group, value) pairs among the
    votes.  Integer counts and integer comparisons only: no result depends on the order of the elements."""
    group, value, n, ignore, fill = _vote_args(group, value, n, ignore, fill, "vote_host")
    if tuple(group.shape) != tuple(value.shape):
        raise ValueError(f"vote_host: group {tuple(group.shape)} and value {tuple(value.shape)} differ in shape")
    g = group.detach().cpu().numpy().reshape(-1).astype(np.int64)
    v = value.detach().cpu().numpy().reshape(-1).astype(np.int64)
    if (g >= n).any():
        raise ValueError(f"vote_host: a group is {int(g.max())}, outside the {n} groups")
    on = (g >= 0) & (v >= 0)
    if ignore is not None:
        on &= v != ignore
    pair, cnt = np.unique((g[on] << 32) | v[on], return_counts=True)
    pg, pv = pair >> 32, pair & 0xffffffff
    total = np.zeros(n, np.int64)
    np.add.at(total, pg, cnt)
    best = np.zeros(n, np.int64)  # count << 32 | (0xffffffff - value): the largest count, then the smallest value
    np.maximum.at(best, pg, (cnt.astype(np.int64) << 32) | (0xffffffff - pv))
    label = np.where(best > 0, 0xffffffff - (best & 0xffffffff), fill)
    out = Lifted(*(torch.from_numpy(a.astype(np.int32)) for a in (label, best >> 32, total)))
    return out, int(pair.size)


def _vote_device(group, value, F, H, W, stride, n, ignore, fill, slots, aggregate, who):
    """gf_frames_vote on group's device: group [F, Hs, Ws] (as its numel says), value [F, H, W], both contiguous."""
    from . import _lib
    from ._lib import check, ptr, stream_ptr

    lib = _lib.load()
    dev, T = group.device, group.numel()
    default, proven = vote_slots(T, n)
    if slots is not None:
        s = int(slots)
        if not (VOTE_MIN_SLOTS <= s <= VOTE_MAX_SLOTS and s & (s - 1) == 0):
            raise ValueError(f"{who}: slots = {slots} (None, or a power of two from {VOTE_MIN_SLOTS} to {VOTE_MAX_SLOTS})")
    with torch.cuda.device(dev):
        out = torch.empty((3, n), dtype=torch.int32, device=dev)
        if T == 0 or n == 0:
            if n == 0 and T and bool((group >= 0).any()):
                raise ValueError(f"{who}: a group is outside the 0 groups")
            out[0] = fill
            out[1:] = 0
            return Lifted(out[0], out[1], out[2]), 0
        has = ignore is not None and -2 ** 31 <= ignore < 2 ** 31  # (no value is another int)
        words = torch.empty(3, dtype=torch.int32, device=dev)
        for s in ((default, proven) if slots is None else (int(slots),)):
            ws = torch.empty(lib.gf_frames_vote_scratch_bytes(s, n) // 8 + 1, dtype=torch.int64, device=dev)
            check(lib.gf_frames_vote(ptr(group), ptr(value), _VALUE_KINDS[value.dtype], F, W, H, stride, n,
                                     ignore if has else 0, int(has), fill, s,
                                     int(VOTE_AGGREGATE if aggregate is None else aggregate), ptr(ws), ptr(out[0]),
                                     ptr(out[1]), ptr(out[2]), ptr(words), stream_ptr()), "gf_frames_vote")
            pairs, overflow, beyond = words.tolist()
            if beyond:
                raise ValueError(f"{who}: a group is outside the {n} groups")
            if not overflow:
                return Lifted(out[0], out[1], out[2]), pairs
            if slots is not None:
                raise ValueError(f"{who}: the table of slots = {s} overflowed; {proven} slots are always enough for "
                                 f"{T} elements")
        raise RuntimeError(f"{who}: a table of {proven} >= 2 T slots overflowed")  # (proven impossible)


def vote(group, value, n, ignore=None, fill=IGNORE_LABEL, slots=None, aggregate=None):
    """(Lifted, pairs) on group's device: vote_host's rule by gf_frames_vote on the current stream (four memsets, three
    launches; integer atomics on a hash table of the distinct pairs: bit-identical to vote_host and from call to
    call).  The three words {pairs, overflow, group out of range} are read back once per run, the only synchronisation;
    a group >= n is a ValueError.  slots: the table's entries, a power of two; with fewer than 2 T of them the table may
    overflow, which is a ValueError that names the size that is always enough.  None: the default size of vote_slots
    and, when that overflows, ONE more run at the proven size.  aggregate: whether adjacent lanes of one pair add once
    (None: VOTE_AGGREGATE; the result is the same).  CPU tensors run the statement."""
    group, value, n, ignore, fill = _vote_args(group, value, n, ignore, fill, "frames.vote")
    if tuple(group.shape) != tuple(value.shape):
        raise ValueError(f"frames.vote: group {tuple(group.shape)} and value {tuple(value.shape)} differ in shape")
    if not group.is_cuda:
        return vote_host(group, value, n, ignore, fill)
    if value.device != group.device:
        raise ValueError(f"frames.vote: value on {value.device}, group on {group.device}")
    return _vote_device(group.contiguous(), value.contiguous(), 1, 1, group.numel(), 1, n, ignore, fill, slots, aggregate,
                        "frames.vote")


def _lift(fused, images, ignore, fill, stride, slots, aggregate, host, who):
    if not isinstance(fused, Fused):
        raise ValueError(f"{who}: expected the Fused of frames.fuse")
    p = fused.point_of
    n = int(fused.xyz.shape[0])
    _, images, n, ignore, fill = _vote_args(p, images, n, ignore, fill, who)
    if p.dim() != 3:
        raise ValueError(f"{who}: point_of: expected [F, Hs, Ws], got {tuple(p.shape)}")
    F, Hs, Ws = p.shape
    s = 1 if stride is None else int(stride)
    if s < 1:
        raise ValueError(f"{who}: stride = {stride} (>= 1)")
    if images.dim() != 3 or images.shape[0] != F or (-(-images.shape[1] // s), -(-images.shape[2] // s)) != (Hs, Ws):
        raise ValueError(f"{who}: images {tuple(images.shape)} at stride {s} do not sample to point_of's {tuple(p.shape)}")
    if host or not p.is_cuda:
        return vote_host(p.detach().cpu(), images.detach().cpu().numpy()[:, ::s, ::s], n, ignore, fill)[0]
    H, W = int(images.shape[1]), int(images.shape[2])
    return _vote_device(p.contiguous(), images.to(p.device).contiguous(), F, H, W, s, n, ignore, fill, slots, aggregate, who)[0]


def lift(fused, images, ignore=None, fill=IGNORE_LABEL, stride=None, slots=None, aggregate=None):
    """Lifted on fused.point_of's device: per fused point the label most of its pixels carry -- vote() with group =
    fused.point_of.  images: uint8, uint16 or int32, of point_of's shape [F, Hs, Ws]; with stride=s the full-resolution
    images [F, H, W] as the sensor wrote them (Hs = ceil(H / s), as fuse samples), read at the sampled pixels by the
    kernel: no conversion and no slicing pass.  ignore: a value that does not vote (0 for ScanNet's label-filt and
    instance-filt).  Exact: a pixel votes for the point it was fused into, nothing is projected or occluded."""
    return _lift(fused, images, ignore, fill, stride, slots, aggregate, False, "frames.lift")


def scene_labels(sem, ins, min_votes=1, min_share=None, host=False):
    """(semantic int32 [n], instance int32 [n]) from the Lifted of the semantic and of the instance images over the same
    n points (lift's, or a Voter's snapshot): the tail of lift_scene.  A point whose instance label fails
    ins.where(min_votes, min_share) has instance -100; the surviving ids are renumbered 0 .. I-1 in ascending order of
    the original id; an instance's class is the vote of its points' lifted classes (points -> instances, the same
    kernel; vote_host with host=True) and is written to all its points; a point without an instance keeps its own."""
    if not (isinstance(sem, Lifted) and isinstance(ins, Lifted)):
        raise ValueError("frames.scene_labels: expected two Lifted")
    if sem.label.shape != ins.label.shape or sem.label.device != ins.label.device:
        raise ValueError(f"frames.scene_labels: the semantic labels {tuple(sem.label.shape)} on {sem.label.device} and the "
                         f"instance labels {tuple(ins.label.shape)} on {ins.label.device} differ in shape or device")
    sem, ins = sem.label, ins.where(min_votes, min_share)
    on = ins >= 0
    ids = torch.unique(ins[on])  # ascending
    new = torch.where(on, torch.searchsorted(ids, ins.clamp(min=0)).to(torch.int32), torch.full_like(ins, IGNORE_LABEL))
    if ids.numel() == 0:
        return sem, new
    # points -> instances: the same vote, with the new instance id as the group and the points' lifted classes as values
    cls = (vote_host if host else vote)(new, sem, int(ids.numel()))[0].label
    return torch.where(on, cls[new.clamp(min=0).long()], sem), new


def _lift_scene(fused, semantic, instance, ignore, stride, min_votes, min_share, host, who):
    sem = _lift(fused, semantic, ignore, IGNORE_LABEL, stride, None, None, host, who)
    ins = _lift(fused, instance, ignore, IGNORE_LABEL, stride, None, None, host, who)
    return scene_labels(sem, ins, min_votes, min_share, host)


def lift_scene(fused, semantic, instance, ignore=None, stride=None, min_votes=1, min_share=None):
    """(semantic int32 [n], instance int32 [n]) on point_of's device: dataset-style labels of the fused points from the
    frames' semantic and instance images (lift's shapes; instance ids consistent across the frames).  Both images are
    lifted; a point whose instance label fails Lifted.where(min_votes, min_share) has instance -100; the surviving ids
    are renumbered 0 .. I-1 in ascending order of the original id; an instance's class is the vote of its points' lifted
    classes (the same kernel, points -> instances) and is written to all its points, so that
    evaluation.gt_ids_from_labels' "label of the first point" is the instance's label whichever point comes first; a
    point without an instance keeps its own lifted class (-100 without a vote)."""
    return _lift_scene(fused, semantic, instance, ignore, stride, min_votes, min_share, False, "frames.lift_scene")


def lift_scene_host(fused, semantic, instance, ignore=None, stride=None, min_votes=1, min_share=None):
    """The statement of lift_scene on the host (vote_host throughout): CPU tensors."""
    return _lift_scene(fused, semantic, instance, ignore, stride, min_votes, min_share, True, "lift_scene_host")


# ---- a map that persists between calls: frames fused chunk by chunk ---------------------------------------------------
_BELOW = ("point(s) outside the grid (not finite in cells, below the origin, or 2097152 cells or more from it): give "
          "origin= three numbers no point of the stream will lie below, or a larger margin=")
_STREAM_BEYOND = f"a point lies {int(STREAM_REACH)} m or more from the map's origin (or below it): see origin= and margin="


_CELLS_RANGE = "cells holds a value below -1, or one outside the map's"


def concat(parts):
    """The Frames of several Frames, one after the other along the frame axis.  ValueError unless all have the same
    depth dtype, image size, depth_shift and device, and colour in all or in none."""
    parts = list(parts)
    if not parts or not all(isinstance(p, Frames) for p in parts):
        raise ValueError("frames.concat: expected a non-empty list of the Frames of frames.make")
    a = parts[0]
    for k, p in enumerate(parts[1:], 1):
        for what, x, y in (("depth dtype", a.depth.dtype, p.depth.dtype), ("image size", a.depth.shape[1:], p.depth.shape[1:]),
                           ("depth_shift", a.depth_shift, p.depth_shift), ("device", a.depth.device, p.depth.device),
                           ("colour", a.color is None, p.color is None)):
            if x != y:
                raise ValueError(f"frames.concat: part {k} differs from part 0 in {what}")
    F = sum(p.depth.shape[0] for p in parts)
    if F > MAX_FRAMES:
        raise ValueError(f"frames.concat: {F} frames (at most {MAX_FRAMES})")
    color = None if a.color is None else torch.cat([p.color for p in parts]).contiguous()
    return Frames(torch.cat([p.depth for p in parts]).contiguous(), color,
                  np.ascontiguousarray(np.concatenate([p.table for p in parts])), a.depth_shift)


def stream_slots(M, n):
    """(default, proven) table sizes of a map of M cells before a call of n points: the smallest power of two at or
    above max(4 M, n / 8) (gf_frames_map_default_slots) and at or above 2 (M + n), which no input overflows; both at
    least 64."""
    def pow2(v):
        p = STREAM_MIN_SLOTS
        while p < v:
            p <<= 1
        return p

    return pow2(max(4 * int(M), int(n) // 8)), pow2(2 * (int(M) + int(n)))


def stream_limits():
    """(probes, reach, pixels) of the library's map, asserted against this module's constants."""
    from . import _lib

    lib = _lib.load()
    got = (lib.gf_frames_map_max_probes(), lib.gf_frames_map_reach(), lib.gf_frames_map_max_pixels())
    if got != (STREAM_MAX_PROBES, STREAM_REACH, STREAM_MAX_PIXELS) or lib.gf_frames_default_chunk() != DEFAULT_CHUNK:
        raise RuntimeError(f"frames: the library's map limits {got} are not this module's")
    return got


def _stream_args(cell, stride, edge, origin, margin, who):
    c, _ = _fuse_args(cell, 1, who)
    if int(stride) < 1:
        raise ValueError(f"{who}: stride = {stride} (>= 1)")
    e = np.float32(0.0 if edge is None else edge)
    if not (e >= 0 and np.isfinite(e)):
        raise ValueError(f"{who}: edge must be None or >= 0 and finite in float32, got {edge!r}")
    m = np.float32(margin)
    if not (m >= 0 and np.isfinite(m)):
        raise ValueError(f"{who}: margin must be >= 0 and finite in float32, got {margin!r}")
    return c, int(stride), _origin_arg(origin, who), m


def _stream_sig(fr, sig, who):
    """What every chunk of a stream must share with the first: image size, depth dtype, depth_shift, colour or none."""
    if not isinstance(fr, Frames):
        raise ValueError(f"{who}: expected the Frames of frames.make")
    mine = (tuple(fr.depth.shape[1:]), fr.depth.dtype, fr.depth_shift, fr.color is not None)
    if sig is not None and mine != sig:
        raise ValueError(f"{who}: this chunk (size, dtype, depth_shift, colour) = {mine} differs from the stream's {sig}: "
                         "a chunk may differ from the one before in the number of frames only")
    return mine


def _stream_budget(pixels, n, who):
    if pixels + n > STREAM_MAX_PIXELS:
        raise ValueError(f"{who}: {pixels} valid pixels so far and {n} more: a map takes at most {STREAM_MAX_PIXELS}")


def _stream_points(xyz, rgb, who):
    h = lambda a: a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)  # noqa: E731
    xyz = h(xyz)
    if xyz.dtype != np.float32 or xyz.ndim != 2 or xyz.shape[1] != 3:
        raise ValueError(f"{who}: xyz: expected float32 [n, 3], got {xyz.dtype} {xyz.shape}")
    rgb = np.zeros((xyz.shape[0], 3), np.uint8) if rgb is None else h(rgb)
    if rgb.dtype != np.uint8 or rgb.shape != xyz.shape:
        raise ValueError(f"{who}: rgb: expected uint8 {xyz.shape} or None, got {rgb.dtype} {rgb.shape}")
    if xyz.shape[0] > MAX_POINTS:
        raise ValueError(f"{who}: {xyz.shape[0]} points (at most {MAX_POINTS})")
    if not np.isfinite(xyz).all():
        raise ValueError(f"{who}: a coordinate is not finite")
    return np.ascontiguousarray(xyz), np.ascontiguousarray(rgb)


def _cells_arg(cells, M, device, who):
    if cells is None:
        return None
    c = cells if torch.is_tensor(cells) else torch.from_numpy(np.ascontiguousarray(cells))
    if c.dtype != torch.int32:
        raise ValueError(f"{who}: cells: expected int32 (what add returned, or several of them concatenated), got {c.dtype}")
    c = c.to(device).contiguous()
    if not c.is_cuda and c.numel() and not (int(c.min()) >= -1 and int(c.max()) < M):  # (on the device: the lookup's flag)
        raise ValueError(f"{who}: {_CELLS_RANGE} {M} cells")
    return c


def _keep_arg(keep, M, device, who):
    """keep as a bool tensor [M] on `device`, or None."""
    if keep is None:
        return None
    k = keep if torch.is_tensor(keep) else torch.from_numpy(np.ascontiguousarray(keep))
    if k.dtype not in (torch.bool, torch.uint8) or k.dim() != 1:
        raise ValueError(f"{who}: keep: expected bool or uint8 [{M}], got {k.dtype} {tuple(k.shape)}")
    if k.shape[0] != M:
        raise ValueError(f"{who}: keep holds {k.shape[0]} cells, the map {M}")
    return (k != 0).to(device)


class FuserHost:
    """The statement of Fuser, in numpy: a map (cell, origin, stride, near, far, edge) that frames are added to a chunk
    at a time.  Per cell, in order of first occurrence: count and six int64 sums (three coordinates in units of 2^-20 m,
    three colour channels).

    add(fr) -> cells int32 [F, Hs, Ws]: backproject_host's rule; every valid pixel's point into its cell by
    grid_subsample_host's rule (t = (x - origin) / cell in float32, c = floor t, valid when t is finite and
    0 <= c < 2^21 per axis); a cell never seen before takes the next numbers, in ascending order of the chunk's sampled
    pixel index of its first pixel; q = (int64)floor(((double)x - (double)o) 2^20) and the colour bytes are added to the
    cell's sums and 1 to its count.  cells: the cell number of every sampled pixel, -1 for an invalid one; numbers never
    change afterwards.  ValueError -- and the map exactly as it was -- for a chunk that differs from the stream's in
    size, dtype, depth_shift or colour, a coordinate that is not finite, a point outside the grid, a point with
    !(0 <= x - o < 4096), or more than 2^31 - 1 valid pixels in all.

    snapshot(min_obs=1, cells=None) -> Fused: cell_means_host's second half on the stored sums: mean =
    (float)((double)o + ((double)sum_q / (double)count) 2^-20), colour (sum + count // 2) // count, cells with
    count >= min_obs kept in order and renumbered densely; point_of = new_id[cells] (-1 stays -1) for the cells given
    (one add's, or several concatenated along the frame axis), an empty [0, 0, 0] without.  Changes nothing.
    keep: bool or uint8 [cells] (a Carver's keep()): only cells with count >= min_obs AND keep are kept; a dropped cell's
    pixels get -1.  None and all True give the same bits; another length is a ValueError.

    For chunks c1..ck, snapshot(min_obs, cat(cells_1..cells_k)) equals fuse_host(concat(c1..ck), ..., min_obs,
    origin=map.origin) in every field, bit for bit.  origin=None: fixed at the first add with a valid pixel, at that
    chunk's per-axis float32 minimum minus margin (one float32 subtraction per axis)."""

    def __init__(self, cell=0.02, stride=1, near=0.1, far=10.0, edge=None, origin=None, margin=STREAM_MARGIN):
        self._who = "frames." + type(self).__name__
        self._cell, self._stride, self._origin, self._margin = _stream_args(cell, stride, edge, origin, margin, self._who)
        self._near, self._far, self._edge = near, far, edge
        self._sig = None
        self._keys = np.zeros(0, np.int64)
        self._count = np.zeros(0, np.int64)
        self._sums = np.zeros((0, 6), np.int64)
        self._pixels = 0

    origin = property(lambda self: None if self._origin is None else self._origin.copy(),
                      doc="float32 [3], or None before the first add with a valid pixel")
    cells = property(lambda self: int(self._keys.shape[0]), doc="the cells of the map")
    pixels = property(lambda self: self._pixels, doc="the valid pixels added so far")

    def state(self):
        """(keys int64 [M], count int64 [M], sums int64 [M, 6]) in cell order, copies."""
        return self._keys.copy(), self._count.copy(), self._sums.copy()

    def _insert(self, xyz, rgb, who):
        """cell_of int64 [n] of n >= 1 finite points; every check is made before anything changes."""
        n, M = xyz.shape[0], self._keys.shape[0]
        _stream_budget(self._pixels, n, who)
        origin = self._origin if self._origin is not None else (xyz.min(0) - self._margin).astype(np.float32)
        with np.errstate(all="ignore"):
            t = (xyz - origin) / self._cell
            c = np.floor(t)
            bad = ~(np.isfinite(t) & (c >= 0) & (c < (1 << 21))).all(1)
        if bad.any():
            raise ValueError(f"{who}: {int(bad.sum())} {_BELOW}")
        e = xyz.astype(np.float64) - origin.astype(np.float64)
        if not ((e >= 0) & (e < STREAM_REACH)).all():
            raise ValueError(f"{who}: {_STREAM_BEYOND}")
        ci = c.astype(np.int64)
        key = ci[:, 0] | ci[:, 1] << 21 | ci[:, 2] << 42
        uniq, first, inv = np.unique(key, return_index=True, return_inverse=True)
        inv = inv.reshape(-1)
        uid = np.empty(uniq.shape[0], np.int64)
        known = np.zeros(uniq.shape[0], bool)
        if M:
            order = np.argsort(self._keys, kind="stable")
            at = np.minimum(np.searchsorted(self._keys[order], uniq), M - 1)
            known = self._keys[order][at] == uniq
            uid[known] = order[at[known]]
        new = np.nonzero(~known)[0]
        new = new[np.argsort(first[new], kind="stable")]  # ascending first point: the order of first occurrence
        uid[new] = M + np.arange(new.shape[0])
        vals = np.concatenate([np.floor(e * UNITS).astype(np.int64), rgb.astype(np.int64), np.ones((n, 1), np.int64)], axis=1)
        by = np.argsort(inv, kind="stable")
        csum = np.zeros((n + 1, 7), np.int64)
        np.cumsum(vals[by], axis=0, out=csum[1:])
        start = np.searchsorted(inv[by], np.arange(uniq.shape[0] + 1))
        per = csum[start[1:]] - csum[start[:-1]]
        # nothing above changed the map
        self._origin = origin
        self._keys = np.concatenate([self._keys, uniq[new]])
        self._count = np.concatenate([self._count, np.zeros(new.shape[0], np.int64)])
        self._sums = np.concatenate([self._sums, np.zeros((new.shape[0], 6), np.int64)])
        self._sums[uid] += per[:, :6]  # (uid holds every cell once)
        self._count[uid] += per[:, 6]
        self._pixels += n
        return uid[inv]

    def add(self, fr):
        who = self._who + ".add"
        sig = _stream_sig(fr, self._sig, who)
        _args(fr, self._stride, self._near, self._far, self._edge, who)
        xyz, rgb, _, point_of, flag = backproject_host(fr, self._stride, self._near, self._far, self._edge)
        if flag:
            raise ValueError(f"{who}: {_NOT_FINITE}")
        cells = point_of
        if xyz.shape[0]:
            cell_of = self._insert(xyz, rgb, who).astype(np.int32)
            cells = np.where(point_of >= 0, cell_of[np.maximum(point_of, 0)], -1).astype(np.int32)
        self._sig = sig
        return torch.from_numpy(np.ascontiguousarray(cells))

    def add_points(self, xyz, rgb=None):
        """cells int32 [n]: n world points (float32 [n, 3], finite; rgb uint8 [n, 3] or None for black) added as add adds
        a chunk's valid pixels, in their order -- for points that come from somewhere else than a depth image."""
        who = self._who + ".add_points"
        xyz, rgb = _stream_points(xyz, rgb, who)
        if xyz.shape[0] == 0:
            return torch.zeros(0, dtype=torch.int32)
        return torch.from_numpy(self._insert(xyz, rgb, who).astype(np.int32))

    def snapshot(self, min_obs=1, cells=None, keep=None):
        who = self._who + ".snapshot"
        if int(min_obs) < 1:
            raise ValueError(f"{who}: min_obs = {min_obs} (>= 1)")
        M = self._keys.shape[0]
        cells = _cells_arg(cells, M, "cpu", who)
        mask = _keep_arg(keep, M, "cpu", who)
        if M == 0:
            return _empty((0, 0, 0) if cells is None else cells.shape, "cpu")
        o = self._origin.astype(np.float64)
        keep = self._count >= int(min_obs)
        if mask is not None:
            keep &= mask.numpy()
        new_id = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
        cnt = self._count[keep]
        mean = (self._sums[keep, :3].astype(np.float64) / cnt[:, None].astype(np.float64)) * (1.0 / UNITS)
        xyz_out = (o + mean).astype(np.float32)
        rgb_out = ((self._sums[keep, 3:] + (cnt // 2)[:, None]) // cnt[:, None]).astype(np.uint8)
        if cells is None:
            point_of = np.zeros((0, 0, 0), np.int32)
        else:
            c = cells.numpy()
            point_of = np.where(c >= 0, new_id[np.maximum(c, 0)], -1).astype(np.int32)
        return Fused(*(torch.from_numpy(np.ascontiguousarray(a)) for a in (xyz_out, rgb_out, cnt.astype(np.int32), point_of)))

    def kept(self, min_obs=1, keep=None):
        """int32 [m]: the cell number of every point of snapshot(min_obs, keep=keep), ascending -- the cells with
        count >= min_obs (and keep, when given)."""
        if int(min_obs) < 1:
            raise ValueError(f"{self._who}.kept: min_obs = {min_obs} (>= 1)")
        mask = _keep_arg(keep, self._keys.shape[0], "cpu", self._who + ".kept")
        on = self._count >= int(min_obs)
        if mask is not None:
            on &= mask.numpy()
        return torch.from_numpy(np.nonzero(on)[0].astype(np.int32))


class Fuser:
    """FuserHost's map on the GPU (csrc/frames_stream.hip): the same add, add_points, snapshot, origin, cells
    and pixels, bit-identical to the statement after every call and from run to run.  The state is torch tensors owned
    here: an open-addressing table (key, id, first) of `slots` entries, count int32 [capacity] and sums int64
    [capacity, 6].  Frames are moved to `device` per add, as fuse does; a chunk may differ from the one before in the
    number of frames only.

    add: gf_frames_backproject, gf_frames_map_insert (claim, rank, number), gf_frames_map_accumulate and
    gf_frames_map_lookup on the current stream; the words {n, not finite} of the back-projection and {M', invalid,
    overflow, beyond} of the insert are read back, the only synchronisations.  After a failed insert the table is
    rehashed (which drops what the insert claimed) before the ValueError is raised: the map is exactly as it was.
    snapshot: gf_frames_map_means, gf_frames_map_lookup; the words {m, accumulate's flag, a cell out of range} are read
    back once, the only synchronisation (the lookup checks every cell against the map's M as it reads it: a value
    below -1 or >= M is a ValueError).  With keep= (FuserHost's rule) gf_frames_map_means gets a copy of the counts
    with zeros at the dropped cells, which its count >= min_obs test refuses before anything is divided; the map itself
    is not touched.

    slots: the table's entries, a power of two.  None: the table starts at stream_slots' default and is doubled by
    gf_frames_map_rehash until slots >= 4 M' after an add; when an insert overflows it, the table is rehashed ONCE to
    the proven size >= 2 (M + n) and the insert run ONCE more.  A given `slots` is kept: overflowing it is a ValueError
    that names the proven size.  capacity: the initial rows of count and sums (they grow to at least double, zero
    filled, the used rows copied).  chunk: the elements one workgroup compacts (None: the default).  aggregate: whether
    adjacent lanes of one cell add up in the wave before the atomics (None: STREAM_AGGREGATE; the result is the same).
    rehashes, retries, row_growths count what their names say.  device "cpu": FuserHost."""

    def __init__(self, cell=0.02, stride=1, near=0.1, far=10.0, edge=None, origin=None, margin=STREAM_MARGIN, device="cuda",
                 slots=None, capacity=None, chunk=None, aggregate=None):
        self._who = who = "frames.Fuser"
        dev = torch.device(device)
        self._host = None
        self.rehashes = self.retries = self.row_growths = 0
        if dev.type != "cuda":
            self._host = FuserHost(cell, stride, near, far, edge, origin, margin)
            return
        self._cell, self._stride, self._origin, self._margin = _stream_args(cell, stride, edge, origin, margin, who)
        self._near, self._far, self._edge = near, far, edge
        self._chunk = _chunk(chunk, who)
        self._aggregate = int(STREAM_AGGREGATE if aggregate is None else aggregate)
        if slots is not None:
            s = int(slots)
            if not (STREAM_MIN_SLOTS <= s <= STREAM_MAX_SLOTS and s & (s - 1) == 0):
                raise ValueError(f"{who}: slots = {slots} (None, or a power of two from {STREAM_MIN_SLOTS} to {STREAM_MAX_SLOTS})")
        self._slots_arg = None if slots is None else int(slots)
        cap = 1024 if capacity is None else int(capacity)
        if cap < 1:
            raise ValueError(f"{who}: capacity = {capacity} (>= 1)")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        stream_limits()
        self._dev = dev
        self._sig = None
        self._M = self._pixels = 0
        self._org = None  # the origin on the device, float32 [3]
        self._keys = self._ids = self._first = None
        with torch.cuda.device(dev):
            self._count = torch.zeros(cap, dtype=torch.int32, device=dev)
            self._sums = torch.zeros((cap, 6), dtype=torch.int64, device=dev)
            # {m of the last snapshot, accumulate's flag (only ever set), the last snapshot's "a cell out of range"}
            self._words = torch.zeros(3, dtype=torch.int32, device=dev)

    @property
    def origin(self):
        """float32 [3], or None before the first add with a valid pixel."""
        if self._host is not None:
            return self._host.origin
        if self._origin is None and self._org is not None:
            self._origin = self._org.cpu().numpy()
        return None if self._origin is None else self._origin.copy()

    cells = property(lambda self: self._host.cells if self._host is not None else self._M, doc="the cells of the map")
    pixels = property(lambda self: self._host.pixels if self._host is not None else self._pixels,
                      doc="the valid pixels added so far")
    slots = property(lambda self: None if self._host is not None or self._keys is None else int(self._keys.shape[0]),
                     doc="the table's entries (None before the first add with a valid pixel)")
    capacity = property(lambda self: None if self._host is not None else int(self._count.shape[0]),
                        doc="the rows of count and sums")

    def state(self):
        """FuserHost.state() of this map: (keys int64 [M], count int64 [M], sums int64 [M, 6]) in cell order, read from
        the table's numbered slots."""
        if self._host is not None:
            return self._host.state()
        M = self._M
        keys = np.zeros(M, np.int64)
        if M:
            ids = self._ids.cpu().numpy()
            on = ids >= 0
            if int(on.sum()) != M or not (np.sort(ids[on]) == np.arange(M)).all():
                raise RuntimeError(f"{self._who}: the table's numbered slots are not the map's {M} cells")
            keys[ids[on]] = self._keys.cpu().numpy()[on]
        return keys, self._count[:M].cpu().numpy().astype(np.int64), self._sums[:M].cpu().numpy()

    def _rehash(self, new_slots):
        """The table moved into a cleared one of new_slots entries (numbered slots only; ids untouched)."""
        from . import _lib
        from ._lib import check, ptr, stream_ptr

        dev, old = self._dev, self._keys
        keys = torch.empty(new_slots, dtype=torch.int64, device=dev)
        ids = torch.empty((2, new_slots), dtype=torch.int32, device=dev)
        check(_lib.load().gf_frames_map_rehash(ptr(old), ptr(self._ids), 0 if old is None else old.shape[0], self._M, ptr(keys),
                                               ptr(ids[0]), ptr(ids[1]), new_slots, stream_ptr()), "gf_frames_map_rehash")
        self._keys, self._ids, self._first = keys, ids[0], ids[1]
        self.rehashes += old is not None

    def _insert(self, xyz, rgb, lo, who):
        """cell_of int32 [n] (device) of n >= 1 points on the device; the map changes only when every check has passed."""
        from . import _lib
        from ._lib import check, ptr, stream_ptr

        lib = _lib.load()
        dev, n, M = self._dev, xyz.shape[0], self._M
        _stream_budget(self._pixels, n, who)
        if self._org is not None:
            org = self._org
        elif self._origin is not None:
            org = torch.from_numpy(self._origin).to(dev)
        else:
            org = torch.sub(lo, torch.full((3,), float(self._margin), dtype=torch.float32, device=dev))
        default, proven = stream_slots(M, n)
        if self._keys is None:
            self._rehash(default if self._slots_arg is None else self._slots_arg)
        elif self._slots_arg is None and self._keys.shape[0] < default:
            self._rehash(default)
        cell_of = torch.empty(n, dtype=torch.int32, device=dev)
        words = torch.empty(4, dtype=torch.int32, device=dev)
        ws = torch.empty(lib.gf_frames_map_insert_scratch_bytes(n, self._chunk) // 8 + 1, dtype=torch.int64, device=dev)
        for attempt in (0, 1):
            slots = self._keys.shape[0]
            check(lib.gf_frames_map_insert(ptr(xyz), n, float(self._cell), ptr(org), ptr(self._keys), ptr(self._ids),
                                           ptr(self._first), slots, M, self._chunk, ptr(ws), ptr(cell_of), ptr(words),
                                           stream_ptr()), "gf_frames_map_insert")
            M2, invalid, overflow, beyond = words.tolist()
            if not (invalid or overflow or beyond):
                break
            if invalid or beyond or self._slots_arg is not None or attempt or proven > STREAM_MAX_SLOTS:
                self._rehash(slots)  # drops what the failed insert claimed (M <= slots: every cell holds a slot)
                if invalid:
                    raise ValueError(f"{who}: {_BELOW}")
                if beyond:
                    raise ValueError(f"{who}: {_STREAM_BEYOND}")
                if attempt:
                    raise RuntimeError(f"{who}: a table of {slots} >= 2 (M + n) slots overflowed")  # (proven impossible)
                raise ValueError(f"{who}: the table of slots = {slots} overflowed; {proven} slots are always enough for "
                                 f"{M} cells and {n} more points")
            self._rehash(proven)
            self.retries += 1
        cap = self._count.shape[0]
        if M2 > cap:
            cap = max(2 * cap, M2)
            count = torch.zeros(cap, dtype=torch.int32, device=dev)
            sums = torch.zeros((cap, 6), dtype=torch.int64, device=dev)
            count[:M] = self._count[:M]
            sums[:M] = self._sums[:M]
            self._count, self._sums = count, sums
            self.row_growths += 1
        check(lib.gf_frames_map_accumulate(ptr(xyz), ptr(rgb), ptr(cell_of), n, M2, ptr(org), self._aggregate, ptr(self._count),
                                           ptr(self._sums), ptr(self._words[1:2]), stream_ptr()), "gf_frames_map_accumulate")
        self._org, self._M, self._pixels = org, M2, self._pixels + n
        if self._slots_arg is None:
            slots = self._keys.shape[0]
            while slots < 4 * M2 and slots < STREAM_MAX_SLOTS:
                slots <<= 1
            if slots != self._keys.shape[0]:
                self._rehash(slots)
        return cell_of

    def add(self, fr):
        if self._host is not None:
            return self._host.add(fr)
        from . import _lib
        from ._lib import check, ptr, stream_ptr

        who = self._who + ".add"
        sig = _stream_sig(fr, self._sig, who)
        _args(fr, self._stride, self._near, self._far, self._edge, who)
        dev = self._dev
        if fr.depth.device != dev:
            fr = fr._replace(depth=fr.depth.to(dev), color=None if fr.color is None else fr.color.to(dev))
        with torch.cuda.device(dev):
            xyz, rgb, _, point_of, lo = backproject(fr, self._stride, self._near, self._far, self._edge, self._chunk or None,
                                                    return_origin=True)
            if xyz.shape[0]:
                cell_of = self._insert(xyz.contiguous(), rgb.contiguous(), lo, who)
                check(_lib.load().gf_frames_map_lookup(ptr(point_of), point_of.numel(), ptr(cell_of), cell_of.shape[0],
                                                       ptr(point_of), None, stream_ptr()), "gf_frames_map_lookup")
        self._sig = sig
        return point_of

    def add_points(self, xyz, rgb=None):
        """FuserHost.add_points on the device: cells int32 [n]."""
        if self._host is not None:
            return self._host.add_points(xyz, rgb)
        who = self._who + ".add_points"
        xyz, rgb = _stream_points(xyz, rgb, who)
        dev = self._dev
        if xyz.shape[0] == 0:
            return torch.zeros(0, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            # (a tensor wants writable memory)
            up = lambda a: torch.from_numpy(a if a.flags.writeable else a.copy()).to(dev)  # noqa: E731
            x = up(xyz)
            return self._insert(x, up(rgb), x.min(0).values, who)

    def snapshot(self, min_obs=1, cells=None, keep=None):
        if self._host is not None:
            return self._host.snapshot(min_obs, cells, keep)
        from . import _lib
        from ._lib import check, ptr, stream_ptr

        who = self._who + ".snapshot"
        if int(min_obs) < 1:
            raise ValueError(f"{who}: min_obs = {min_obs} (>= 1)")
        lib = _lib.load()
        dev, M = self._dev, self._M
        with torch.cuda.device(dev):
            cells = _cells_arg(cells, M, dev, who)
            mask = _keep_arg(keep, M, dev, who)
            if M == 0:
                return _empty((0, 0, 0) if cells is None else cells.shape, dev)
            count = self._count
            if mask is not None:  # a dropped cell's count reads 0 < min_obs: FmKept refuses it before anything is divided
                count = torch.where(mask, count[:M], torch.zeros((), dtype=torch.int32, device=dev))
            xyz_out = torch.empty((M, 3), dtype=torch.float32, device=dev)
            rgb_out = torch.empty((M, 3), dtype=torch.uint8, device=dev)
            out_i = torch.empty((2, M), dtype=torch.int32, device=dev)
            ws = torch.empty(lib.gf_frames_map_means_scratch_bytes(M, self._chunk) // 8 + 1, dtype=torch.int64, device=dev)
            check(lib.gf_frames_map_means(ptr(count), ptr(self._sums), M, ptr(self._org), int(min_obs), self._chunk, ptr(ws),
                                          ptr(xyz_out), ptr(rgb_out), ptr(out_i[0]), ptr(out_i[1]), ptr(self._words),
                                          stream_ptr()), "gf_frames_map_means")
            if cells is None:
                point_of = torch.zeros((0, 0, 0), dtype=torch.int32, device=dev)
            else:
                point_of = torch.empty_like(cells)
                self._words[2:].zero_()
                check(lib.gf_frames_map_lookup(ptr(cells), cells.numel(), ptr(out_i[1]), M, ptr(point_of), ptr(self._words[2:]),
                                               stream_ptr()), "gf_frames_map_lookup")
            m, late, outside = self._words.tolist()
        if cells is not None and outside:
            raise ValueError(f"{who}: {_CELLS_RANGE} {M} cells")
        if late:  # (the insert's claim pass makes the same comparison first: proven impossible)
            raise RuntimeError(f"{who}: an accumulate met a point beyond the map's reach")
        return Fused(xyz_out[:m], rgb_out[:m], out_i[0, :m], point_of)

    def kept(self, min_obs=1, keep=None):
        """FuserHost.kept on the device: int32 [m], a torch reduction over the M counts (nothing of the map is read back
        but m, the length of the result)."""
        if self._host is not None:
            return self._host.kept(min_obs, keep)
        if int(min_obs) < 1:
            raise ValueError(f"{self._who}.kept: min_obs = {min_obs} (>= 1)")
        with torch.cuda.device(self._dev):
            mask = _keep_arg(keep, self._M, self._dev, self._who + ".kept")
            on = self._count[:self._M] >= int(min_obs)
            if mask is not None:
                on = on & mask
            return torch.nonzero(on).reshape(-1).to(torch.int32)


# ---- votes that persist between calls: labels lifted chunk by chunk ---------------------------------------------------
def voter_slots(P, T):
    """(default, proven) table sizes of a voter of P stored pairs before an add of T elements: the smallest power of two
    at or above max(4 P, T / 8) (gf_frames_votes_default_slots; at most VOTER_MAX_SLOTS) and at or above 2 (P + T), which
    no input overflows; both at least 64."""
    def pow2(v):
        p = VOTER_MIN_SLOTS
        while p < v:
            p <<= 1
        return p

    return min(pow2(max(4 * int(P), int(T) // 8)), VOTER_MAX_SLOTS), pow2(2 * (int(P) + int(T)))


def voter_limits():
    """(probes, elements) of the library's persistent vote, asserted against this module's constants."""
    from . import _lib

    lib = _lib.load()
    got = (lib.gf_frames_votes_max_probes(), lib.gf_frames_votes_max_elements())
    if got != (VOTER_MAX_PROBES, VOTER_MAX_ELEMENTS) or lib.gf_resample_max_points() != MAX_POINTS:
        raise RuntimeError(f"frames: the library's voter limits {got} are not this module's")
    return got


def _voter_add_args(group, value, stride, elements, who):
    """(group, value, F, H, W, stride, T) of an add: tensors as given (any device), every check of shape, dtype and the
    element budget made."""
    def h(a):  # (a read-only or strided array is copied: a tensor wants writable, contiguous memory)
        return a if torch.is_tensor(a) else torch.from_numpy(a if a.flags.writeable and a.flags.c_contiguous else np.array(a, order="C"))

    if not (torch.is_tensor(group) or isinstance(group, np.ndarray)) or not (torch.is_tensor(value) or isinstance(value, np.ndarray)):
        raise ValueError(f"{who}: group and value: numpy arrays or torch tensors")
    group, value = h(group), h(value)
    if group.dtype != torch.int32:
        raise ValueError(f"{who}: group: expected int32, got {group.dtype}")
    if value.dtype not in _VALUE_KINDS:
        raise ValueError(f"{who}: value: expected uint8, uint16 or int32, got {value.dtype}")
    s = 1 if stride is None else int(stride)
    if s < 1:
        raise ValueError(f"{who}: stride = {stride} (>= 1)")
    if s == 1:
        if tuple(group.shape) != tuple(value.shape):
            raise ValueError(f"{who}: group {tuple(group.shape)} and value {tuple(value.shape)} differ in shape")
        F, H, W = 1, 1, group.numel()
    else:
        if group.dim() != 3 or value.dim() != 3 or value.shape[0] != group.shape[0] or \
                (-(-value.shape[1] // s), -(-value.shape[2] // s)) != tuple(group.shape[1:]):
            raise ValueError(f"{who}: value {tuple(value.shape)} at stride {s} does not sample to group's {tuple(group.shape)}")
        F, H, W = (int(d) for d in value.shape)
    T = group.numel()
    if T > MAX_POINTS:
        raise ValueError(f"{who}: {T} elements in one add (at most {MAX_POINTS})")
    if elements + T > VOTER_MAX_ELEMENTS:
        raise ValueError(f"{who}: {elements} elements so far and {T} more: a voter takes at most {VOTER_MAX_ELEMENTS}")
    return group, value, F, H, W, s, T


def _voter_init_args(ignore, who):
    if ignore is not None and int(ignore) != ignore:
        raise ValueError(f"{who}: ignore must be None or an integer, got {ignore!r}")
    return None if ignore is None else int(ignore)


def _voter_snapshot_args(n, fill, rows, who):
    n = int(n)
    if not 0 <= n <= VOTER_MAX_GROUPS:
        raise ValueError(f"{who}: n = {n} groups (0 to {VOTER_MAX_GROUPS})")
    if not -2 ** 31 <= int(fill) < 2 ** 31:
        raise ValueError(f"{who}: fill = {fill} is no int32")
    if rows is not None:
        rows = rows if torch.is_tensor(rows) else torch.from_numpy(np.ascontiguousarray(rows))
        if rows.dtype != torch.int32 or rows.dim() != 1:
            raise ValueError(f"{who}: rows: expected int32 [m], got {rows.dtype} {tuple(rows.shape)}")
    return n, int(fill), rows


_ROWS_RANGE = "rows holds a value outside the"


class VoterHost:
    """The statement of Voter, in numpy: the multiset of (group, value) pairs seen so far with an integer count each, for
    one `ignore` (an int or None, as in vote_host) fixed at construction.

    add(group, value, stride=None): lift's shapes -- group int32 [F, Hs, Ws] (what Fuser.add returns) with value uint8,
    uint16 or int32 [F, H, W] read at the pixels (j0 stride, i0 stride) -- or, without a stride, group and value of one
    equal shape.  Element t votes when group[t] >= 0, value[t] >= 0 and value[t] != ignore: vote_host's test without the
    upper bound on the group.  The value dtype may differ from one add to the next.  At most MAX_POINTS elements per add
    and VOTER_MAX_ELEMENTS in all, counted as offered; a failed add leaves the voter exactly as it was.

    snapshot(n, fill=IGNORE_LABEL, rows=None) -> (Lifted of CPU tensors, pairs): vote_host's second half on the stored
    counts, per group 0 <= g < n: total = the group's votes; the value with the largest count wins, ties go to the
    smallest value; a group without a vote gets fill and 0 votes.  pairs: the distinct stored pairs.  A stored pair with
    group >= n is a ValueError.  rows: int32 [m] with values in [0, n) (anything else is a ValueError): the groups
    reported, in that order.  Changes nothing.

    For adds (g1, v1) .. (gk, vk), snapshot(n, fill) equals vote_host(cat(g_i).ravel(), cat(sampled v_i).ravel(), n,
    ignore, fill) in every field and in pairs, as bits."""

    def __init__(self, ignore=None):
        self._who = "frames." + type(self).__name__
        self._ignore = _voter_init_args(ignore, self._who)
        self._keys = np.zeros(0, np.int64)
        self._count = np.zeros(0, np.int64)
        self._elements = 0

    pairs = property(lambda self: int(self._keys.shape[0]), doc="the distinct (group, value) pairs stored")
    elements = property(lambda self: self._elements, doc="the elements offered so far, voting or not")

    def state(self):
        """(keys int64 [P] ascending, count int64 [P]) with key = group << 32 | value, copies."""
        return self._keys.copy(), self._count.copy()

    def add(self, group, value, stride=None):
        who = self._who + ".add"
        group, value, F, H, W, s, T = _voter_add_args(group, value, stride, self._elements, who)
        g = group.detach().cpu().numpy().reshape(-1).astype(np.int64)
        v = value.detach().cpu().numpy()
        v = (v[:, ::s, ::s] if s != 1 else v).reshape(-1).astype(np.int64)
        on = (g >= 0) & (v >= 0)
        if self._ignore is not None:
            on &= v != self._ignore
        keys, inv = np.unique(np.concatenate([self._keys, (g[on] << 32) | v[on]]), return_inverse=True)
        count = np.zeros(keys.shape[0], np.int64)
        np.add.at(count, inv.reshape(-1), np.concatenate([self._count, np.ones(int(on.sum()), np.int64)]))
        self._keys, self._count, self._elements = keys, count, self._elements + T

    def snapshot(self, n, fill=IGNORE_LABEL, rows=None):
        who = self._who + ".snapshot"
        n, fill, rows = _voter_snapshot_args(n, fill, rows, who)
        pg, pv = self._keys >> 32, self._keys & 0xffffffff
        if pg.size and int(pg.max()) >= n:
            raise ValueError(f"{who}: a stored group is {int(pg.max())}, outside the {n} groups")
        total = np.zeros(n, np.int64)
        np.add.at(total, pg, self._count)
        best = np.zeros(n, np.int64)  # count << 32 | (0xffffffff - value): the largest count, then the smallest value
        np.maximum.at(best, pg, (self._count << 32) | (0xffffffff - pv))
        label = np.where(best > 0, 0xffffffff - (best & 0xffffffff), fill)
        out = [a.astype(np.int32) for a in (label, best >> 32, total)]
        if rows is not None:
            r = rows.detach().cpu().numpy()
            if r.size and not (int(r.min()) >= 0 and int(r.max()) < n):
                raise ValueError(f"{who}: {_ROWS_RANGE} {n} groups")
            out = [a[r] for a in out]
        return Lifted(*(torch.from_numpy(np.ascontiguousarray(a)) for a in out)), self.pairs


class Voter:
    """VoterHost's votes on the GPU (csrc/frames_vote_stream.hip): the same add, snapshot, state, pairs and
    elements, bit-identical to the statement after every call and from run to run.  The state is two torch tensors owned
    here: an open-addressing table of `slots` entries, keys (group << 32 | value, all ones = empty) and counts.  group
    and value are moved to `device` per add when they are on the host; a tensor on another GPU is a ValueError.

    add: gf_frames_votes_add on the current stream (claim, then commit); the two words {new pairs, overflow} are read
    back once, the only synchronisation.  An add that overflows its table has changed no count; the table is rehashed
    (which drops the keys it claimed) before anything else happens, so a failed add leaves no trace.
    snapshot: gf_frames_votes_pick and, with rows=, three gathers; {pairs, group out of range, rows out of range} are
    read back once.

    slots: the table's entries, a power of two.  None: the table starts at voter_slots' default and is doubled by
    gf_frames_votes_rehash until slots >= 4 P' after an add; when an add overflows it, the table is rehashed ONCE to the
    proven size >= 2 (P + T) and the add run ONCE more.  A given `slots` is kept: overflowing it is a ValueError that
    names the proven size, raised after the cleaning rehash; so is a proven size above VOTER_MAX_SLOTS.  aggregate:
    whether adjacent lanes of one pair record one add (None: VOTER_AGGREGATE; the result is the same).  rehashes and
    retries count what their names say.  device "cpu": VoterHost."""

    def __init__(self, ignore=None, device="cuda", slots=None, aggregate=None):
        self._who = who = "frames.Voter"
        dev = torch.device(device)
        self._host = None
        self.rehashes = self.retries = 0
        if dev.type != "cuda":
            self._host = VoterHost(ignore)
            return
        self._ignore = _voter_init_args(ignore, who)
        self._aggregate = int(VOTER_AGGREGATE if aggregate is None else aggregate)
        if slots is not None:
            s = int(slots)
            if not (VOTER_MIN_SLOTS <= s <= VOTER_MAX_SLOTS and s & (s - 1) == 0):
                raise ValueError(f"{who}: slots = {slots} (None, or a power of two from {VOTER_MIN_SLOTS} to {VOTER_MAX_SLOTS})")
        self._slots_arg = None if slots is None else int(slots)
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        voter_limits()
        self._dev = dev
        self._keys = self._cnt = None  # int64 / int32 [slots]: the bits of the library's uint64 / uint32
        self._pairs = self._elements = 0

    pairs = property(lambda self: self._host.pairs if self._host is not None else self._pairs,
                     doc="the distinct (group, value) pairs stored")
    elements = property(lambda self: self._host.elements if self._host is not None else self._elements,
                        doc="the elements offered so far, voting or not")
    slots = property(lambda self: None if self._host is not None or self._keys is None else int(self._keys.shape[0]),
                     doc="the table's entries (None before the first add with an element)")

    def state(self):
        """VoterHost.state() of these votes: (keys int64 [P] ascending, count int64 [P]), read from the table's slots
        that hold a count."""
        if self._host is not None:
            return self._host.state()
        if self._keys is None:
            return np.zeros(0, np.int64), np.zeros(0, np.int64)
        keys, cnt = self._keys.cpu().numpy(), self._cnt.cpu().numpy().astype(np.int64)
        on = (keys != -1) & (cnt > 0)
        if int(on.sum()) != self._pairs:
            raise RuntimeError(f"{self._who}: the table holds {int(on.sum())} counted pairs, not the voter's {self._pairs}")
        order = np.argsort(keys[on], kind="stable")
        return keys[on][order], cnt[on][order]

    def _rehash(self, new_slots):
        """The table moved into a cleared one of new_slots entries (slots with a count only)."""
        from . import _lib
        from ._lib import check, ptr, stream_ptr

        dev, old = self._dev, self._keys
        keys = torch.empty(new_slots, dtype=torch.int64, device=dev)
        cnt = torch.empty(new_slots, dtype=torch.int32, device=dev)
        check(_lib.load().gf_frames_votes_rehash(ptr(old), ptr(self._cnt), 0 if old is None else old.shape[0], self._pairs,
                                                 ptr(keys), ptr(cnt), new_slots, stream_ptr()), "gf_frames_votes_rehash")
        self._keys, self._cnt = keys, cnt
        self.rehashes += old is not None

    def add(self, group, value, stride=None):
        if self._host is not None:
            return self._host.add(group, value, stride)
        from . import _lib
        from ._lib import check, ptr, stream_ptr

        who = self._who + ".add"
        group, value, F, H, W, s, T = _voter_add_args(group, value, stride, self._elements, who)
        dev, P = self._dev, self._pairs
        for t, name in ((group, "group"), (value, "value")):
            if t.is_cuda and t.device != dev:
                raise ValueError(f"{who}: {name} on {t.device}, the voter on {dev}")
        if T == 0:
            return
        lib = _lib.load()
        default, proven = voter_slots(P, T)
        has = self._ignore is not None and -2 ** 31 <= self._ignore < 2 ** 31  # (no value is another int)
        with torch.cuda.device(dev):
            group, value = group.to(dev).contiguous(), value.to(dev).contiguous()
            if self._keys is None:
                self._rehash(default if self._slots_arg is None else self._slots_arg)
            elif self._slots_arg is None and self._keys.shape[0] < default:
                self._rehash(default)
            words = torch.empty(2, dtype=torch.int32, device=dev)
            ws = torch.empty(lib.gf_frames_votes_add_scratch_bytes(T) // 8 + 1, dtype=torch.int64, device=dev)
            for attempt in (0, 1):
                slots = self._keys.shape[0]
                check(lib.gf_frames_votes_add(ptr(group), ptr(value), _VALUE_KINDS[value.dtype], F, W, H, s,
                                              self._ignore if has else 0, int(has), ptr(self._keys), ptr(self._cnt), slots, P,
                                              self._aggregate, ptr(ws), ptr(words), stream_ptr()), "gf_frames_votes_add")
                new, overflow = words.tolist()
                if not overflow:
                    break
                if self._slots_arg is not None or attempt or proven > VOTER_MAX_SLOTS:
                    self._rehash(slots)  # drops what the failed add claimed (P <= slots: every pair holds a slot)
                    if attempt:
                        raise RuntimeError(f"{who}: a table of {slots} >= 2 (P + T) slots overflowed")  # (proven impossible)
                    raise ValueError(f"{who}: the table of slots = {slots} overflowed; {proven} slots are always enough for "
                                     f"{P} pairs and {T} more elements" +
                                     (f", above the largest table of {VOTER_MAX_SLOTS}" if proven > VOTER_MAX_SLOTS else ""))
                self._rehash(proven)
                self.retries += 1
            self._pairs, self._elements = P + new, self._elements + T
            if self._slots_arg is None:
                slots = self._keys.shape[0]
                while slots < 4 * self._pairs and slots < VOTER_MAX_SLOTS:
                    slots <<= 1
                if slots != self._keys.shape[0]:
                    self._rehash(slots)

    def snapshot(self, n, fill=IGNORE_LABEL, rows=None):
        if self._host is not None:
            return self._host.snapshot(n, fill, rows)
        from . import _lib
        from ._lib import check, ptr, stream_ptr

        who = self._who + ".snapshot"
        n, fill, rows = _voter_snapshot_args(n, fill, rows, who)
        lib = _lib.load()
        dev = self._dev
        if rows is not None and rows.is_cuda and rows.device != dev:
            raise ValueError(f"{who}: rows on {rows.device}, the voter on {dev}")
        if rows is not None and not rows.is_cuda and rows.numel() and not (int(rows.min()) >= 0 and int(rows.max()) < n):
            raise ValueError(f"{who}: {_ROWS_RANGE} {n} groups")
        with torch.cuda.device(dev):
            out = torch.empty((3, n), dtype=torch.int32, device=dev)
            if n == 0 or self._keys is None:
                if self._pairs:
                    raise ValueError(f"{who}: a stored group is outside the {n} groups")
                out[0] = fill
                out[1:] = 0
                words = torch.zeros(2, dtype=torch.int32, device=dev)
            else:
                words = torch.empty(2, dtype=torch.int32, device=dev)
                ws = torch.empty(lib.gf_frames_votes_pick_scratch_bytes(n) // 8 + 1, dtype=torch.int64, device=dev)
                check(lib.gf_frames_votes_pick(ptr(self._keys), ptr(self._cnt), self._keys.shape[0], n, fill, ptr(ws),
                                               ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(words), stream_ptr()),
                      "gf_frames_votes_pick")
            if rows is not None:
                rows = rows.to(dev)
                bad = ((rows < 0) | (rows >= n)).any().to(torch.int32).reshape(1)
                out = out[:, rows.clamp(0, max(n - 1, 0)).long()] if n else out[:, :0]
                pairs, beyond, outside = torch.cat([words, bad]).tolist()  # the one read-back
            else:
                (pairs, beyond), outside = words.tolist(), 0
        if beyond:
            raise ValueError(f"{who}: a stored group is outside the {n} groups")
        if outside:
            raise ValueError(f"{who}: {_ROWS_RANGE} {n} groups")
        if pairs != self._pairs:
            raise RuntimeError(f"{who}: the table holds {pairs} counted pairs, not the voter's {self._pairs}")
        return Lifted(out[0], out[1], out[2]), pairs


def lift_scene_stream(fuser, sem_voter, ins_voter, min_obs=1, min_votes=1, min_share=None, keep=None):
    """(semantic int32 [m], instance int32 [m]) of the points of fuser.snapshot(min_obs): scene_labels of the two voters'
    snapshots over fuser.kept(min_obs).  sem_voter and ins_voter were fed every chunk's cells (what fuser.add returned)
    with its label and its instance images.  Equal, as bits, to lift_scene(fuser.snapshot(min_obs, all cells), all label
    images, all instance images, ...) -- with nothing kept but the map and the two tables.  keep: the points are those of
    fuser.snapshot(min_obs, keep=keep) (a Carver's keep(): bool or uint8 [fuser.cells])."""
    if not isinstance(fuser, (Fuser, FuserHost)) or not all(isinstance(v, (Voter, VoterHost)) for v in (sem_voter, ins_voter)):
        raise ValueError("frames.lift_scene_stream: expected a Fuser and two Voters (or their host statements)")
    rows, n = fuser.kept(min_obs, keep), fuser.cells
    sem = sem_voter.snapshot(n, IGNORE_LABEL, rows)[0]
    ins = ins_voter.snapshot(n, IGNORE_LABEL, rows)[0]
    return scene_labels(sem, ins, min_votes, min_share, host=not sem.label.is_cuda)


# ---- instance ids that persist between model runs on successive snapshots ----------------------------------------------
class TrackTable(NamedTuple):
    """One entry per track, ids 0 .. T - 1 (never reused): cls int32 and score fp32 of the best-scored sighting (the
    later one on a tie), born / seen int32 (the update index of the first and the last match), hits int32 (matches),
    misses int32 (consecutive updates that saw its cells and did not match it), size int32 (cells of the map that are
    this track's; 0 once retired) and alive bool."""
    cls: object
    score: object
    born: object
    seen: object
    hits: object
    misses: object
    size: object
    alive: object


class Tracked(NamedTuple):
    """What an update returns: ids int32 [m] (the map at `cells` after the update, -1 for no track or a retired one),
    track int32 [p] (the row's track id, -1 for a row without one), matched bool [p] (the row continued a track), new
    and retired int32 [.] (the ids of the tracks born and retired by this update, ascending)."""
    ids: object
    track: object
    matched: object
    new: object
    retired: object


def tracker_slots(p, live, m):
    """(default, proven) pair-table sizes of an update of p rows and m points against `live` alive tracks: the smallest
    power of two at or above 8 (p + live) (gf_frames_track_default_slots) and at or above 2 m, which no input overflows;
    both at least 64.  An update starts at the smaller of the two."""
    def pow2(v):
        s = TRACK_MIN_SLOTS
        while s < v and s < TRACK_MAX_SLOTS:
            s <<= 1
        return s

    return pow2(8 * (int(p) + int(live))), pow2(2 * int(m))


def tracker_limits():
    """(rows, probes, tracks) of the library's tracker, asserted against this module's constants."""
    from . import _lib

    lib = _lib.load()
    got = (lib.gf_frames_track_max_rows(), lib.gf_frames_track_max_probes(), lib.gf_frames_track_max_tracks())
    if got != (TRACK_MAX_ROWS, TRACK_MAX_PROBES, TRACK_MAX_TRACKS) or lib.gf_resample_max_points() != MAX_POINTS or \
            lib.gf_frames_track_columns() != len(TrackTable._fields) or lib.gf_frames_track_words() != _TRACK_WORDS:
        raise RuntimeError(f"frames: the library's tracker limits {got} are not this module's")
    return got


def _tracker_init_args(iou, max_misses, min_points, same_class, who):
    iou = float(iou)
    if not 0.0 <= iou <= 1.0:
        raise ValueError(f"{who}: iou = {iou} (0 to 1)")
    if int(max_misses) != max_misses or int(max_misses) < 0 or int(max_misses) >= 2 ** 31 - 1:
        raise ValueError(f"{who}: max_misses = {max_misses!r} (an integer >= 0)")
    if int(min_points) != min_points or not 1 <= int(min_points) < 2 ** 31:
        raise ValueError(f"{who}: min_points = {min_points!r} (an integer >= 1)")
    return iou, int(max_misses), int(min_points), bool(same_class)


_CELLS_ASCEND = "cells must be non-negative and strictly ascending (what Fuser.kept returns)"
_OWNER_RANGE = "owner holds a value outside -1 .."


def _tracker_update_args(cells, owner, cls, score, keep, T, who):
    """(cells, owner, cls, score, keep) of an update as torch tensors (any device) of int32 [m], int32 [m], int32 [p],
    fp32 [p], bool [p]: every check of shape and dtype made, and of the values of whatever is on the host."""
    def h(a, name):
        if torch.is_tensor(a):
            return a.detach()
        if isinstance(a, np.ndarray):
            return torch.from_numpy(a if a.flags.writeable and a.flags.c_contiguous else np.array(a, order="C"))
        raise ValueError(f"{who}: {name}: expected a numpy array or a torch tensor, got {type(a).__name__}")

    cells, owner, cls, score = h(cells, "cells"), h(owner, "owner"), h(cls, "cls"), h(score, "score")
    for t, name in ((cells, "cells"), (owner, "owner")):
        if t.dtype != torch.int32 or t.dim() != 1:
            raise ValueError(f"{who}: {name}: expected int32 [m], got {t.dtype} {tuple(t.shape)}")
    m = cells.shape[0]
    if owner.shape[0] != m:
        raise ValueError(f"{who}: {m} cells and {owner.shape[0]} owners")
    if m > MAX_POINTS:
        raise ValueError(f"{who}: {m} points in one update (at most {MAX_POINTS})")
    if cls.dim() != 1 or cls.dtype not in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64):
        raise ValueError(f"{who}: cls: expected integers [p], got {cls.dtype} {tuple(cls.shape)}")
    p = cls.shape[0]
    if score.dtype != torch.float32 or tuple(score.shape) != (p,):
        raise ValueError(f"{who}: score: expected float32 [{p}], got {score.dtype} {tuple(score.shape)}")
    if keep is None:
        keep = torch.ones(p, dtype=torch.bool, device=score.device)
    else:
        keep = h(keep, "keep")
        if keep.dtype != torch.bool or tuple(keep.shape) != (p,):
            raise ValueError(f"{who}: keep: expected bool [{p}], got {keep.dtype} {tuple(keep.shape)}")
    if p > TRACK_MAX_ROWS:
        raise ValueError(f"{who}: {p} rows in one update (at most {TRACK_MAX_ROWS})")
    if T + p > TRACK_MAX_TRACKS:
        raise ValueError(f"{who}: {T} tracks so far and {p} rows: a tracker holds at most {TRACK_MAX_TRACKS} tracks")
    if not cls.is_cuda and p and not (-2 ** 31 <= int(cls.min()) and int(cls.max()) < 2 ** 31):
        raise ValueError(f"{who}: cls holds a value that is no int32")
    if not cells.is_cuda and m:
        c = cells.numpy()
        if int(c[0]) < 0 or (m > 1 and not (c[1:] > c[:-1]).all()):
            raise ValueError(f"{who}: {_CELLS_ASCEND}")
    if not owner.is_cuda and m and not (int(owner.min()) >= -1 and int(owner.max()) < p):
        raise ValueError(f"{who}: {_OWNER_RANGE} {p - 1}")
    return cells, owner, cls.to(torch.int32), score, keep


class TrackerHost:
    """The statement of Tracker, in numpy: instance ids that persist over successive model runs on the snapshots of one
    Fuser, keyed by its persistent cell numbers.

    State after u updates: M cells with track_of int32 [M] (-1: none) and T tracks, ids 0 .. T - 1, never reused, with
    the columns of TrackTable.

    update(cells, owner, cls, score, keep=None) -> Tracked.  cells int32 [m], non-negative and strictly ascending (what
    fuser.kept(min_obs) returns): point i of the snapshot is cell cells[i].  owner int32 [m] in [-1, p): the row of this
    run that owns the point (SceneLabels.owner).  cls integers [p], score fp32 [p], keep bool [p] (default all true).
      0. the map is extended to M' = max(M, cells[-1] + 1) cells, new ones -1;
      1. r_i = owner[i] when it is >= 0 and kept, else -1; t_i = track_of[cells[i]] when the cell is < M and that track
         alive, else -1; a[r], b[t], n[r, t] count the points with that row, that track, and both;
      2. best_row[r]: among the t with n[r, t] > 0 (and cls equal when same_class) the one of the largest IoU
         n / (a[r] + b[t] - n), compared exactly (cross-multiplied integers), a tie to the smaller t; best_track[t]
         likewise over r, a tie to the smaller r; (r, t) match when each is the other's best and
         float64(n) >= iou * float64(union): one to one, so the threshold alone cannot glue two objects together;
      3. a matched row takes its track's id; the other kept rows with a[r] >= min_points get new ids T, T + 1, .. in
         ascending r; every other row gets -1 and its points count as unowned;
      4. a matched track: hits + 1, misses 0, seen = u, and when score[r] >= its score (fp32) it takes the row's score and
         cls; a new track: born = seen = u, hits 1; an alive unmatched track with b[t] > 0 (it was in view): misses + 1,
         retired when misses > max_misses; a track with b[t] == 0 is untouched (a partial update leaves the rest alone);
      5. point by point, with tid the row's id: tid >= 0 sets track_of[c] = tid; else a cell whose old track matched or
         retired in this update is set to -1; else the cell is unchanged (a track that was merely missed holds its
         cells).  size follows; a retired track has size 0 and its remaining cells read as -1; after the pass an alive
         track with size 0 is retired too.
    A failed update (a ValueError) changes nothing.

    labels(cells) reads the map (int32, any shape, -1 allowed and answered by -1; a value from M on is a ValueError);
    table() is the TrackTable; state() is (track_of [M] with retired tracks as -1, table) as numpy copies.

    The defaults (iou 0.3, max_misses 2, min_points 1, same_class False) are chosen by reasoning -- a half-seen object is
    often misclassified, and its identity should survive the class flipping --; their effect on a tracking metric is NOT
    measured: there is no trained checkpoint and no sequence ground truth here."""

    def __init__(self, iou=0.3, max_misses=2, min_points=1, same_class=False):
        self._who = "frames." + type(self).__name__
        self._iou, self._max_misses, self._min_points, self._same_class = \
            _tracker_init_args(iou, max_misses, min_points, same_class, self._who)
        self._map = np.zeros(0, np.int32)
        self._tab = TrackTable(*(np.zeros(0, np.float32 if f == "score" else bool if f == "alive" else np.int32)
                                 for f in TrackTable._fields))
        self._updates = 0

    tracks = property(lambda self: int(self._tab.alive.shape[0]), doc="the tracks so far, alive or retired: the next new id")
    live = property(lambda self: int(self._tab.alive.sum()), doc="the tracks alive")
    cells = property(lambda self: int(self._map.shape[0]), doc="the cells of the map")
    updates = property(lambda self: self._updates, doc="the updates that succeeded")

    def table(self):
        return TrackTable(*(c.copy() for c in self._tab))

    def state(self):
        t, alive = self._map, self._tab.alive
        shown = np.where((t >= 0) & alive[np.maximum(t, 0)], t, -1).astype(np.int32) if alive.size else t.copy()
        return shown, self.table()

    def labels(self, cells):
        who = self._who + ".labels"
        c = _cells_arg(cells, self.cells, "cpu", who).numpy()
        if c.size and not (int(c.min()) >= -1 and int(c.max()) < self.cells):
            raise ValueError(f"{who}: {_CELLS_RANGE} {self.cells} cells")
        shown = self.state()[0]
        return torch.from_numpy(np.where(c >= 0, shown[np.maximum(c, 0)], -1).astype(np.int32) if shown.size
                                else np.full(c.shape, -1, np.int32))

    def update(self, cells, owner, cls, score, keep=None):
        who = self._who + ".update"
        T, u = self.tracks, self._updates
        cells, owner, cls, score, keep = (t.cpu().numpy() for t in _tracker_update_args(cells, owner, cls, score, keep, T, who))
        m, p = cells.shape[0], cls.shape[0]
        if m and (int(cells[0]) < 0 or (m > 1 and not (cells[1:] > cells[:-1]).all())):
            raise ValueError(f"{who}: {_CELLS_ASCEND}")
        if m and not (int(owner.min()) >= -1 and int(owner.max()) < p):
            raise ValueError(f"{who}: {_OWNER_RANGE} {p - 1}")
        M = self.cells
        tab = [c.copy() for c in self._tab]
        t_cls, t_score, t_born, t_seen, t_hits, t_misses, t_size, t_alive = tab
        track_of = np.concatenate([self._map, np.full(max(0, (int(cells[-1]) + 1 if m else 0) - M), -1, np.int32)])
        # 1. rows, tracks, counts
        r = np.where((owner >= 0) & keep[np.maximum(owner, 0)], owner, -1).astype(np.int64) if p else np.full(m, -1, np.int64)
        was = track_of[cells].astype(np.int64)
        t = np.where((was >= 0) & t_alive[np.maximum(was, 0)], was, -1) if T else np.full(m, -1, np.int64)
        a = np.bincount(r[r >= 0], minlength=p).astype(np.int64)
        b = np.bincount(t[t >= 0], minlength=T).astype(np.int64)
        both = (r >= 0) & (t >= 0)
        keys, n = np.unique((r[both] << 32) | t[both], return_counts=True)
        pr, pt, n = keys >> 32, keys & 0xffffffff, n.astype(np.int64)
        if self._same_class:
            on = cls[pr] == t_cls[pt]
            pr, pt, n = pr[on], pt[on], n[on]
        uni = a[pr] + b[pt] - n
        # 2. the best of every row and of every track under the exact order: the larger IoU by cross-multiplied python
        # integers, then the smaller index (one pass over the pairs; there are few of them)
        def best_of(group, index, size):
            best = [-1] * size
            for k, (g, x, nk, uk) in enumerate(zip(group.tolist(), index.tolist(), n.tolist(), uni.tolist())):
                c = best[g]
                if c >= 0:
                    l, rr = nk * int(uni[c]), int(n[c]) * uk
                    if l < rr or (l == rr and x > int(index[c])):
                        continue
                best[g] = k
            return np.array(best, np.int64).reshape(size)

        best_row, best_track = best_of(pr, pt, p), best_of(pt, pr, T)
        # 3. ids
        track = np.full(p, -1, np.int64)
        row_of = np.full(T, -1, np.int64)
        for g in range(p):
            k = best_row[g]
            if k >= 0 and best_track[pt[k]] == k and np.float64(n[k]) >= np.float64(self._iou) * np.float64(uni[k]):
                track[g], row_of[pt[k]] = pt[k], g
        matched = track >= 0
        fresh = ~matched & keep & (a >= self._min_points)
        track[fresh] = T + np.arange(int(fresh.sum()))
        # 4. the table
        k = int(fresh.sum())
        for g in np.nonzero(matched)[0]:
            q = track[g]
            t_hits[q] += 1
            t_misses[q] = 0
            t_seen[q] = u
            if score[g] >= t_score[q]:
                t_score[q], t_cls[q] = score[g], cls[g]
        missed = t_alive & (row_of < 0) & (b > 0)
        t_misses[missed] += 1
        gone = missed & (t_misses > self._max_misses)
        t_alive[gone] = False
        t_size[gone] = 0
        rows = np.nonzero(fresh)[0]
        i32 = lambda v: np.full(k, v, np.int32)  # noqa: E731
        t_cls, t_score = np.concatenate([t_cls, cls[rows].astype(np.int32)]), np.concatenate([t_score, score[rows]])
        t_born, t_seen = np.concatenate([t_born, i32(u)]), np.concatenate([t_seen, i32(u)])
        t_hits, t_misses, t_size = np.concatenate([t_hits, i32(1)]), np.concatenate([t_misses, i32(0)]), np.concatenate([t_size, i32(0)])
        t_alive = np.concatenate([t_alive, np.ones(k, bool)])
        gone = np.concatenate([gone, np.zeros(k, bool)])
        # 5. the map
        tid = np.where(r >= 0, track[np.maximum(r, 0)], -1) if p else np.full(m, -1, np.int64)
        cleared = (t >= 0) & ((row_of[np.maximum(t, 0)] >= 0) | gone[np.maximum(t, 0)]) if T else np.zeros(m, bool)
        now = np.where(tid >= 0, tid, np.where(cleared, -1, t))
        write = (tid >= 0) | cleared
        track_of[cells[write]] = now[write]
        moved = now != t
        lose = moved & (t >= 0)
        lose[lose] = ~gone[t[lose]]
        t_size = t_size - np.bincount(t[lose], minlength=T + k).astype(np.int32) + \
            np.bincount(now[moved & (now >= 0)], minlength=T + k).astype(np.int32)
        empty = t_alive & (t_size == 0)
        t_alive = t_alive & ~empty
        gone |= empty
        self._map = track_of.astype(np.int32)
        self._tab = TrackTable(t_cls.astype(np.int32), t_score.astype(np.float32), t_born, t_seen, t_hits, t_misses,
                               t_size.astype(np.int32), t_alive)
        self._updates = u + 1
        f = lambda v: torch.from_numpy(np.ascontiguousarray(v))  # noqa: E731
        return Tracked(f(now.astype(np.int32)), f(track.astype(np.int32)), f(matched), f(np.arange(T, T + k, dtype=np.int32)),
                       f(np.nonzero(gone)[0].astype(np.int32)))


class Tracker:
    """TrackerHost on the GPU (csrc/frames_track.hip): the same update, labels, table, state and properties,
    bit-identical to the statement after every update and from run to run.  The state is two torch tensors owned here, the
    map int32 [capacity] and the table int32 [8, capacity], each grown by doubling (map_growths, row_growths).  Inputs on
    the host are moved to `device` per update; a tensor on another GPU is a ValueError.

    update: gf_frames_track_update on the current stream (count, best, match, apply, finish); its words are read back
    once, the only synchronisation.  Whatever is on the host is checked before the first launch; on the device the
    count pass raises a word for cells that do not ascend, an owner outside [-1, p) or an overflowing pair table, every
    later launch switches itself off, and the ValueError leaves state() exactly as it was.

    slots: the pair table's entries, a power of two.  None: the smaller of tracker_slots' two sizes; when an update
    overflows it, the update runs ONCE more at the proven size >= 2 m (retries counts these).  A given `slots` is kept:
    overflowing it is a ValueError that names the proven size.  aggregate: whether adjacent lanes of one (row, track)
    pair add once (None: TRACK_AGGREGATE; the result is the same).  pairs: the (row, track) pairs the last update
    counted.  device "cpu": TrackerHost."""

    def __init__(self, iou=0.3, max_misses=2, min_points=1, same_class=False, device="cuda", slots=None, aggregate=None):
        self._who = who = "frames.Tracker"
        dev = torch.device(device)
        self._host = None
        self.retries = self.row_growths = self.map_growths = self.pairs = 0
        if dev.type != "cuda":
            self._host = TrackerHost(iou, max_misses, min_points, same_class)
            return
        self._iou, self._max_misses, self._min_points, self._same_class = \
            _tracker_init_args(iou, max_misses, min_points, same_class, who)
        self._aggregate = int(TRACK_AGGREGATE if aggregate is None else aggregate)
        if slots is not None:
            s = int(slots)
            if not (TRACK_MIN_SLOTS <= s <= TRACK_MAX_SLOTS and s & (s - 1) == 0):
                raise ValueError(f"{who}: slots = {slots} (None, or a power of two from {TRACK_MIN_SLOTS} to {TRACK_MAX_SLOTS})")
        self._slots_arg = None if slots is None else int(slots)
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        tracker_limits()
        self._dev = dev
        self._map = torch.full((_TRACK_MIN_MAP,), -1, dtype=torch.int32, device=dev)
        self._tab = torch.zeros((len(TrackTable._fields), _TRACK_MIN_TABLE), dtype=torch.int32, device=dev)
        self._M = self._T = self._live = self._updates = 0

    tracks = property(lambda self: self._host.tracks if self._host is not None else self._T,
                      doc="the tracks so far, alive or retired: the next new id")
    live = property(lambda self: self._host.live if self._host is not None else self._live, doc="the tracks alive")
    cells = property(lambda self: self._host.cells if self._host is not None else self._M, doc="the cells of the map")
    updates = property(lambda self: self._host.updates if self._host is not None else self._updates,
                       doc="the updates that succeeded")

    def table(self):
        """The TrackTable as torch tensors on the device (copies)."""
        if self._host is not None:
            return self._host.table()
        t = self._tab[:, :self._T]
        return TrackTable(t[0].clone(), t[1].clone().view(torch.float32), t[2].clone(), t[3].clone(), t[4].clone(), t[5].clone(),
                          t[6].clone(), t[7] != 0)

    def _shown(self):
        t = self._map[:self._M]
        if not self._T:
            return t.clone()
        alive = self._tab[7, :self._T] != 0
        return torch.where((t >= 0) & alive[t.clamp(min=0).long()], t, torch.full_like(t, -1))

    def state(self):
        if self._host is not None:
            return self._host.state()
        with torch.cuda.device(self._dev):
            return self._shown().cpu().numpy(), TrackTable(*(c.cpu().numpy() for c in self.table()))

    def labels(self, cells):
        if self._host is not None:
            return self._host.labels(cells)
        who = self._who + ".labels"
        if torch.is_tensor(cells) and cells.is_cuda and cells.device != self._dev:
            raise ValueError(f"{who}: cells on {cells.device}, the tracker on {self._dev}")
        on_host = not (torch.is_tensor(cells) and cells.is_cuda)
        with torch.cuda.device(self._dev):
            c = _cells_arg(cells, self._M, "cpu" if on_host else self._dev, who).to(self._dev)
            if not on_host and c.numel() and bool(((c < -1) | (c >= self._M)).any()):
                raise ValueError(f"{who}: {_CELLS_RANGE} {self._M} cells")
            if not self._M:
                return torch.full_like(c, -1)
            return torch.where(c >= 0, self._shown()[c.clamp(min=0).long()], torch.full_like(c, -1))

    def _grow(self, cells_needed, tracks_needed):
        if cells_needed > self._map.shape[0]:
            cap = self._map.shape[0]
            while cap < cells_needed:
                cap *= 2
            new = torch.full((cap,), -1, dtype=torch.int32, device=self._dev)
            new[:self._M] = self._map[:self._M]
            self._map = new
            self.map_growths += 1
        if tracks_needed > self._tab.shape[1]:
            cap = self._tab.shape[1]
            while cap < tracks_needed:
                cap *= 2
            new = torch.zeros((self._tab.shape[0], cap), dtype=torch.int32, device=self._dev)
            new[:, :self._T] = self._tab[:, :self._T]
            self._tab = new
            self.row_growths += 1

    def update(self, cells, owner, cls, score, keep=None):
        if self._host is not None:
            return self._host.update(cells, owner, cls, score, keep)
        from . import _lib
        from ._lib import check, ptr, stream_ptr

        who = self._who + ".update"
        dev, T, M = self._dev, self._T, self._M
        args = _tracker_update_args(cells, owner, cls, score, keep, T, who)
        for t, name in zip(args, ("cells", "owner", "cls", "score", "keep")):
            if t.is_cuda and t.device != dev:
                raise ValueError(f"{who}: {name} on {t.device}, the tracker on {dev}")
        m, p = args[0].shape[0], args[2].shape[0]
        last = int(args[0][-1]) if m and not args[0].is_cuda else -1  # (cells on the device: the count pass reports it)
        if last >= 2 ** 31 - 1:
            raise ValueError(f"{who}: cell {last}: a map holds at most {2 ** 31 - 1} cells")
        lib = _lib.load()
        default, proven = tracker_slots(p, self._live, m)
        slots = min(default, proven) if self._slots_arg is None else self._slots_arg
        with torch.cuda.device(dev):
            cells, owner, cls, score, keep = (t.to(dev).contiguous() for t in args)
            keep = keep.to(torch.uint8)
            self._grow(last + 1, T + p)
            ids = torch.empty(m, dtype=torch.int32, device=dev)
            track = torch.empty(p, dtype=torch.int32, device=dev)
            gone = torch.empty(max(T, 1), dtype=torch.int32, device=dev)
            words = torch.empty(_TRACK_WORDS, dtype=torch.int32, device=dev)
            for attempt in range(4):
                ws = torch.empty(lib.gf_frames_track_scratch_bytes(m, p, T, slots) // 8 + 1, dtype=torch.int64, device=dev)
                check(lib.gf_frames_track_update(ptr(cells), ptr(owner), m, ptr(cls), ptr(score), ptr(keep), p, ptr(self._map), M,
                                                 self._map.shape[0], ptr(self._tab), T, self._tab.shape[1], self._iou,
                                                 self._max_misses, self._min_points, int(self._same_class), self._updates, slots,
                                                 self._aggregate, ptr(ws), ptr(ids), ptr(track), ptr(gone), ptr(words),
                                                 stream_ptr()), "gf_frames_track_update")
                order, outside, overflow, new, retired, pairs, room, last = words.tolist()[:8]  # the one read-back
                if order:
                    raise ValueError(f"{who}: {_CELLS_ASCEND}")
                if outside:
                    raise ValueError(f"{who}: {_OWNER_RANGE} {p - 1}")
                if room and last >= 2 ** 31 - 1:
                    raise ValueError(f"{who}: cell {last}: a map holds at most {2 ** 31 - 1} cells")
                if room and self._map.shape[0] <= last:
                    self._grow(last + 1, 0)  # cells came on the device: the map is grown and the update run again
                    continue
                if overflow and self._slots_arg is None and slots < proven:
                    slots = proven
                    self.retries += 1
                    continue
                if overflow and self._slots_arg is not None:
                    raise ValueError(f"{who}: the pair table of slots = {slots} overflowed; {proven} slots are always enough "
                                     f"for {m} points")
                if overflow or room:
                    raise RuntimeError(f"{who}: the update failed at {slots} slots and a map of {self._map.shape[0]} cells")
                break
            else:
                raise RuntimeError(f"{who}: the update did not settle")
            self._M = max(M, last + 1) if m else M
            self._T, self._live, self._updates, self.pairs = T + new, self._live + new - retired, self._updates + 1, pairs
            matched = (track >= 0) & (track < T)
            fresh = torch.arange(T, T + new, dtype=torch.int32, device=dev)
            lost = torch.nonzero(gone[:T]).reshape(-1).to(torch.int32) if retired else torch.zeros(0, dtype=torch.int32, device=dev)
        return Tracked(ids, track, matched, fresh, lost)


def track_scene(tracker, fuser, labels, min_obs=1, keep=None):
    """tracker.update over the points of fuser.snapshot(min_obs) with the model's labels of that snapshot (a SceneLabels of
    batch_eval.label_batches): update(fuser.kept(min_obs), labels.owner, table.label_id, table.score, table.kept).
    frames.gather(fused, tracked.ids) then gives every depth pixel its persistent id.  keep: the points are those of
    fuser.snapshot(min_obs, keep=keep)."""
    if not isinstance(tracker, (Tracker, TrackerHost)) or not isinstance(fuser, (Fuser, FuserHost)):
        raise ValueError("frames.track_scene: expected a Tracker and a Fuser (or their host statements)")
    t = labels.table
    return tracker.update(fuser.kept(min_obs, keep), labels.owner, t.label_id, t.score, t.kept)


# ---- free-space evidence: what later frames see of the map's cells ----------------------------------------------------
OUTSIDE, UNKNOWN, OCCLUDED, SEEN, FREE = 0, 1, 2, 3, 4   # the class of a probe, as `codes` holds it


class Visibility(NamedTuple):
    """Per point, int32 [n]: the frames in which it was seen (the depth pixel it projects into measures it, within the
    tolerance), in which the ray went through it (free: the pixel measures a surface well behind it) and in which
    something nearer hides it (occluded).  Frames in which it projects outside the image or onto an invalid pixel count
    nowhere."""
    seen: object
    free: object
    occluded: object


def inverse_records(fr):
    """float32 [F, 12]: per frame the inverse of the 3 x 3 block A of the frame's float32 record (fr.table[f, 4:], the
    camera-to-world P = [A | t]) row-major, then t.  inv = adj(A) / det(A) in float64, written out as cofactors (no
    library call: the bits depend on nothing but the record), rounded to float32 once.  A need not be orthonormal.
    ValueError when a determinant is zero or a value is not finite in float32.  Host only: the statement and the device
    wrapper both call it."""
    if not isinstance(fr, Frames):
        raise ValueError("frames.inverse_records: expected the Frames of frames.make")
    P = fr.table[:, 4:].astype(np.float64).reshape(-1, 3, 4)
    a = lambda r, c: P[:, r, c]  # noqa: E731
    with np.errstate(all="ignore"):
        cof = [a(1, 1) * a(2, 2) - a(1, 2) * a(2, 1), a(0, 2) * a(2, 1) - a(0, 1) * a(2, 2), a(0, 1) * a(1, 2) - a(0, 2) * a(1, 1),
               a(1, 2) * a(2, 0) - a(1, 0) * a(2, 2), a(0, 0) * a(2, 2) - a(0, 2) * a(2, 0), a(0, 2) * a(1, 0) - a(0, 0) * a(1, 2),
               a(1, 0) * a(2, 1) - a(1, 1) * a(2, 0), a(0, 1) * a(2, 0) - a(0, 0) * a(2, 1), a(0, 0) * a(1, 1) - a(0, 1) * a(1, 0)]
        det = (a(0, 0) * cof[0] + a(0, 1) * cof[3]) + a(0, 2) * cof[6]
        if not (np.isfinite(det) & (det != 0)).all():
            raise ValueError(f"frames.inverse_records: frame {int(np.argmin(np.isfinite(det) & (det != 0)))}: the pose's 3 x 3 "
                             "block is singular")
        out = np.concatenate([np.stack(cof, axis=1) / det[:, None], P[:, :, 3]], axis=1).astype(np.float32)
    if not np.isfinite(out).all():
        raise ValueError("frames.inverse_records: an inverse record is not finite in float32")
    return np.ascontiguousarray(out)


def _vis_args(near, far, edge, band, rel, who):
    f32 = np.float32
    near, far, e, band, rel = f32(near), f32(far), f32(0.0 if edge is None else edge), f32(band), f32(rel)
    if np.isnan(near) or np.isnan(far):
        raise ValueError(f"{who}: near and far must be numbers")
    for name, v in (("edge", e), ("band", band), ("rel", rel)):
        if not (v >= 0 and np.isfinite(v)):
            raise ValueError(f"{who}: {name} must be >= 0 and finite in float32, got {v!r}")
    return near, far, e, band, rel


def _vis_points(xyz, who):
    """xyz as it came (a tensor or an array), checked: float32 [n, 3], n <= MAX_POINTS."""
    if not (torch.is_tensor(xyz) or isinstance(xyz, np.ndarray)):
        raise ValueError(f"{who}: xyz: expected a numpy array or a torch tensor, got {type(xyz).__name__}")
    dt = xyz.dtype
    if dt not in (torch.float32, np.float32) or len(xyz.shape) != 2 or xyz.shape[1] != 3:
        raise ValueError(f"{who}: xyz: expected float32 [n, 3], got {dt} {tuple(xyz.shape)}")
    if xyz.shape[0] > MAX_POINTS:
        raise ValueError(f"{who}: {xyz.shape[0]} points (at most {MAX_POINTS})")
    return xyz


def _visibility_host(xyz, fr, inv, near, far, e, band, rel, codes):
    """(counts int32 [3, n] = seen, free, occluded; codes uint8 [F, n] or None) of checked arguments: the rule, one
    frame at a time over all the points."""
    f32 = np.float32
    d = fr.depth.detach().cpu().numpy()
    F, H, W = d.shape
    n = xyz.shape[0]
    counts = np.zeros((3, n), np.int32)
    out = np.zeros((F, n), np.uint8) if codes else None
    x = [np.ascontiguousarray(xyz[:, a]) for a in range(3)]
    with np.errstate(all="ignore"):
        for f in range(F):
            fx, fy, cx, cy = (f32(v) for v in fr.table[f, :4])
            m, t = inv[f, :9].reshape(3, 3), inv[f, 9:]
            dd = [x[a] - t[a] for a in range(3)]
            c = [(m[a, 0] * dd[0] + m[a, 1] * dd[1]) + m[a, 2] * dd[2] for a in range(3)]
            zc = c[2]
            u = ((c[0] * fx) / zc) + cx
            v = ((c[1] * fy) / zc) + cy
            assert zc.dtype == u.dtype == v.dtype == np.float32
            i, j = np.floor(u), np.floor(v)
            inside = (zc >= near) & (i >= 0) & (i < f32(W)) & (j >= 0) & (j < f32(H))
            ii, jj = np.where(inside, i, 0).astype(np.int64), np.where(inside, j, 0).astype(np.int64)
            z = d[f].astype(np.float32) / f32(fr.depth_shift)  # the frame at full resolution; backproject_host's rule
            inr = (z >= near) & (z <= far)
            ok = inr.copy()
            if e > 0:
                lim = e * z
                for dx, dy in ((-1, 0), (1, 0), (0, -1), (0, 1)):
                    zn = _shift2(z[None], dx, dy, f32(0))[0]
                    ok &= ~(_shift2(inr[None], dx, dy, False)[0] & (np.abs(zn - z) > lim))
            zp = z[jj, ii]
            tol = (rel * zp) + band
            assert tol.dtype == np.float32
            cls = np.where(zc < zp - tol, FREE, np.where(zc > zp + tol, OCCLUDED, SEEN))
            cls = np.where(inside, np.where(ok[jj, ii], cls, UNKNOWN), OUTSIDE).astype(np.uint8)
            for row, k in enumerate((SEEN, FREE, OCCLUDED)):
                counts[row] += cls == k
            if codes:
                out[f] = cls
    return counts, out


def visibility_host(xyz, fr, near=0.1, far=10.0, edge=None, band=0.06, rel=0.02, codes=False):
    """The statement of gf_frames_visibility: Visibility of numpy int32 [n] arrays -- per point of xyz (float32 [n, 3],
    world coordinates) the frames of fr that see it, see through it and see something nearer -- and with codes=True
    (Visibility, codes uint8 [F, n]): the class of every probe, 0 OUTSIDE, 1 UNKNOWN, 2 OCCLUDED, 3 SEEN, 4 FREE.  One
    probe, point X in frame f, in float32 with every operation rounded on its own (inv, t: inverse_records):
        d = X - t;  c_a = ((inv[a,0] d0 + inv[a,1] d1) + inv[a,2] d2);  zc = c_2;  !(zc >= near) -> OUTSIDE
        u = ((c_0 fx) / zc) + cx, v likewise; i = floor u, j = floor v; !(0 <= i < W && 0 <= j < H) -> OUTSIDE
        z = depth[f, j, i] / depth_shift (full resolution); the pixel invalid by backproject_host's rule -> UNKNOWN
        tol = (rel z) + band;  zc < z - tol -> FREE;  zc > z + tol -> OCCLUDED;  else SEEN.
    A point that is not finite is OUTSIDE everywhere.  band is metres, rel a share of the measured depth."""
    who = "visibility_host"
    if not isinstance(fr, Frames):
        raise ValueError(f"{who}: expected the Frames of frames.make")
    xyz = _vis_points(xyz, who)
    xyz = xyz.detach().cpu().numpy() if torch.is_tensor(xyz) else xyz
    near, far, e, band, rel = _vis_args(near, far, edge, band, rel, who)
    counts, out = _visibility_host(xyz, fr, inverse_records(fr), near, far, e, band, rel, bool(codes))
    vis = Visibility(counts[0], counts[1], counts[2])
    return (vis, out) if codes else vis


def carve_limits():
    """(stage frames, threads, points, launch shapes) of the library, asserted against this module's constants."""
    from . import _lib

    lib = _lib.load()
    got = (lib.gf_frames_carve_stage_frames(), lib.gf_frames_carve_threads(), lib.gf_frames_carve_max_points(),
           lib.gf_frames_visibility_variants())
    if got != (CARVE_STAGE, CARVE_THREADS, MAX_POINTS, 2):
        raise RuntimeError(f"frames: the library's carve limits {got} are not this module's")
    return got


def _variant_arg(variant, who):
    v = CARVE_VARIANT if variant is None else int(variant)
    if v not in (0, 1):
        raise ValueError(f"{who}: variant = {variant!r} (None, 0: a thread per point, or 1: a thread per probe)")
    return v


def _visibility_device(xyz, fr, inv, near, far, e, band, rel, codes, state, variant, who):
    """(out int32 [3, n], codes uint8 [F, n] or None) on xyz's device; state: None or (seen, free, score, hit, miss, floor,
    ceil), updated by the same call.  Every argument has been checked."""
    from . import _lib
    from ._lib import check, ptr, stream_ptr

    dev, n = xyz.device, xyz.shape[0]
    F, H, W = fr.depth.shape
    with torch.cuda.device(dev):
        depth = (fr.depth if fr.depth.device == dev else fr.depth.to(dev)).contiguous()
        table =torch.from_numpy(fr.table).to(dev, non_blocking=True)
        invd = torch.from_numpy(inv).to(dev, non_blocking=True)
        out = torch.empty((3, n), dtype=torch.int32, device=dev)
        cod = torch.empty((F, n), dtype=torch.uint8, device=dev) if codes else None
        s = state or (None, None, None, 0, 0, 0, 0)
        check(_lib.load().gf_frames_visibility(ptr(xyz), n, ptr(depth), int(depth.dtype == torch.float32), F, H, W,
                                               fr.depth_shift, ptr(table), ptr(invd), float(near), float(far), float(e),
                                               float(band), float(rel), ptr(out), ptr(cod), ptr(s[0]), ptr(s[1]), ptr(s[2]),
                                               *s[3:], variant, stream_ptr()), "gf_frames_visibility")
    return out, cod


def visibility(xyz, fr, near=0.1, far=10.0, edge=None, band=0.06, rel=0.02, codes=False, variant=None):
    """visibility_host on xyz's device: Visibility of int32 [n] tensors (and codes uint8 [F, n] with codes=True), by
    gf_frames_visibility on the current stream -- bit-identical to the statement and from call to call, nothing read
    back.  xyz: a contiguous float32 tensor [n, 3]; the frames are moved to its device when they are elsewhere, as fuse
    does.  variant: the launch shape (None: CARVE_VARIANT; the result is the same).  A CPU tensor runs the statement."""
    who = "frames.visibility"
    if not isinstance(fr, Frames):
        raise ValueError(f"{who}: expected the Frames of frames.make")
    if not torch.is_tensor(xyz):
        raise ValueError(f"{who}: xyz: expected a torch tensor (visibility_host takes arrays)")
    xyz = _vis_points(xyz, who).contiguous()
    near, far, e, band, rel = _vis_args(near, far, edge, band, rel, who)
    variant = _variant_arg(variant, who)
    inv = inverse_records(fr)
    if not xyz.is_cuda:
        counts, out = _visibility_host(xyz.detach().numpy(), fr, inv, near, far, e, band, rel, bool(codes))
        counts, out = torch.from_numpy(counts), None if out is None else torch.from_numpy(out)
    else:
        counts, out = _visibility_device(xyz, fr, inv, near, far, e, band, rel, bool(codes), None, variant, who)
    vis = Visibility(counts[0], counts[1], counts[2])
    return (vis, out) if codes else vis


def _carve_args(fuser, band, rel, hit, miss, floor, ceil, drop, who):
    band = 3.0 * float(fuser._cell) if band is None else band
    near, far, e, band, rel = _vis_args(fuser._near, fuser._far, fuser._edge, band, rel, who)
    ints = []
    for name, v in (("hit", hit), ("miss", miss), ("floor", floor), ("ceil", ceil), ("drop", drop)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not -2 ** 31 <= int(v) < 2 ** 31:
            raise ValueError(f"{who}: {name} = {v!r} (an int32)")
        ints.append(int(v))
    hit, miss, floor, ceil, drop = ints
    if hit < 0 or miss < 0 or floor > ceil:
        raise ValueError(f"{who}: hit = {hit}, miss = {miss} (each >= 0), floor = {floor} <= ceil = {ceil}")
    return (near, far, e, band, rel), (hit, miss, floor, ceil), drop


class CarverHost:
    """The statement of Carver, in numpy, bound to one FuserHost: per cell of the map int32 seen, free (the probes so
    far that saw the cell and that went through it, saturating at 2^31 - 1) and score, OctoMap's clamped occupancy update
    in integers.  A cell that is new since the last call starts at zeros.

    observe(fr) -> Visibility (int32 [fuser.cells] CPU tensors): every cell's current mean (fuser.snapshot(1).xyz) probed
    in every frame of the chunk by visibility_host's rule (near, far and edge are the fuser's; band=None is three times
    its cell), then per cell, with s and f the call's seen and free counts: seen += s, free += f, score = min(ceil,
    max(floor, score + hit s - miss f)) in int64 -- one clamp per cell per call, so the result depends on the order of
    the calls and on nothing inside one.  The chunk need not have the size, dtype or depth_shift of the fuser's stream.
    ValueError -- and the state exactly as it was -- for anything but Frames, a singular pose, or an empty map.

    keep(drop=None) -> bool [fuser.cells]: score > drop (cells newer than the last observe: True).  state() -> (seen,
    free, score) int32 [cells observed so far], copies.  The typical loop is cells = fuser.add(chunk);
    carver.observe(chunk): a cell the chunk created is seen by its own pixels, one it looks through loses score."""

    def __init__(self, fuser, band=None, rel=0.02, hit=1, miss=1, floor=-8, ceil=8, drop=-2):
        self._who = "frames." + type(self).__name__
        if not isinstance(fuser, FuserHost):
            raise ValueError(f"{self._who}: expected a FuserHost")
        self._fuser = fuser
        self._probe, self._rule, self._drop = _carve_args(fuser, band, rel, hit, miss, floor, ceil, drop, self._who)
        self._state = np.zeros((3, 0), np.int32)

    fuser = property(lambda self: self._fuser, doc="the map this carver is bound to")
    cells = property(lambda self: int(self._state.shape[1]), doc="the cells observed so far")
    band = property(lambda self: float(self._probe[3]), doc="the tolerance in metres, as float32")
    drop = property(lambda self: self._drop, doc="keep() drops the cells whose score is at or below it")

    def state(self):
        """(seen, free, score) int32 [cells], copies."""
        return tuple(self._state[k].copy() for k in range(3))

    def observe(self, fr):
        who = self._who + ".observe"
        if not isinstance(fr, Frames):
            raise ValueError(f"{who}: expected the Frames of frames.make")
        M = self._fuser.cells
        if M == 0:
            raise ValueError(f"{who}: the map is empty")
        inv = inverse_records(fr)
        xyz = self._fuser.snapshot(1).xyz.numpy()
        counts, _ = _visibility_host(xyz, fr, inv, *self._probe, False)
        hit, miss, floor, ceil = self._rule
        old = np.zeros((3, M), np.int64)
        old[:, :self._state.shape[1]] = self._state
        s, f = counts[0].astype(np.int64), counts[1].astype(np.int64)
        new = np.empty((3, M), np.int64)
        new[0] = np.minimum(old[0] + s, 2 ** 31 - 1)
        new[1] = np.minimum(old[1] + f, 2 ** 31 - 1)
        new[2] = np.minimum(ceil, np.maximum(floor, old[2] + hit * s - miss * f))
        self._state = new.astype(np.int32)  # nothing above changed the state
        return Visibility(*(torch.from_numpy(np.ascontiguousarray(c)) for c in counts))

    def keep(self, drop=None):
        drop = self._drop if drop is None else int(drop)
        k = np.ones(self._fuser.cells, bool)
        k[:self._state.shape[1]] = self._state[2] > drop
        return torch.from_numpy(k)


class Carver:
    """CarverHost's state on the GPU (csrc/frames_carve.hip), bound to one Fuser: the same observe, keep,
    state and cells, bit-identical to the statement after every call.  seen, free and score are three int32 tensors
    owned here; they grow with fuser.cells (to at least double, zero filled, the old rows copied).  observe is
    fuser.snapshot(1) and one gf_frames_visibility on the current stream, which probes and updates the state in the same
    call; it synchronises nothing itself (the snapshot reads its three words back).  Every check is made before the
    launch: a failed observe leaves the state as it was.  Frames are moved to the fuser's device per observe.  variant:
    the launch shape (None: CARVE_VARIANT; the result is the same).  device "cpu", or a FuserHost: CarverHost."""

    def __init__(self, fuser, band=None, rel=0.02, hit=1, miss=1, floor=-8, ceil=8, drop=-2, device=None, variant=None):
        self._who = who = "frames.Carver"
        self._host = None
        if isinstance(fuser, Fuser) and fuser._host is not None:
            fuser = fuser._host
        if isinstance(fuser, FuserHost):
            if device is not None and torch.device(device).type != "cpu":
                raise ValueError(f"{who}: a FuserHost's carver lives on the CPU, got device = {device!r}")
            self._host = CarverHost(fuser, band, rel, hit, miss, floor, ceil, drop)
            return
        if not isinstance(fuser, Fuser):
            raise ValueError(f"{who}: expected a Fuser (or a FuserHost)")
        if device is not None and torch.device(device).type != "cuda":
            raise ValueError(f"{who}: a Fuser's carver lives on its device {fuser._dev}, got device = {device!r}")
        self._fuser = fuser
        self._probe, self._rule, self._drop = _carve_args(fuser, band, rel, hit, miss, floor, ceil, drop, who)
        self._variant = _variant_arg(variant, who)
        carve_limits()
        self._dev = fuser._dev
        self._M = 0
        self.row_growths = 0
        with torch.cuda.device(self._dev):
            self._seen, self._free, self._score = (torch.zeros(_CARVE_MIN_ROWS, dtype=torch.int32, device=self._dev)
                                                   for _ in range(3))

    fuser = property(lambda self: self._host.fuser if self._host is not None else self._fuser,
                     doc="the map this carver is bound to")
    cells = property(lambda self: self._host.cells if self._host is not None else self._M, doc="the cells observed so far")
    band = property(lambda self: self._host.band if self._host is not None else float(self._probe[3]),
                    doc="the tolerance in metres, as float32")
    drop = property(lambda self: self._host.drop if self._host is not None else self._drop,
                    doc="keep() drops the cells whose score is at or below it")

    def state(self):
        """CarverHost.state() of this carver: (seen, free, score) int32 [cells] numpy arrays, read back."""
        if self._host is not None:
            return self._host.state()
        return tuple(t[:self._M].cpu().numpy() for t in (self._seen, self._free, self._score))

    def observe(self, fr):
        if self._host is not None:
            return self._host.observe(fr)
        who = self._who + ".observe"
        if not isinstance(fr, Frames):
            raise ValueError(f"{who}: expected the Frames of frames.make")
        M, dev = self._fuser.cells, self._dev
        if M == 0:
            raise ValueError(f"{who}: the map is empty")
        inv = inverse_records(fr)
        with torch.cuda.device(dev):
            xyz = self._fuser.snapshot(1).xyz.contiguous()  # all M cells in cell order
            cap = self._seen.shape[0]
            if M > cap:
                cap = max(2 * cap, M)
                grown = []
                for old in (self._seen, self._free, self._score):
                    t = torch.zeros(cap, dtype=torch.int32, device=dev)
                    t[:self._M] = old[:self._M]
                    grown.append(t)
                self._seen, self._free, self._score = grown
                self.row_growths += 1
            out, _ = _visibility_device(xyz, fr, inv, *self._probe, False, (self._seen, self._free, self._score) + self._rule,
                                        self._variant, who)
        self._M = M
        return Visibility(out[0], out[1], out[2])

    def keep(self, drop=None):
        if self._host is not None:
            return self._host.keep(drop)
        drop = self._drop if drop is None else int(drop)
        with torch.cuda.device(self._dev):
            k = torch.ones(self._fuser.cells, dtype=torch.bool, device=self._dev)
            k[:self._M] = self._score[:self._M] > drop
        return k
