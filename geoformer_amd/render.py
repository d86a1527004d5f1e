"""Headless rendering of a scene's points to images: what util/visualize.py shows in a viewer (the input colours, the
semantic labels or predictions, the instances), as uint8 images on the device, with no display and no imaging library.

    cams = render.turntable(render.bounds_of(xyz), 8, 30.0, (1024, 768))
    rgb, ids, keep = render.colors_for("instance_pred", raw_scene=raw, labels=labels)
    image, index = render.render(xyz, rgb, cams, (1024, 768), ids=ids, keep=keep)   # uint8 [8, 768, 1024, 3] on the GPU

The hot path is csrc/render.hip: a z-buffered point splat (64-bit atomicMin of depthkey << 32 | point index) and a
resolve pass (shading, outlines, the supersampling mean); a fill, the splat and the resolve are the three stream
operations of a chunk of views.  splat_host / resolve_host are the numpy statement of the two kernels, float32 and
integer operations in the same order: the kernels are tested bit for bit against them.

Image coordinates: x to the right, y down, pixel (i, j) covers [i, i + 1) x [j, j + 1).  A Camera is given in output
pixels; camera_table scales it to the sub-pixel grid of the supersampling factor.  Radii are in sub-pixels.
"""
from __future__ import annotations

import colorsys
import math
from typing import NamedTuple

import numpy as np

CAMERA_FLOATS = 20  # gf_render_camera_floats(): asserted against the library in limits()
MAX_VIEWS = 64
MAX_SIDE = 4096
MAX_RADIUS = 16
MAX_SUPERSAMPLE = 4
MAX_STRIDE = 16
SMALL_RADIUS = 3  # up to here a thread per (point, view); above, the lanes of a wave cover each footprint
KINDS = {"ortho": 0, "persp": 1}
TASKS = ("input", "semantic_gt", "semantic_pred", "instance_gt", "instance_pred")
IGNORE_LABEL = -100  # util/visualize.py drops these points
BACKGROUND_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)


class Camera(NamedTuple):
    """One view, in output pixels.  R's rows are the image's right, the image's down and the viewing direction; scale is
    pixels per metre (ortho) or the focal length in pixels (persp); near only culls in persp."""
    eye: tuple
    R: tuple  # 3 x 3, row-major
    kind: str
    scale: float
    cx: float
    cy: float
    near: float = 0.05


class Shade(NamedTuple):
    """Depth-cue shading of the resolve pass: lut[o] (Q8, 256 = unchanged) for a sub-pixel with o of its 8 neighbours at
    `stride` sub-pixels nearer to the camera by more than dz metres."""
    lut: tuple = (256, 238, 220, 203, 187, 172, 158, 145, 133)
    stride: int = 2
    dz: float = 0.02


NO_SHADE = Shade((256,) * 9, 1, 0.0)


# ---- cameras (host, float64; rounded to float32 once, in camera_table) -------------------------------------------------
def bounds_of(xyz):
    """(lo [3], hi [3]) of the points, float64 on the host."""
    p = xyz.detach().cpu().numpy() if hasattr(xyz, "detach") else np.asarray(xyz)
    p = p.reshape(-1, 3).astype(np.float64)
    if p.shape[0] == 0:
        return np.zeros(3), np.zeros(3)
    return p.min(0), p.max(0)


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """R float64 [3, 3] of a camera at eye looking at target: rows right, down, forward (right x down = forward)."""
    eye, target, up = (np.asarray(a, np.float64).reshape(3) for a in (eye, target, up))
    fwd = target - eye
    n = np.linalg.norm(fwd)
    if not n > 0:
        raise ValueError("look_at: eye and target coincide")
    fwd = fwd / n
    right = np.cross(fwd, up)
    if np.linalg.norm(right) < 1e-9:  # looking along up: any horizontal direction serves
        right = np.cross(fwd, np.roll(up, 1))
    right = right / np.linalg.norm(right)
    down = np.cross(fwd, right)
    return np.stack([right, down, fwd])


def _size(size):
    W, H = (int(s) for s in size)
    if not (1 <= W <= MAX_SIDE and 1 <= H <= MAX_SIDE):
        raise ValueError(f"render: an image of {W} x {H} pixels (each side 1 to {MAX_SIDE})")
    return W, H


def _cam(eye, R, kind, scale, W, H, near):
    return Camera(tuple(float(v) for v in eye), tuple(float(v) for v in np.asarray(R).reshape(9)), kind, float(scale),
                  W / 2.0, H / 2.0, float(near))


def top_down(bounds, size, margin=0.95):
    """An orthographic camera above the box looking down -z, +y up in the image, the box's x / y extent inside
    `margin` of the image."""
    lo, hi = (np.asarray(b, np.float64).reshape(3) for b in bounds)
    W, H = _size(size)
    c = (lo + hi) / 2
    ext = np.maximum(hi - lo, 1e-6)
    scale = margin * min(W / ext[0], H / ext[1])
    eye = (c[0], c[1], hi[2] + 1.0)
    return _cam(eye, look_at(eye, (c[0], c[1], c[2] - 1.0 + hi[2] - c[2]), up=(0.0, 1.0, 0.0)), "ortho", scale, W, H, 0.05)


def turntable(bounds, n_views, elevation_deg, size, kind="persp", fov_deg=45.0, margin=0.95):
    """n_views cameras on a circle around the box's centre at elevation_deg above the horizon, z up, each framing the
    box's bounding sphere inside `margin` of the image's shorter side."""
    if kind not in KINDS:
        raise ValueError(f"turntable: kind must be one of {tuple(KINDS)}, got {kind!r}")
    if int(n_views) < 1:
        raise ValueError(f"turntable: n_views = {n_views}")
    lo, hi = (np.asarray(b, np.float64).reshape(3) for b in bounds)
    W, H = _size(size)
    c = (lo + hi) / 2
    rad = max(float(np.linalg.norm(hi - lo)) / 2, 1e-3)
    half = margin * min(W, H) / 2  # pixels the sphere's outline may reach from the centre
    if kind == "persp":
        scale = (H / 2) / math.tan(math.radians(fov_deg) / 2)
        dist = rad / math.sin(math.atan(half / scale))
        near = (dist - rad) / 2
    else:
        scale = half / rad
        dist = 2 * rad + 1.0
        near = 0.05
    el = math.radians(elevation_deg)
    cams = []
    for k in range(int(n_views)):
        az = 2 * math.pi * k / int(n_views)
        eye = c + dist * np.array([math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el)])
        cams.append(_cam(eye, look_at(eye, c), kind, scale, W, H, near))
    return cams


def _radius(radius):
    rmin, rmax = (radius, radius) if np.isscalar(radius) else radius
    rmin, rmax = int(rmin), int(rmax)
    if not 0 <= rmin <= rmax <= MAX_RADIUS:
        raise ValueError(f"render: radius = {radius!r} (0 <= rmin <= rmax <= {MAX_RADIUS} sub-pixels)")
    return rmin, rmax


def camera_table(cams, supersample=1, radius=0, point_size=0.0):
    """fp32 [V, CAMERA_FLOATS] of gf_render_splat for the sub-pixel grid of `supersample`: per view {eye, R, kind,
    scale, cx, cy, near, spx, rmin, rmax}, computed in float64 and rounded once.  radius: the disc's radius in
    sub-pixels, or (rmin, rmax) with point_size metres: a perspective view then draws a point floor(spx / depth)
    sub-pixels wide within those bounds, spx = scale * point_size."""
    cams = [cams] if isinstance(cams, Camera) else list(cams)
    S = int(supersample)
    if not 1 <= S <= MAX_SUPERSAMPLE:
        raise ValueError(f"render: supersample = {supersample} (1 to {MAX_SUPERSAMPLE})")
    rmin, rmax = _radius(radius)
    t = np.zeros((len(cams), CAMERA_FLOATS), np.float64)
    for i, c in enumerate(cams):
        if c.kind not in KINDS:
            raise ValueError(f"render: camera {i}: kind must be one of {tuple(KINDS)}, got {c.kind!r}")
        t[i, 0:3] = c.eye
        t[i, 3:12] = np.asarray(c.R, np.float64).reshape(9)
        t[i, 12] = KINDS[c.kind]
        t[i, 13:16] = (c.scale * S, c.cx * S, c.cy * S)
        t[i, 16] = c.near
        t[i, 17] = c.scale * S * float(point_size)
        t[i, 18:20] = (rmin, rmax)
        if c.kind == "persp" and not c.near > 0:
            raise ValueError(f"render: camera {i}: a perspective camera needs near > 0, got {c.near}")
    if not np.isfinite(t).all():
        raise ValueError("render: a camera holds a value that is not finite")
    out = t.astype(np.float32)
    assert out.shape[1] == CAMERA_FLOATS
    return out


# ---- the host statement -----------------------------------------------------------------------------------------------
def _check_table(table, name):
    t = np.asarray(table)
    if t.ndim != 2 or t.shape[1] != CAMERA_FLOATS or t.dtype != np.float32 or not 1 <= t.shape[0] <= MAX_VIEWS:
        raise ValueError(f"{name}: cams: expected float32 [1..{MAX_VIEWS}, {CAMERA_FLOATS}], got {t.dtype} {t.shape}")
    return np.ascontiguousarray(t)


def _check_grid(Ws, Hs, max_radius, name):
    side = MAX_SIDE * MAX_SUPERSAMPLE
    Ws, Hs, max_radius = int(Ws), int(Hs), int(max_radius)
    if not (1 <= Ws <= side and 1 <= Hs <= side):
        raise ValueError(f"{name}: a grid of {Ws} x {Hs} sub-pixels (each side 1 to {side})")
    if not 0 <= max_radius <= MAX_RADIUS:
        raise ValueError(f"{name}: max_radius = {max_radius} (0 to {MAX_RADIUS})")
    return Ws, Hs, max_radius


def project_host(xyz, cam, Ws, Hs, max_radius):
    """One view of the splat's projection, float32, each operation rounded on its own: (ok bool [N], iu, iv, r int64
    [N], depthkey uint32 [N]); the integers are valid where ok."""
    p = np.asarray(xyz, np.float32).reshape(-1, 3)
    c = np.asarray(cam, np.float32)
    f = np.float32
    with np.errstate(all="ignore"):
        d0, d1, d2 = p[:, 0] - c[0], p[:, 1] - c[1], p[:, 2] - c[2]
        xc = (c[3] * d0 + c[4] * d1) + c[5] * d2
        yc = (c[6] * d0 + c[7] * d1) + c[8] * d2
        zc = (c[9] * d0 + c[10] * d1) + c[11] * d2
        rm = c[19] if c[19] <= f(max_radius) else f(max_radius)
        rf = np.full(p.shape[0], c[18], np.float32)
        ok = np.ones(p.shape[0], bool)
        if c[12] != 0:
            ok = zc >= c[16]
            u = (xc * c[13]) / zc + c[14]
            v = (yc * c[13]) / zc + c[15]
            q = np.floor(c[17] / zc)
            rf = np.where(q > rf, q, rf)
        else:
            u = xc * c[13] + c[14]
            v = yc * c[13] + c[15]
        rf = np.where(rf > rm, rm, rf)
        rf = np.where(rf >= 0, rf, f(0))
        m = rm + f(1)
        ok = ok & (u >= -m) & (u < f(Ws) + m) & (v >= -m) & (v < f(Hs) + m)
        assert u.dtype == np.float32 and rf.dtype == np.float32 and zc.dtype == np.float32
        iu = np.floor(np.where(ok, u, f(0))).astype(np.int64)
        iv = np.floor(np.where(ok, v, f(0))).astype(np.int64)
    bits = np.ascontiguousarray(zc).view(np.uint32)
    dk = np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000))
    return ok, iu, iv, rf.astype(np.int64), dk


def disc_offsets(r):
    """(dx, dy) int64 [k] each of the disc dx^2 + dy^2 <= r^2 + r."""
    a = np.arange(-r, r + 1)
    dx, dy = np.meshgrid(a, a)
    sel = dx * dx + dy * dy <= r * r + r
    return dx[sel], dy[sel]


def splat_host(xyz, keep, cams, Ws, Hs, max_radius=MAX_RADIUS):
    """The statement of gf_render_splat: keys uint64 [V, Hs, Ws], all-ones where no point lands."""
    cams = _check_table(cams, "splat_host")
    Ws, Hs, max_radius = _check_grid(Ws, Hs, max_radius, "splat_host")
    p = np.asarray(xyz, np.float32).reshape(-1, 3)
    keys = np.full((cams.shape[0], Hs * Ws), BACKGROUND_KEY, np.uint64)
    live = np.ones(p.shape[0], bool) if keep is None else np.asarray(keep).reshape(-1) != 0
    for vi, cam in enumerate(cams):
        ok, iu, iv, r, dk = project_host(p, cam, Ws, Hs, max_radius)
        ok &= live
        idx = np.nonzero(ok)[0]
        key = (dk[idx].astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint64)
        for rr in np.unique(r[idx]):
            sel = r[idx] == rr
            dx, dy = disc_offsets(int(rr))
            x = iu[idx][sel][:, None] + dx[None, :]
            y = iv[idx][sel][:, None] + dy[None, :]
            inside = (x >= 0) & (x < Ws) & (y >= 0) & (y < Hs)
            k = np.broadcast_to(key[sel][:, None], x.shape)
            np.minimum.at(keys[vi], (y * Ws + x)[inside], k[inside])
    return keys.reshape(cams.shape[0], Hs, Ws)


def depth_of_keys(keys):
    """The float32 depth a key's high word holds (exactly the zc it was made from)."""
    dk = (np.asarray(keys).view(np.uint64) >> np.uint64(32)).astype(np.uint32)
    bits = np.where(dk & np.uint32(0x80000000), dk ^ np.uint32(0x80000000), ~dk)
    return np.ascontiguousarray(bits).view(np.float32)


def _shifted(a, dx, dy, fill):
    """out[..., y, x] = a[..., y + dy, x + dx] inside the image, fill outside."""
    out = np.full_like(a, fill)
    H, W = a.shape[-2:]
    ys, xs = slice(max(0, -dy), max(0, min(H, H - dy))), slice(max(0, -dx), max(0, min(W, W - dx)))
    yt, xt = slice(ys.start + dy, ys.stop + dy), slice(xs.start + dx, xs.stop + dx)
    if ys.stop > ys.start and xs.stop > xs.start:
        out[..., ys, xs] = a[..., yt, xt]
    return out


def _rgb24(c, name):
    c = tuple(int(v) for v in c)
    if len(c) != 3 or not all(0 <= v <= 255 for v in c):
        raise ValueError(f"render: {name} = {c!r} (three values 0 to 255)")
    return c


def _check_shade(shade):
    shade = NO_SHADE if shade is None else shade
    lut = np.asarray(shade.lut, np.int64).reshape(-1)
    if lut.shape != (9,) or lut.min() < 0 or lut.max() > 256:
        raise ValueError("render: shade.lut: 9 entries in 0..256")
    if not 1 <= int(shade.stride) <= MAX_STRIDE:
        raise ValueError(f"render: shade.stride = {shade.stride} (1 to {MAX_STRIDE})")
    return lut.astype(np.int32), int(shade.stride), float(np.float32(shade.dz))


def resolve_host(keys, S, rgb, ids=None, shade=None, background=(255, 255, 255), outline=(0, 0, 0)):
    """The statement of gf_render_resolve: (image uint8 [V, H, W, 3], index int32 [V, H S, W S])."""
    keys = np.asarray(keys).view(np.uint64)
    S = int(S)
    if not 1 <= S <= MAX_SUPERSAMPLE:
        raise ValueError(f"render: supersample = {S} (1 to {MAX_SUPERSAMPLE})")
    if keys.ndim != 3 or keys.shape[1] % S or keys.shape[2] % S or 0 in keys.shape:
        raise ValueError(f"resolve_host: keys {keys.shape} is not [V, H S, W S] for S = {S}")
    V, Hs, Ws = keys.shape
    rgb = np.asarray(rgb, np.uint8).reshape(-1, 3)
    N = rgb.shape[0]
    lut, st, dz = _check_shade(shade)
    bg, ol = _rgb24(background, "background"), _rgb24(outline, "outline")
    lo = keys & np.uint64(0xFFFFFFFF)
    fg = lo < np.uint64(N)
    index = np.where(fg, lo, 0).astype(np.int64)
    z = depth_of_keys(keys)
    o = np.zeros(keys.shape, np.int64)
    with np.errstate(all="ignore"):
        for ny in (-1, 0, 1):
            for nx in (-1, 0, 1):
                if nx or ny:
                    o += _shifted(fg, nx * st, ny * st, False) & (_shifted(z, nx * st, ny * st, 0) + np.float32(dz) < z)
    col = (rgb[index].astype(np.int64) * lut[o][..., None] + 128) >> 8 if N else np.zeros(keys.shape + (3,), np.int64)
    if ids is not None:
        ids = np.asarray(ids).reshape(-1)
        mine = ids[index] if N else np.zeros(keys.shape, np.int64)
        edge = np.zeros(keys.shape, bool)
        for dx, dy in ((1, 0), (0, 1)):
            inside = _shifted(np.ones(keys.shape, bool), dx, dy, False)
            edge |= inside & (~_shifted(fg, dx, dy, False) | (_shifted(mine, dx, dy, 0) != mine))
        col = np.where(edge[..., None], np.array(ol, np.int64), col)
    col = np.where(fg[..., None], col, np.array(bg, np.int64))
    image = (col.reshape(V, Hs // S, S, Ws // S, S, 3).sum((2, 4)) + S * S // 2) // (S * S)
    return image.astype(np.uint8), np.where(fg, index, -1).astype(np.int32)


# ---- device wrappers --------------------------------------------------------------------------------------------------
def limits():
    """(camera floats, views, side, radius, supersample) of the library, asserted against this module's constants."""
    from . import _lib

    lib = _lib.load()
    got = (lib.gf_render_camera_floats(), lib.gf_render_max_views(), lib.gf_render_max_side(), lib.gf_render_max_radius(),
           lib.gf_render_max_supersample())
    if got != (CAMERA_FLOATS, MAX_VIEWS, MAX_SIDE, MAX_RADIUS, MAX_SUPERSAMPLE):
        raise RuntimeError(f"render: the library's limits {got} are not this module's")
    return got


def _dev_tensor(t, dtype, shape, name, optional=False):
    import torch

    if t is None and optional:
        return None
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dtype and t.is_contiguous()):
        raise RuntimeError(f"render: {name}: expected a contiguous {dtype} tensor on the GPU")
    if tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"render: {name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    return t


def _xyz_checked(xyz):
    import torch

    if not (torch.is_tensor(xyz) and xyz.is_cuda and xyz.dtype == torch.float32 and xyz.is_contiguous()
            and xyz.dim() == 2 and xyz.shape[1] == 3):
        raise RuntimeError("render: xyz: expected a contiguous float32 tensor [N, 3] on the GPU")
    return xyz


def splat(xyz, keep, cams, Ws, Hs, max_radius=MAX_RADIUS):
    """keys int64 [V, Hs, Ws] on xyz's device (gf_render_splat; the bit patterns of splat_host): one fill and one launch
    on the current stream.  xyz fp32 [N, 3] and keep uint8 [N] or None on the device; cams: the fp32 [V, F] table of
    camera_table, on the host (uploaded here) or already on the device.  Everything is checked before any launch."""
    import torch

    from . import _lib
    from .pointops import check, ptr, stream_ptr

    xyz = _xyz_checked(xyz)
    N = xyz.shape[0]
    keep = _dev_tensor(keep, torch.uint8, (N,), "keep", optional=True)
    Ws, Hs, max_radius = _check_grid(Ws, Hs, max_radius, "render.splat")
    if torch.is_tensor(cams):
        if cams.dim() != 2 or not 1 <= cams.shape[0] <= MAX_VIEWS:
            raise RuntimeError(f"render: cams: 1 to {MAX_VIEWS} views, got {tuple(cams.shape)}")
        table = _dev_tensor(cams, torch.float32, (cams.shape[0], CAMERA_FLOATS), "cams")
    else:
        table = torch.from_numpy(_check_table(cams, "render.splat")).to(xyz.device, non_blocking=True)
    V = table.shape[0]
    with torch.cuda.device(xyz.device):
        keys = torch.full((V, Hs, Ws), -1, dtype=torch.int64, device=xyz.device)  # all-ones: background
        check(_lib.load().gf_render_splat(ptr(xyz), ptr(keep), N, ptr(table), V, Ws, Hs, max_radius, ptr(keys),
                                          stream_ptr()), "gf_render_splat")
    return keys


def resolve(keys, S, rgb, ids=None, shade=None, background=(255, 255, 255), outline=(0, 0, 0)):
    """(image uint8 [V, H, W, 3], index int32 [V, H S, W S]) on the device from the keys of splat (gf_render_resolve, the
    values of resolve_host): one launch, every cell of both written.  rgb uint8 [N, 3], ids int32 [N] or None."""
    import torch

    from . import _lib
    from .pointops import check, ptr, stream_ptr

    S = int(S)
    if not 1 <= S <= MAX_SUPERSAMPLE:
        raise ValueError(f"render: supersample = {S} (1 to {MAX_SUPERSAMPLE})")
    if not (torch.is_tensor(keys) and keys.is_cuda and keys.dtype == torch.int64 and keys.is_contiguous()
            and keys.dim() == 3 and 0 not in keys.shape and keys.shape[1] % S == 0 and keys.shape[2] % S == 0):
        raise RuntimeError(f"render: keys: expected a contiguous int64 tensor [V, H S, W S] on the GPU for S = {S}")
    V, Hs, Ws = keys.shape
    W, H = _size((Ws // S, Hs // S))
    if not 1 <= V <= MAX_VIEWS:
        raise RuntimeError(f"render: {V} views (1 to {MAX_VIEWS})")
    if not (torch.is_tensor(rgb) and rgb.dim() == 2 and rgb.shape[1] == 3):
        raise RuntimeError("render: rgb: expected a uint8 tensor [N, 3] on the GPU")
    N = rgb.shape[0]
    rgb = _dev_tensor(rgb, torch.uint8, (N, 3), "rgb")
    ids = _dev_tensor(ids, torch.int32, (N,), "ids", optional=True)
    lut, st, dz = _check_shade(shade)
    bg, ol = _rgb24(background, "background"), _rgb24(outline, "outline")
    pack = lambda c: (c[0] << 16) | (c[1] << 8) | c[2]  # noqa: E731
    with torch.cuda.device(keys.device):
        image = torch.empty((V, H, W, 3), dtype=torch.uint8, device=keys.device)
        index = torch.empty((V, Hs, Ws), dtype=torch.int32, device=keys.device)
        check(_lib.load().gf_render_resolve(ptr(keys), V, W, H, S, ptr(rgb), ptr(ids), N, lut.ctypes.data, st, dz, pack(bg),
                                            pack(ol), ptr(image), ptr(index), stream_ptr()), "gf_render_resolve")
    return image, index


def render(xyz, rgb, cams, size, *, supersample=2, radius=2, ids=None, keep=None, shade=Shade(), point_size=0.0,
           background=(255, 255, 255), outline=(0, 0, 0), max_bytes=256 << 20):
    """(image uint8 [V, H, W, 3], index int32 [V, H S, W S]) on xyz's device: the points xyz fp32 [N, 3] in the colours
    rgb uint8 [N, 3] seen by the cameras (a Camera or a list of them), size = (W, H) pixels.  supersample S: the splat
    and the shading run on a W S x H S grid and a pixel is the mean of its S x S block.  radius (sub-pixels), point_size:
    see camera_table.  ids int32 [N]: outlines where neighbouring sub-pixels hold different ids; keep uint8 [N]: points
    with 0 are not drawn; shade: a Shade, or None for flat colours.  The views go in chunks whose key buffer (8 bytes per
    sub-pixel and view) stays under max_bytes: a fill, the splat and the resolve per chunk, nothing read back.  Every
    argument is checked before the first launch."""
    import torch

    cams = [cams] if isinstance(cams, Camera) else list(cams)
    if not cams:
        raise ValueError("render: no cameras")
    W, H = _size(size)
    S = int(supersample)
    table = camera_table(cams, S, radius, point_size)
    rmax = _radius(radius)[1]
    xyz = _xyz_checked(xyz)
    N = xyz.shape[0]
    if not (torch.is_tensor(rgb) and rgb.dim() == 2):
        raise RuntimeError("render: rgb: expected a uint8 tensor [N, 3] on the GPU")
    rgb = _dev_tensor(rgb, torch.uint8, (N, 3), "rgb")
    ids = _dev_tensor(ids, torch.int32, (N,), "ids", optional=True)
    keep = _dev_tensor(keep, torch.uint8, (N,), "keep", optional=True)
    _check_shade(shade), _rgb24(background, "background"), _rgb24(outline, "outline")
    per_view = 8 * W * S * H * S
    chunk = int(min(MAX_VIEWS, max(1, int(max_bytes) // per_view)))
    images, indices = [], []
    for a in range(0, len(cams), chunk):
        keys = splat(xyz, keep, table[a:a + chunk], W * S, H * S, rmax)
        im, ix = resolve(keys, S, rgb, ids, shade, background, outline)
        images.append(im)
        indices.append(ix)
    return (images[0], indices[0]) if len(images) == 1 else (torch.cat(images), torch.cat(indices))


def render_host(xyz, rgb, cams, size, *, supersample=2, radius=2, ids=None, keep=None, shade=Shade(), point_size=0.0,
                background=(255, 255, 255), outline=(0, 0, 0)):
    """render on the host: resolve_host(splat_host(...)) with the same arguments as numpy arrays."""
    cams = [cams] if isinstance(cams, Camera) else list(cams)
    W, H = _size(size)
    S = int(supersample)
    table = camera_table(cams, S, radius, point_size)
    outs = [resolve_host(splat_host(xyz, keep, table[a:a + MAX_VIEWS], W * S, H * S, _radius(radius)[1]), S, rgb, ids,
                         shade, background, outline) for a in range(0, len(cams), MAX_VIEWS)]
    return np.concatenate([o[0] for o in outs]), np.concatenate([o[1] for o in outs])


# ---- colours ----------------------------------------------------------------------------------------------------------
def _class_palette(n=41):
    """The project's class table (wide enough for the benchmark's label ids 0..40): hues a golden-ratio step apart,
    three lightness levels in turn."""
    out = []
    for k in range(n):
        r, g, b = colorsys.hls_to_rgb((0.11 + 0.61803398875 * k) % 1.0, (0.45, 0.62, 0.34)[k % 3], (0.70, 0.55, 0.85)[k % 2])
        out.append((round(255 * r), round(255 * g), round(255 * b)))
    return np.array(out, np.uint8)


CLASS_PALETTE = _class_palette()
UNLABELLED_RGB = (190, 190, 190)  # a point without a class or an instance


def instance_colors(ids):
    """uint8 [N, 3] of integer ids (tensor): a multiplicative hash of the id, three of its bytes mapped into 56..247;
    negative ids (no instance) are UNLABELLED_RGB."""
    import torch

    i = ids.to(torch.int64)
    h = ((i + 1) * 2654435761) & 0xFFFFFFFF
    h = (h ^ (h >> 15)) * 2246822519 & 0xFFFFFFFF
    rgb = torch.stack([(h >> s) & 0xFF for s in (24, 13, 3)], dim=1)
    rgb = (56 + (rgb * 3 >> 2)).to(torch.uint8)
    rgb[i < 0] = torch.tensor(UNLABELLED_RGB, dtype=torch.uint8, device=rgb.device)
    return rgb


def colors_for(task, raw_scene=None, labels=None, semantic=None, palette=None, device=None):
    """(rgb uint8 [N, 3], ids int32 [N] or None, keep uint8 [N] or None) of one of TASKS, as tensors on `device` (default:
    where the given tensors are, else the CPU), by plain tensor indexing.
      input          raw_scene [N, 8]: its colours, stored in [-1, 1]
      semantic_gt    raw_scene: column 6 through the palette; keep drops the unannotated points (-100)
      semantic_pred  semantic: int [N], the class per point (batch_eval.semantic_batches' preds)
      instance_gt    raw_scene: column 7 hashed to a colour, ids = the instance; keep as semantic_gt
      instance_pred  labels: a postprocess.SceneLabels (host or device): owner hashed to a colour, ids = owner
    palette: uint8 [K, 3] for the semantic tasks (default CLASS_PALETTE); a class outside it is UNLABELLED_RGB."""
    import torch

    if task not in TASKS:
        raise ValueError(f"colors_for: task must be one of {TASKS}, got {task!r}")
    need = {"input": raw_scene, "semantic_gt": raw_scene, "instance_gt": raw_scene, "semantic_pred": semantic,
            "instance_pred": labels}[task]
    if need is None:
        raise ValueError(f"colors_for: {task} needs " + {"semantic_pred": "semantic=", "instance_pred": "labels="}.get(
            task, "raw_scene="))
    src = labels.owner if task == "instance_pred" else need
    if device is None:
        device = src.device if torch.is_tensor(src) else "cpu"
    t = torch.as_tensor(src).to(device)

    def classes(cls):
        pal = torch.as_tensor(CLASS_PALETTE if palette is None else palette)
        if pal.dtype != torch.uint8 or pal.dim() != 2 or pal.shape[1] != 3 or pal.shape[0] < 1:
            raise ValueError("colors_for: palette: expected uint8 [K, 3]")
        pal = torch.cat([pal.to(device), torch.tensor([UNLABELLED_RGB], dtype=torch.uint8, device=device)])
        K = pal.shape[0] - 1
        cls = cls.to(torch.int64)
        return pal[torch.where((cls >= 0) & (cls < K), cls, torch.full_like(cls, K))]

    if task == "input":
        if t.dim() != 2 or t.shape[1] < 6:
            raise ValueError(f"colors_for: raw_scene: expected [N, 8], got {tuple(t.shape)}")
        c = torch.floor((t[:, 3:6].to(torch.float32) + 1.0) * 127.5).clamp_(0, 255)
        return c.to(torch.uint8).contiguous(), None, None
    if task == "semantic_pred":
        return classes(t.reshape(-1)), None, None
    if task == "instance_pred":
        return instance_colors(t.reshape(-1)), t.reshape(-1).to(torch.int32).contiguous(), None
    if t.dim() != 2 or t.shape[1] != 8:
        raise ValueError(f"colors_for: raw_scene: expected [N, 8], got {tuple(t.shape)}")
    sem = t[:, 6].to(torch.int64)
    keep = (sem != IGNORE_LABEL).to(torch.uint8)
    if task == "semantic_gt":
        return classes(sem), None, keep
    inst = t[:, 7].to(torch.int32).contiguous()
    return instance_colors(inst), inst, keep


# ---- boxes as points: the existing splat draws them over a scene ------------------------------------------------------
BOX_EDGES = ((0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7))


def box_corners(boxes):
    """float64 [p, 8, 3]: the corners of every box of a postprocess.Boxes: the lower face counter-clockwise from the
    (-u, -v) corner, then the upper face in the same order."""
    h = lambda a: np.asarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a, dtype=np.float64)  # noqa: E731
    c, s = h(boxes.cos).reshape(-1, 1), h(boxes.sin).reshape(-1, 1)
    center, half = h(boxes.center).reshape(-1, 3), h(boxes.size).reshape(-1, 3) / 2
    su = np.array([-1.0, 1.0, 1.0, -1.0, -1.0, 1.0, 1.0, -1.0])[None, :]
    sv = np.array([-1.0, -1.0, 1.0, 1.0, -1.0, -1.0, 1.0, 1.0])[None, :]
    sz = np.array([-1.0] * 4 + [1.0] * 4)[None, :]
    u, v = su * half[:, 0:1], sv * half[:, 1:2]
    return np.stack([center[:, 0:1] + u * c - v * s, center[:, 1:2] + u * s + v * c, center[:, 2:3] + sz * half[:, 2:3]],
                    axis=2)


def box_points(boxes, step=0.02, rgb=(255, 0, 0)):
    """(xyz fp32 [M, 3], rgb uint8 [M, 3]): the 12 edges of every box as points `step` metres apart (both end points
    included), box after box, edge after edge in BOX_EDGES' order.  rgb: one colour, or one per box [p, 3].  Concatenate
    them with a scene's points and colours and render.render draws the boxes over the scene."""
    if not step > 0:
        raise ValueError(f"box_points: step must be positive, got {step!r}")
    corners = box_corners(boxes)
    p = corners.shape[0]
    colours = np.broadcast_to(np.asarray(rgb, dtype=np.uint8).reshape(-1, 3), (p, 3)) if p else np.zeros((0, 3), np.uint8)
    pts, cols = [np.zeros((0, 3), np.float32)], [np.zeros((0, 3), np.uint8)]
    for b in range(p):
        for i, j in BOX_EDGES:
            a, e = corners[b, i], corners[b, j]
            k = int(np.ceil(np.linalg.norm(e - a) / step)) + 1
            t = np.linspace(0.0, 1.0, max(k, 2))[:, None]
            seg = (a[None, :] * (1.0 - t) + e[None, :] * t).astype(np.float32)
            pts.append(seg)
            cols.append(np.broadcast_to(colours[b], seg.shape).copy())
    return np.concatenate(pts), np.concatenate(cols)
