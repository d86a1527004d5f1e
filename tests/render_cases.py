"""Scenes, cameras and an independent per-pixel brute force for the renderer's tests (test_render_host.py on the host,
test_gpu_render.py on the GPU).  Coordinates are metre-scale, so no denormal arises."""
import numpy as np

from geoformer_amd import render

F32 = np.float32


def axis_camera(kind="ortho", scale=1.0, cx=0.0, cy=0.0, near=1.0, eye=(0.0, 0.0, 0.0)):
    """Right = +x, down = +y, forward = +z: with the defaults a point (x, y, z) lands on sub-pixel (floor x, floor y)
    at depth z."""
    return render.Camera(tuple(eye), (1, 0, 0, 0, 1, 0, 0, 0, 1), kind, scale, cx, cy, near)


def project_point(p, c, Ws, Hs, max_radius):
    """One point, one camera record, scalar float32 operations in the order of include/geoformer_hip.h: None when
    culled, else (iu, iv, r, depthkey)."""
    p = [F32(v) for v in p]
    c = [F32(v) for v in c]
    with np.errstate(all="ignore"):
        d = [p[0] - c[0], p[1] - c[1], p[2] - c[2]]
        xc, yc, zc = [F32(F32(F32(c[3 + 3 * j] * d[0]) + F32(c[4 + 3 * j] * d[1])) + F32(c[5 + 3 * j] * d[2]))
                      for j in range(3)]
        rm = c[19] if c[19] <= F32(max_radius) else F32(max_radius)
        r = c[18]
        if c[12] != 0:
            if not zc >= c[16]:
                return None
            u = F32(F32(F32(xc * c[13]) / zc) + c[14])
            v = F32(F32(F32(yc * c[13]) / zc) + c[15])
            q = np.floor(F32(c[17] / zc))
            if q > r:
                r = q
        else:
            u = F32(F32(xc * c[13]) + c[14])
            v = F32(F32(yc * c[13]) + c[15])
        if r > rm:
            r = rm
        if not r >= 0:
            r = F32(0)
        m = F32(rm + F32(1))
        if not (u >= -m and u < F32(F32(Ws) + m) and v >= -m and v < F32(F32(Hs) + m)):
            return None
    bits = int(np.array(zc, F32).view(np.uint32))
    dk = (~bits & 0xFFFFFFFF) if bits & 0x80000000 else bits | 0x80000000
    return int(np.floor(u)), int(np.floor(v)), int(r), dk


def brute_force_keys(xyz, keep, table, Ws, Hs, max_radius):
    """uint64 [V, Hs, Ws]: per sub-pixel the minimum key over all points whose disc covers it (a loop over sub-pixels
    inside a loop over points' projections; nothing is scattered)."""
    out = np.full((len(table), Hs, Ws), 0xFFFFFFFFFFFFFFFF, np.uint64)
    for vi, c in enumerate(table):
        hits = []
        for i, p in enumerate(np.asarray(xyz, F32).reshape(-1, 3)):
            if keep is not None and not keep[i]:
                continue
            h = project_point(p, c, Ws, Hs, max_radius)
            if h is not None:
                hits.append(h + (i,))
        for y in range(Hs):
            for x in range(Ws):
                best = 0xFFFFFFFFFFFFFFFF
                for iu, iv, r, dk, i in hits:
                    if (x - iu) ** 2 + (y - iv) ** 2 <= r * r + r:
                        best = min(best, (dk << 32) | i)
                out[vi, y, x] = best
    return out


def random_case(N, size, V, S, kind, radius, seed, point_size=0.0, spread=1.25, with_ids=True, with_keep=True):
    """A random cloud in a box around the origin seen by a turntable (kind) whose frame is that of a box 1 / spread as
    large, so that some points fall outside the image.  Returns the arguments of render.render / render_host."""
    rng = np.random.default_rng(seed)
    W, H = size
    xyz = (rng.uniform(-1.0, 1.0, (N, 3)) * np.array([2.0, 1.5, 1.0]) * spread).astype(F32)
    lo, hi = np.array([-2.0, -1.5, -1.0]), np.array([2.0, 1.5, 1.0])
    cams = render.turntable((lo, hi), V, 25.0, (W, H), kind=kind)
    return dict(xyz=xyz, rgb=rng.integers(0, 256, (N, 3), dtype=np.uint8), cams=cams, size=(W, H), supersample=S,
                radius=radius, point_size=point_size,
                ids=rng.integers(0, 5, N).astype(np.int32) if with_ids else None,
                keep=(rng.random(N) < 0.9).astype(np.uint8) if with_keep else None)


def axis_case(points, size, S=1, radius=0, kind="ortho", rgb=None, ids=None, keep=None, shade=None, **cam):
    """Points given in sub-pixel coordinates of an axis_camera (scale 1 on the sub-pixel grid)."""
    xyz = np.asarray(points, F32).reshape(-1, 3)
    N = xyz.shape[0]
    c = axis_camera(kind, scale=cam.pop("scale", 1.0) / S, **cam)
    if rgb is None:
        rgb = (np.arange(3 * N, dtype=np.int64).reshape(N, 3) * 37 % 251 + 2).astype(np.uint8)
    return dict(xyz=xyz, rgb=np.asarray(rgb, np.uint8).reshape(N, 3), cams=[c], size=size, supersample=S, radius=radius,
                point_size=0.0, ids=None if ids is None else np.asarray(ids, np.int32),
                keep=None if keep is None else np.asarray(keep, np.uint8), shade=shade)


def named_cases():
    """name -> case: the situations of the issue's list, on an axis camera so that the expected picture is plain."""
    W, H = 12, 9
    out = {}
    # a radius-3 disc clipped at each border and at a corner
    for name, (x, y) in {"clip_left": (0.5, 4.5), "clip_right": (11.5, 4.5), "clip_top": (5.5, 0.5),
                         "clip_bottom": (5.5, 8.5), "clip_corner": (11.5, 8.5), "centre_just_outside": (-2.5, 0.5)}.items():
        out[name] = axis_case([(x, y, 2.0), (6.5, 4.5, 3.0)], (W, H), radius=3)
    out["outside_frustum"] = axis_case([(-40.0, 4.0, 1.0), (6.0, 90.0, 1.0), (1e9, 1.0, 1.0), (5.5, 4.5, 2.0)], (W, H), radius=1)
    out["near_plane"] = axis_case([(0.0, 0.0, 1.0), (0.3, 0.1, 0.99999994), (0.0, 0.2, -1.0), (0.1, 0.0, 0.0), (-2.0, -1.0, 4.0)],
                                  (W, H), radius=1, kind="persp", scale=8.0, cx=6.0, cy=4.5, near=1.0)
    out["negative_depth_ortho"] = axis_case([(3.5, 3.5, -2.0), (3.5, 3.5, -1.0), (3.5, 3.5, 1.0), (4.5, 3.5, -0.0),
                                             (4.5, 3.5, 0.0), (5.5, 3.5, 0.5), (5.5, 3.5, -0.5)], (W, H), radius=0)
    out["same_position"] = axis_case([(9.5, 2.5, 1.0), (3.5, 3.5, 1.5), (3.5, 3.5, 1.5), (3.5, 3.5, 1.5)], (W, H), radius=2)
    rng = np.random.default_rng(5)
    crowd = np.concatenate([np.full((1000, 1), 6.25), np.full((1000, 1), 4.75), rng.integers(1, 9, (1000, 1)) * 0.25], 1)
    out["contention_1000_on_one_pixel"] = axis_case(crowd, (W, H), radius=1)
    out["keep_removes_nearest"] = axis_case([(5.5, 4.5, 1.0), (5.5, 4.5, 2.0), (7.5, 4.5, 3.0)], (W, H), radius=1,
                                            keep=[0, 1, 1])
    return out


def host_arrays(case):
    """(xyz, keep, table, Ws, Hs, max_radius) of a case for splat_host / brute_force_keys."""
    S = case["supersample"]
    table = render.camera_table(case["cams"], S, case["radius"], case.get("point_size", 0.0))
    W, H = case["size"]
    return case["xyz"], case["keep"], table, W * S, H * S, render._radius(case["radius"])[1]


def render_kwargs(case):
    kw = {k: case[k] for k in ("supersample", "radius", "point_size")}
    if "shade" in case:
        kw["shade"] = case["shade"]
    return kw
