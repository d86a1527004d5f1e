"""The renderer's kernels (csrc/render.hip) beside the same z-buffer written as a plain framework expression, timed with
events around each call:

    python tools/render_trace.py                      # kernel and framework form, one JSON line each
    rocprofv3 --kernel-trace --stats -d artifacts/render -- python tools/render_trace.py --what kernel

The scene is the benchmark generator's room (scene.make_raw_scene(--points, 1234)), seen by --views perspective
turntable cameras at 30 degrees, --size pixels, supersampling --supersample, discs of --radius sub-pixels.
--what kernel: render.render as a whole (per chunk of views a fill, the splat, the resolve), and the fill + splat and
the resolve on their own, and the fill alone.  Derived: atomic_updates = the (point, view, sub-pixel) triples inside the
image, each one read and at most one atomicMin, per second of the splat (fill + splat minus the fill); resolve bytes = 8 (key) + 4 (index) per sub-pixel and 3 per pixel, the bytes the pass cannot
avoid (the neighbour keys it reads again, and the colours of the winners, come on top).
--what torch: the yardstick, the same keys from framework operations: the projection as float32 tensor expressions
over [V, N], int64 keys with the sign bit flipped (signed order = the kernel's unsigned order), and one
scatter_reduce_(amin) per cell of the disc into a [V Hs Ws + 1] buffer whose last cell takes what falls outside; the
keys are compared with the kernel's bit for bit once.  Each figure is min / median / max over --reps calls after 3
warm-ups."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

HBM_BYTES_PER_S = 8e12


def build_parser():
    from predict_scenes import parse_size

    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=("both", "kernel", "torch"), default="both")
    ap.add_argument("--points", type=int, default=150_000)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--size", type=parse_size, default=(1024, 768))
    ap.add_argument("--supersample", type=int, default=2)
    ap.add_argument("--radius", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    return ap


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    us.sort()
    return [round(us[0], 1), round(us[len(us) // 2], 1), round(us[-1], 1)]


SIGN = -(1 << 63)


def torch_project(xyz, table, Ws, Hs):
    """(ok [V, N], iu, iv int64, key int64 with the sign bit flipped) of perspective records with one radius."""
    c = table[:, None, :]
    d0, d1, d2 = (xyz[None, :, j] - c[..., j] for j in range(3))
    xc = (c[..., 3] * d0 + c[..., 4] * d1) + c[..., 5] * d2
    yc = (c[..., 6] * d0 + c[..., 7] * d1) + c[..., 8] * d2
    zc = ((c[..., 9] * d0 + c[..., 10] * d1) + c[..., 11] * d2).contiguous()
    u = (xc * c[..., 13]) / zc + c[..., 14]
    v = (yc * c[..., 13]) / zc + c[..., 15]
    m = c[..., 19] + 1.0
    ok = (zc >= c[..., 16]) & (u >= -m) & (u < Ws + m) & (v >= -m) & (v < Hs + m)
    bits = zc.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    dk = torch.where((bits & 0x80000000) != 0, ~bits & 0xFFFFFFFF, bits | 0x80000000)
    key = ((dk << 32) | torch.arange(xyz.shape[0], device=xyz.device)[None, :]) ^ SIGN
    zero = torch.zeros_like(u)
    return ok, torch.floor(torch.where(ok, u, zero)).to(torch.int64), torch.floor(torch.where(ok, v, zero)).to(torch.int64), key


def torch_splat(xyz, table, Ws, Hs, r):
    """The z-buffer of render.splat as framework operations: int64 [V, Hs, Ws], the kernel's bit patterns."""
    from geoformer_amd import render

    V = table.shape[0]
    ok, iu, iv, key = torch_project(xyz, table, Ws, Hs)
    buf = torch.full((V * Hs * Ws + 1,), torch.iinfo(torch.int64).max, dtype=torch.int64, device=xyz.device)
    base = (torch.arange(V, device=xyz.device) * (Hs * Ws))[:, None]
    dump = torch.full_like(iu, V * Hs * Ws)
    for dx, dy in zip(*render.disc_offsets(r)):
        x, y = iu + int(dx), iv + int(dy)
        inside = ok & (x >= 0) & (x < Ws) & (y >= 0) & (y < Hs)
        cell = torch.where(inside, base + y * Ws + x, dump)
        buf.scatter_reduce_(0, cell.reshape(-1), key.reshape(-1), "amin")
    return (buf[:-1] ^ SIGN).view(V, Hs, Ws)


def main():
    args = build_parser().parse_args()

    import geoformer_amd

    geoformer_amd.configure_runtime()
    from geoformer_amd import render, scene

    raw = scene.make_raw_scene(args.points, 1234)
    W, H = args.size
    S, r, V = args.supersample, args.radius, args.views
    Ws, Hs = W * S, H * S
    cams = render.turntable(render.bounds_of(raw[:, :3]), V, 30.0, (W, H))
    table = render.camera_table(cams, S, r)
    table_d = torch.from_numpy(table).cuda()
    xyz = torch.from_numpy(raw[:, :3].astype(np.float32)).cuda()
    rgb, ids, _ = render.colors_for("instance_gt", raw_scene=raw, device="cuda")
    ok, iu, iv, _ = torch_project(xyz, table_d, Ws, Hs)
    updates = 0
    for dx, dy in zip(*render.disc_offsets(r)):
        x, y = iu + int(dx), iv + int(dy)
        updates += int((ok & (x >= 0) & (x < Ws) & (y >= 0) & (y < Hs)).sum())
    print(json.dumps({"points": xyz.shape[0], "views": V, "size": [W, H], "supersample": S, "radius": r,
                      "point_views_in_frustum": int(ok.sum()), "atomic_updates": updates, "sub_pixels": V * Hs * Ws}))
    keys = render.splat(xyz, None, table_d, Ws, Hs, r)
    if args.what in ("both", "kernel"):
        out = {"form": "kernel"}
        out["render_us"] = timed(lambda: render.render(xyz, rgb, cams, (W, H), supersample=S, radius=r, ids=ids,
                                                       max_bytes=1 << 40), args.reps)
        out["fill_splat_us"] = timed(lambda: render.splat(xyz, None, table_d, Ws, Hs, r), args.reps)
        out["fill_us"] = timed(lambda: torch.full((V, Hs, Ws), -1, dtype=torch.int64, device="cuda"), args.reps)
        image, index = render.resolve(keys, S, rgb, ids, render.Shade())
        out["resolve_us"] = timed(lambda: render.resolve(keys, S, rgb, ids, render.Shade()), args.reps)
        out["foreground_fraction"] = round(float((index >= 0).float().mean()), 3)
        nbytes = 12 * V * Hs * Ws + 3 * V * H * W
        out["atomic_updates_per_s"] = round(updates / ((out["fill_splat_us"][1] - out["fill_us"][1]) * 1e-6), 0)
        out["resolved_sub_pixels_per_s"] = round(V * Hs * Ws / (out["resolve_us"][1] * 1e-6), 0)
        out["resolve_bytes"] = nbytes
        out["resolve_fraction_of_hbm_peak"] = round(nbytes / (out["resolve_us"][1] * 1e-6) / HBM_BYTES_PER_S, 3)
        print(json.dumps(out))
    if args.what in ("both", "torch"):
        got = torch_splat(xyz, table_d, Ws, Hs, r)
        out = {"form": "torch", "keys_equal_kernel": bool(torch.equal(got, keys)),
               "splat_us": timed(lambda: torch_splat(xyz, table_d, Ws, Hs, r), args.reps),
               "launches_scatter_reduce": len(render.disc_offsets(r)[0])}
        print(json.dumps(out))


if __name__ == "__main__":
    main()
