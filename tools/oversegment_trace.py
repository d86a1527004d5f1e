"""The launches of the geometric over-segmentation on one generated scene, for a kernel trace:

    rocprofv3 --kernel-trace --stats -d artifacts/oversegment -- python tools/oversegment_trace.py

One scene.make_scene of --points points (default 150 000; spacing ~2 cm), radius = 3 x spacing, offset = 0.5 x spacing,
the other parameters at their defaults.  --reps calls of each of the three stages, back to back and nothing read back in
between: pointops.knn_radius (the hash grid's launches and k_knn_radius in the stats), pointops.point_normals
(k_point_normals) and pointops.smooth_components (k_sc_init, k_sc_hook, k_sc_flatten, k_sc_dissolve, k_sc_attach), then
--reps calls of pointops.oversegment, the chain a user runs.  Prints one JSON line: microseconds per call of each stage
and of the chain between events on the stream (back-to-back calls, host included), the segments found, the share of
points without one, and the algorithmic bytes of the two new stages (point_normals: the rows, one 12-byte gather per
row entry, 16 bytes out; smooth_components: the rows twice, two 16-byte normals and two 12-byte points per row entry).
The per-kernel times are the profiler's; this tool only makes the launches.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=150_000)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--seed", type=int, default=1234)
    args = ap.parse_args()

    import geoformer_amd

    geoformer_amd.configure_runtime()
    from geoformer_amd import pointops, scene

    sc = scene.make_scene(args.points, args.seed)
    sp = float(sc["spacing"])
    xyz = torch.from_numpy(sc["xyz"].astype(np.float32)).cuda()
    n, k = xyz.shape[0], args.k
    kw = dict(offset=0.5 * sp)
    _, I, deg = pointops.knn_radius(xyz, k, 3 * sp, sqrt_out=False, check_overflow=True)
    n4 = pointops.point_normals(xyz, I, deg)
    stages = {
        "knn_radius": lambda: pointops.knn_radius(xyz, k, 3 * sp, sqrt_out=False),
        "point_normals": lambda: pointops.point_normals(xyz, I, deg),
        "smooth_components": lambda: pointops.smooth_components(xyz, n4, I, deg, **kw),
        "oversegment": lambda: pointops.oversegment(xyz, k=k, radius=3 * sp, **kw),
    }
    out = {"points": n, "k": k, "radius": round(3 * sp, 5), "reps": args.reps}
    ids = None
    for name, fn in stages.items():
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for i in range(args.reps + 5):
            if i == 5:
                torch.cuda.synchronize()
                ev0.record()
            ids = fn()
        ev1.record()
        torch.cuda.synchronize()
        out[f"{name}_call_us_events"] = round(ev0.elapsed_time(ev1) * 1e3 / args.reps, 2)
    ids = ids.cpu().numpy()
    entries = int((deg.cpu().numpy().astype(np.int64) + 1).sum())
    out.update(segments=int(np.unique(ids[ids >= 0]).size), without_segment=round(float((ids < 0).mean()), 4),
               row_entries=entries, point_normals_algorithmic_bytes=n * (k * 4 + 4 + 12 + 16) + entries * 12,
               smooth_components_algorithmic_bytes=2 * n * (k * 4 + 4) + entries * (2 * 16 + 2 * 12) + n * 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
