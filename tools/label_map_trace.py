"""One 150k-point scene with ~50 picked instances through the scene-labelling kernels and through the device-to-host
copy of the [n, N] int32 masks they replace, for a kernel trace:

    rocprofv3 --kernel-trace --stats -d artifacts/label_map -- python tools/label_map_trace.py

Also prints both times from device events / the wall clock (median of --reps), one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=150_000)
    ap.add_argument("--proposals", type=int, default=67)  # pick = the best three quarters: 50 instances
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()

    import geoformer_amd

    geoformer_amd.configure_runtime()
    from geoformer_amd import postprocess
    from tests.test_label_map_host import label_case

    case = label_case(np.random.default_rng(11), args.proposals, args.points)
    masks, scores, label_ids, pick, xyz = [torch.from_numpy(a).cuda() for a in case]
    host = torch.empty(masks.shape, dtype=masks.dtype).pin_memory()
    kern, copy, small = [], [], []
    for i in range(args.reps + 3):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        e[0].record()
        lab = postprocess.label_points(masks, scores, label_ids, pick, xyz)
        e[1].record()
        torch.cuda.synchronize()
        t = time.perf_counter()
        lab.to_host()
        t1 = time.perf_counter()
        host.copy_(masks)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if i >= 3:
            kern.append(e[0].elapsed_time(e[1]) * 1e3), small.append((t1 - t) * 1e6), copy.append((t2 - t1) * 1e6)
    med = lambda v: round(float(np.median(v)), 1)  # noqa: E731
    print(json.dumps({"points": args.points, "proposals": args.proposals, "picked": int(pick.numel()),
                      "label_points_us_events": med(kern), "labels_to_host_us": med(small),
                      "masks_int32_to_pinned_host_us": med(copy), "mask_bytes": masks.numel() * 4}))


if __name__ == "__main__":
    main()
