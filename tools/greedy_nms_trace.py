"""Time of the greedy NMS walk kernel against the framework loop on device tensors (postprocess.greedy_nms_loop, one
read-back per proposal: what there was before the kernel), on random run-masks with distinct scores.

    python tools/greedy_nms_trace.py [--sizes 256x60000 1024x60000] [--thresh 0.3] [--reps 30]

Per size one JSON line: picks kept, device-event time of ONE launch of gf_greedy_nms_ious and of gf_greedy_nms_batched's
walk (median [min, max] over --reps launches after a warm-up; the intersections are computed once, outside), host wall
time of the whole calls (non_max_suppression_gpu; greedy_nms_batched with packing, intersections and the read-back of
the count) and of the loop, each ending in a synchronise.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run_masks(rng, n, N):
    masks = np.zeros((n, N), np.int32)
    for i in range(n):
        ln = int(rng.integers(N // 50 + 1, N // 4 + 2))
        s = int(rng.integers(0, N - ln + 1))
        masks[i, s:s + ln] = 1
    return masks, ((rng.permutation(n) + 1) / (n + 1)).astype(np.float32)


def spread(ts):
    ts = sorted(ts)
    return [round(ts[len(ts) // 2], 2), round(ts[0], 2), round(ts[-1], 2)]


def events(fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return spread(out)


def wall(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e6)
    return spread(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", nargs="*", default=["256x60000", "1024x60000"])
    ap.add_argument("--thresh", type=float, default=0.3)
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    import geoformer_amd

    geoformer_amd.configure_runtime()
    from geoformer_amd import pointops, postprocess as pp

    for size in args.sizes:
        n, N = (int(v) for v in size.split("x"))
        masks, scores = run_masks(np.random.default_rng(n), n, N)
        m, s = torch.from_numpy(masks).cuda(), torch.from_numpy(scores).cuda()
        f = m.float()
        inter = f @ f.t()
        d = torch.diagonal(inter)
        ious = (inter / ((d[:, None] + d[None, :]) - inter)).contiguous()
        want = pp.greedy_nms_loop(ious, s, args.thresh)
        got = pp.non_max_suppression_gpu(ious, s, args.thresh)
        (got_b,) = pp.greedy_nms_batched([m], [s], args.thresh)
        assert torch.equal(want, got) and torch.equal(want, got_b), "kernel and loop disagree"
        _, table, table_d, sizes, _keep = pp._nms_batch_table("greedy_nms_batched", [m], [s])
        inter_i = pointops.mask_intersections_batched(table_d, sizes)
        for _ in range(3):  # warm-up of every timed shape
            pointops.greedy_nms_ious(ious, s, args.thresh)
            pointops.greedy_nms_batched(table_d, inter_i, sizes, args.thresh)
        torch.cuda.synchronize()
        res = {"n": n, "N": N, "threshold": args.thresh, "kept": int(want.numel()), "unit": "us, median [min, max]",
               "launch_ious_events": events(lambda: pointops.greedy_nms_ious(ious, s, args.thresh), args.reps),
               "launch_batched_walk_events": events(lambda: pointops.greedy_nms_batched(table_d, inter_i, sizes,
                                                                                         args.thresh), args.reps),
               "call_non_max_suppression_gpu_wall": wall(lambda: pp.non_max_suppression_gpu(ious, s, args.thresh),
                                                         args.reps),
               "call_greedy_nms_batched_wall": wall(lambda: pp.greedy_nms_batched([m], [s], args.thresh), args.reps),
               "framework_loop_wall": wall(lambda: pp.greedy_nms_loop(ious, s, args.thresh), max(3, args.reps // 10))}
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
