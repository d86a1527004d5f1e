"""The segment-pooling kernel family beside the framework statement of the same pooling, for a kernel trace:

    rocprofv3 --kernel-trace --stats -d artifacts/segment_pool -- python tools/segment_pool_trace.py --what kernel
    rocprofv3 --kernel-trace --stats -d artifacts/segment_pool_torch -- python tools/segment_pool_trace.py --what torch

One scene of --points foreground points and --nq queries (default 256) whose over-segments look like
scene.grid_segments' on a scanned room: runs of a few tens to a few hundreds of points that are neighbours in point
order too, a few large ones, ~3 % of the points without a segment.
--what kernel: --reps calls of pointops.segment_pool_batched (the key arithmetic and the stable sort of the framework,
then k_sp_heads, the three scan launches, k_sp_runs, k_sp_pool, k_sp_combine and k_sp_open in the stats; nothing is read
back between the calls).
--what torch: the same pooling as a user can write it behind the forward: index_add_ of the logits into [nq, segments]
sums (float atomics: the order of the additions is not fixed), a division and a gather (the dense segment index is
prepared once, outside the timed part).
Both check their result once against postprocess.segment_pool_host -- the kernel to the bound of the GPU tests, the
framework form loosely, its sums being unordered -- and print one JSON line: microseconds per call and the algorithmic
bytes 2 * nq * N_fg * 4 (the logits read once and written once).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_segments(n, seed=1):
    """int32 [n]: run lengths drawn log-uniformly from 8 .. 400 with one run in 200 ten times longer, members next to
    each other in point order up to a local shuffle (a mesh's vertex order is only roughly spatial), 3 % without."""
    rng = np.random.default_rng(seed)
    lens = []
    total = 0
    while total < n:
        k = int(np.exp(rng.uniform(np.log(8), np.log(400))))
        if rng.random() < 0.005:
            k *= 10
        lens.append(k)
        total += k
    seg = np.repeat(rng.permutation(len(lens)) * 7 + 3, lens)[:n]  # sparse, unsorted ids
    for lo in range(0, n, 2048):  # neighbours in space, not in index: shuffle inside windows
        w = seg[lo:lo + 2048]
        seg[lo:lo + 2048] = w[rng.permutation(len(w))]
    seg[rng.random(n) < 0.03] = -1
    return seg.astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=("kernel", "torch"), default="kernel")
    ap.add_argument("--points", type=int, default=100_003)
    ap.add_argument("--nq", type=int, default=256)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()

    import geoformer_amd

    geoformer_amd.configure_runtime()
    from geoformer_amd import pointops, postprocess

    n, nq = args.points, args.nq
    seg = make_segments(n)
    rng = np.random.default_rng(2)
    x = (rng.standard_normal((nq, n)) * 8).astype(np.float32)
    want = postprocess.segment_pool_host(x, seg)
    ids, counts = np.unique(seg[seg >= 0], return_counts=True)
    out = {"what": args.what, "points": n, "nq": nq, "segments": int(ids.size), "longest": int(counts.max()),
           "median": int(np.median(counts)), "algorithmic_bytes": 2 * nq * n * 4}
    x_d, seg_d = torch.from_numpy(x).cuda(), torch.from_numpy(seg).cuda()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if args.what == "kernel":
        for i in range(args.reps + 5):
            if i == 5:
                torch.cuda.synchronize()
                ev0.record()
            got = pointops.segment_pool_batched([x_d], seg_d, [0, n])[0]
        ev1.record()
        torch.cuda.synchronize()
        # the bound of tests/test_gpu_segment_pool.py: k * 2^-23 * mean|x| per (query, run of k points)
        k = np.ones(n)
        k[seg >= 0] = counts[np.searchsorted(ids, seg[seg >= 0])]
        mean_abs = postprocess.segment_pool_host(np.abs(x), seg).astype(np.float64)
        assert (np.abs(got.cpu().numpy().astype(np.float64) - want) <= k[None, :] * 2.0 ** -23 * mean_abs + 1e-30).all()
    else:
        # the dense segment index, prepared once: a point without a segment is a segment of its own
        dense = np.empty(n, np.int64)
        dense[seg >= 0] = np.searchsorted(ids, seg[seg >= 0])
        dense[seg < 0] = ids.size + np.arange(int((seg < 0).sum()))
        n_seg = int(dense.max()) + 1
        dense_d = torch.from_numpy(dense).cuda()
        cnt = torch.bincount(dense_d, minlength=n_seg).float()
        for i in range(args.reps + 5):
            if i == 5:
                torch.cuda.synchronize()
                ev0.record()
            sums = torch.zeros((nq, n_seg), dtype=torch.float32, device="cuda").index_add_(1, dense_d, x_d)
            got = (sums / cnt[None, :])[:, dense_d]
        ev1.record()
        torch.cuda.synchronize()
        assert np.allclose(got.cpu().numpy(), want, rtol=1e-3, atol=1e-3)
    us = ev0.elapsed_time(ev1) * 1e3 / args.reps  # back-to-back calls, host included
    out["call_us_events"] = round(us, 2)
    out["algorithmic_GBps_of_call"] = round(out["algorithmic_bytes"] / us / 1e3, 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
