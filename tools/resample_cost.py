"""What the grid subsample and the nearest-point search (csrc/resample.hip) cost on a dense scan, beside their host
statements on the same input:

    python tools/resample_cost.py                         # one JSON line per figure
    python tools/resample_cost.py --points 20000 --copies 50 --reps 21

The scan: the benchmark generator's room (scene.make_raw_scene(--points, 1234)) densified to about 1 M points -- every
point --copies times, each copy jittered by a normal of 2 mm -- in a random order.
grid_subsample: gf_grid_subsample at --cell (default 0.02) in both modes, timed with a pair of events recorded on the
stream right before the call's first memset and right after its last launch (the device path: six memsets, seven
launches and the copy of the two words; the wrapper's read-back of the words and its allocations are outside), as the
median of --reps calls after 5 warm-ups.
nearest_point: gf_nearest_point of every point of the scan against the subsample's representatives at max_dist =
2 * cell, timed the same way.
host: postprocess.grid_subsample_host on the whole scan, once, wall clock; postprocess.nearest_point_host on the first
--host-queries queries (brute force: Q x n distances), scaled to the whole scan's Q.  Both device results are compared
with the statements once (the nearest point on the host's queries)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def dense_scan(points, copies, seed=0):
    from geoformer_amd import scene

    x = scene.make_raw_scene(points, 1234)[:, :3].astype(np.float32)
    rng = np.random.default_rng(seed)
    x = np.repeat(x, copies, 0) + rng.normal(0, 0.002, (x.shape[0] * copies, 3)).astype(np.float32)
    return np.ascontiguousarray(x[rng.permutation(x.shape[0])])


def device_us(call, reps):
    """median / min / max microseconds between two events recorded on the stream around `call` (which only enqueues)."""
    for _ in range(5):
        call()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    us.sort()
    return {"median_us": round(us[len(us) // 2], 1), "min_us": round(us[0], 1), "max_us": round(us[-1], 1)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--copies", type=int, default=50)
    ap.add_argument("--cell", type=float, default=0.02)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--host-queries", type=int, default=2000)
    args = ap.parse_args()

    import geoformer_amd

    geoformer_amd.configure_runtime()
    from geoformer_amd import _lib, pointops, postprocess
    from geoformer_amd._lib import check, ptr, stream_ptr

    lib = _lib.load()
    x = dense_scan(args.points, args.copies)
    N = x.shape[0]
    xd = torch.from_numpy(x).cuda()
    out = torch.empty((3, N), dtype=torch.int32, device="cuda")
    words = torch.empty(2, dtype=torch.int32, device="cuda")
    ws = torch.empty(lib.gf_grid_subsample_scratch_bytes(N) // 8 + 1, dtype=torch.int64, device="cuda")
    host = {}
    for mode in ("first", "center"):
        def call(mode=mode):
            check(lib.gf_grid_subsample(ptr(xd), N, args.cell, pointops.GRID_MODES[mode], None, ptr(ws), ptr(out[0]),
                                        ptr(out[1]), ptr(out[2]), ptr(words), stream_ptr()), "gf_grid_subsample")

        dev = device_us(call, args.reps)
        got = pointops.grid_subsample(xd, args.cell, mode)
        t = time.perf_counter()
        host[mode] = postprocess.grid_subsample_host(x, args.cell, mode)
        host_us = (time.perf_counter() - t) * 1e6
        same = all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, host[mode]))
        print(json.dumps({"what": "grid_subsample", "mode": mode, "N": N, "cell": args.cell, "M": int(got[0].shape[0]),
                          "most_in_a_cell": int(host[mode][2].max()), **dev,
                          "host_statement_us": round(host_us, 1), "equal_to_statement": bool(same)}))
    rep = host["center"][0]
    pd = xd[torch.from_numpy(rep).cuda().long()].contiguous()
    n = pd.shape[0]
    idx = torch.empty(N, dtype=torch.int32, device="cuda")
    d2 = torch.empty(N, dtype=torch.float32, device="cuda")
    flag = torch.empty(1, dtype=torch.int32, device="cuda")
    ws = torch.empty(lib.gf_nearest_point_scratch_bytes(n) // 8 + 1, dtype=torch.int64, device="cuda")
    md = 2 * args.cell

    def call():
        check(lib.gf_nearest_point(ptr(xd), N, ptr(pd), n, md, ptr(ws), ptr(idx), ptr(d2), ptr(flag), stream_ptr()),
              "gf_nearest_point")

    dev = device_us(call, args.reps)
    hq = min(args.host_queries, N)
    t = time.perf_counter()
    want = postprocess.nearest_point_host(x[:hq], x[rep], md)
    host_us = (time.perf_counter() - t) * 1e6
    same = np.array_equal(idx[:hq].cpu().numpy(), want[0]) and \
        np.array_equal(d2[:hq].cpu().numpy().view(np.int32), want[1].view(np.int32))
    print(json.dumps({"what": "nearest_point", "Q": N, "n": n, "max_dist": md, "found": int((idx >= 0).sum()),
                      "flag": int(flag.item()), **dev, "host_queries": hq, "host_statement_us": round(host_us, 1),
                      "host_statement_us_scaled_to_Q": round(host_us * N / hq, 1), "equal_to_statement": bool(same)}))


if __name__ == "__main__":
    main()
