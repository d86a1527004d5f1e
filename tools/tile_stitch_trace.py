"""The tile stitch kernel (csrc/tile_stitch.hip) beside the same gather written as a plain framework expression, timed
with events around each call:

    python tools/tile_stitch_trace.py                      # both modes, kernel and framework form, one JSON line each
    rocprofv3 --kernel-trace --stats -d artifacts/tile_stitch -- python tools/tile_stitch_trace.py --what kernel

The scan is DESIGN.md §18's: the benchmark generator's room (scene.make_raw_scene(--points, 1234)) placed 2 x 2 with
0.1 m between the copies, 601 076 points at the default 150 000, Tiling(max_points=100_000): T = 8.  Every tile gets
standard normal scores fp32 [n_s, C] (C = --classes, default the 13 of the test config).
--what kernel: pointops.tile_stitch_scores with the tables already on the device (one launch per call), and
postprocess.stitch_tiles as a whole (the table and the plan's three tables uploaded per call).
--what torch: the yardstick.  core: torch.cat(scores)[index] with the int64 index prepared once (a concatenation and an
indexed gather: 2 launches).  mean: the concatenation, four indexed gathers, three masked adds (an add and a where each)
and a division: 12 launches.
Each figure is min / median / max over --reps calls after 5 warm-ups.  The plain figures repeat the call on the same
working set (84 - 100 MB at the defaults: resident in the 256 MiB Infinity Cache after the first call); the *_cold
figures overwrite a 1 GiB buffer on the stream before every timed call, so the inputs come from HBM, as they do for
the one stitch of a scan in the loops.  Both forms are compared bit for bit with
postprocess.stitch_tiles_host once.  bytes: the plan's tables (32 N, + 4 N core_of in core mode, + 16 T), the source
rows read (4 C per slot that counts) and the output (4 C N)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 8e12


def make_scan(points):
    from geoformer_amd import scene

    r = scene.make_raw_scene(points, 1234)
    ex = r[:, :3].max(0) - r[:, :3].min(0)
    parts = []
    for iy in range(2):
        for ix in range(2):
            q = r.copy()
            q[:, 0] += ix * (ex[0] + 0.1)
            q[:, 1] += iy * (ex[1] + 0.1)
            parts.append(q)
    return np.concatenate(parts)


def timed(fn, reps, flush=None):
    """min / median / max microseconds of fn over reps calls after 5 warm-ups, events around each call.  flush: a device
    buffer larger than the 256 MiB Infinity Cache that is overwritten on the stream before every timed call, so that the
    call reads its inputs from HBM."""
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if flush is not None:
            flush.add_(1)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    us.sort()
    return [round(us[0], 1), round(us[len(us) // 2], 1), round(us[-1], 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=("both", "kernel", "torch"), default="both")
    ap.add_argument("--points", type=int, default=150_000)
    ap.add_argument("--classes", type=int, default=13)
    ap.add_argument("--tile-max-points", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()

    import geoformer_amd

    geoformer_amd.configure_runtime()
    from geoformer_amd import batch_eval, pointops, postprocess

    C = args.classes
    plan = batch_eval.Tiling(max_points=args.tile_max_points).plan_of(make_scan(args.points))
    N, T = plan.N, plan.T
    rng = np.random.default_rng(3)
    sizes = np.diff(plan.offsets)
    host = [rng.standard_normal((int(n), C)).astype(np.float32) for n in sizes]
    scores = [torch.from_numpy(x).cuda() for x in host]
    valid = plan.tile_of >= 0
    counts = valid.sum(1)
    head = {"points": N, "tiles": T, "classes": C, "tile_points": [int(sizes.min()), int(sizes.max())],
            "points_in_1_2_4_tiles": [int((counts == k).sum()) for k in (1, 2, 4)]}
    print(json.dumps(head))
    table = np.array([[x.data_ptr(), x.shape[0]] for x in scores], np.int64)
    table_d = pointops._table_dev(table, "cuda")
    tile_of, local_of = torch.from_numpy(plan.tile_of).cuda(), torch.from_numpy(plan.local_of).cuda()
    core_of = torch.from_numpy(plan.core_of).cuda()
    # the framework form's indices, prepared once: the row of every slot in the concatenation, and of the core slot
    rows = np.where(valid, plan.offsets[np.clip(plan.tile_of, 0, T - 1)] + plan.local_of, 0)
    core_slot = (plan.tile_of == plan.core_of[:, None]).argmax(1)
    idx_core = torch.from_numpy(rows[np.arange(N), core_slot]).cuda()
    idx = [torch.from_numpy(np.ascontiguousarray(rows[:, j])).cuda() for j in range(4)]
    mask = [torch.from_numpy(np.ascontiguousarray(valid[:, j])).cuda()[:, None] for j in range(4)]
    cnt = torch.from_numpy(counts.astype(np.float32)).cuda()[:, None]
    flush = torch.zeros(1 << 28, dtype=torch.int32, device="cuda")  # 1 GiB: four times the Infinity Cache

    def torch_core():
        return torch.cat(scores)[idx_core]

    def torch_mean():
        flat = torch.cat(scores)
        acc = flat[idx[0]]  # (every point of a tile_plan has its first slot)
        for j in range(1, 4):
            acc = torch.where(mask[j], acc + flat[idx[j]], acc)
        return acc / cnt

    for mode in ("core", "mean"):
        want = torch.from_numpy(postprocess.stitch_tiles_host(plan, host, mode)).view(torch.int32)
        slots = N if mode == "core" else int(counts.sum())
        nbytes = 32 * N + (4 * N if mode == "core" else 0) + 16 * T + 4 * C * slots + 4 * C * N
        out = {"mode": mode, "bytes": nbytes}
        if args.what in ("both", "kernel"):
            def kernel():
                return pointops.tile_stitch_scores(table_d, table, tile_of, local_of, core_of, C, mode)

            assert torch.equal(kernel().cpu().view(torch.int32), want)
            out["kernel_us"] = timed(kernel, args.reps)
            out["kernel_GBps"] = round(nbytes / out["kernel_us"][1] / 1e3, 1)
            out["kernel_cache_warm_bytes_over_hbm_peak"] =round(nbytes / (out["kernel_us"][1] * 1e-6) / HBM_BYTES_PER_S, 3)
            out["kernel_cold_us"] = timed(kernel, args.reps, flush)
            out["kernel_cold_GBps"] = round(nbytes / out["kernel_cold_us"][1] / 1e3, 1)
            out["kernel_cold_fraction_of_hbm_peak"] = round(nbytes / (out["kernel_cold_us"][1] * 1e-6) / HBM_BYTES_PER_S, 3)
            out["stitch_tiles_us"] = timed(lambda: postprocess.stitch_tiles(plan, scores, mode), args.reps)
        if args.what in ("both", "torch"):
            fn = torch_core if mode == "core" else torch_mean
            assert torch.equal(fn().cpu().view(torch.int32), want)
            out["torch_us"] = timed(fn, args.reps)
            out["torch_cold_us"] = timed(fn, args.reps, flush)
            out["torch_launches"] = 2 if mode == "core" else 12
        print(json.dumps(out))


if __name__ == "__main__":
    main()
