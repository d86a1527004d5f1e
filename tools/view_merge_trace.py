"""The join of instances across views (csrc/view_merge.hip), timed launch by launch, and what views= costs the loop:

    python tools/view_merge_trace.py                      # the join chain, one JSON line
    python tools/view_merge_trace.py --what loop          # predict_batches with and without views=Views(rotations=4)

--what chain: one scene of --points points (default 150 000) under --views views (8) of --picks picked rows (50) each,
synthetic rows (tests/view_merge_cases.synthetic_rows: every view sees a random choice of 60 interval objects with
jittered ends).  view_merge.view_pack, view_overlaps, view_best, view_merge and view_assemble are each timed with events
around the call, tables and inputs already on the device: min / median / max microseconds over --reps calls after 5
warm-ups; `merge_views` is the whole of postprocess.merge_views (uploads, the five calls and the read of G), `host` the
numpy statement on the same input (one call, wall clock).  The outputs are compared with the statement once.
overlap_pairs: the row pairs times words the overlap kernel forms (the blocks of the upper triangle, padded to 64 rows),
and overlap_Gpairs_per_s their rate, beside the VALU bound of one v_and_b32 and one v_bcnt_u32_b32 per pair:
256 CUs x 4 SIMDs x 32 lanes per cycle x 2.4 GHz / 2 instructions = 39.3 T pairs / s.
--what loop: batch_eval.predict_batches over --scenes synthetic scenes (scene.make_raw_scene(--points, 500 + i), the
scenes of tools/batched_eval.py) at --batch-size 4, plain and with views=Views(rotations=4), alternating, wall clock
around each pass after one warm-up pass each; the join's share is timed by running the same views as plain scenes.
--nms-score X is the loop's final_score_thresh: at the default 0.5 the benchmark's synthetic model picks nothing and the
join has no rows; at 0 every view keeps its proposals and the join runs over V x 256 rows."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VALU_PAIRS_PER_S = 256 * 4 * 32 * 2.4e9 / 2


def timed(fn, reps):
    for _ in range(5):
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


def chain(args):
    from geoformer_amd import pointops, postprocess, view_merge
    from tests.view_merge_cases import synthetic_rows

    c = synthetic_rows(1, args.points, args.views, args.picks)
    N, V = c["N"], args.views
    t = time.perf_counter()
    want = postprocess.merge_views_host(c["per_view"], N, return_tables=True)
    host_s = time.perf_counter() - t
    dev = [tuple(torch.from_numpy(x).cuda() for x in v) for v in c["per_view"]]
    rows = [(m, p, k, s) for k, s, m, p in dev]
    table, sizes = postprocess.view_scene_table(rows, N)
    P = sizes["rows"]
    table_d = pointops._table_dev(table, "cuda")
    row_view, view_first = (torch.from_numpy(sizes[k]).cuda() for k in ("row_view", "view_first"))
    cls_all = torch.cat([k[p] for _, p, k, _ in rows]).contiguous()
    sc_all = torch.cat([s[p] for _, p, _, s in rows]).contiguous()
    mv = (V + 1) // 2
    bits, cnt = view_merge.view_pack(table_d, table, N)
    inter = view_merge.view_overlaps(bits, N)
    best = view_merge.view_best(inter, cnt, cls_all, row_view, view_first)
    merged = view_merge.view_merge(inter, cnt, best, cls_all, sc_all, row_view, 0.5, mv)
    G = int(merged["G"].item())
    masks, count = view_merge.view_assemble(bits, merged, row_view, G, N, 0.5)
    got = postprocess.merge_views(dev, N, return_tables=True)
    for g, w in zip((got[0], got[1], got[2], got[3], masks, inter), (*want[:4], want[2], want[4]["inter"])):
        assert torch.equal(g.cpu(), torch.from_numpy(w))
    W, nb = (N + 31) // 32, (P + 63) // 64
    pairs = nb * (nb + 1) // 2 * 64 * 64 * W
    out = {"tool": "view_merge_trace", "points": N, "views": V, "rows": P, "instances": G,
           "joined_rows": int(P - np.unique(want[4]["comp"]).size), "words": W,
           "us": {"pack": timed(lambda: view_merge.view_pack(table_d, table, N), args.reps),
                  "overlaps": timed(lambda: view_merge.view_overlaps(bits, N), args.reps),
                  "best": timed(lambda: view_merge.view_best(inter, cnt, cls_all, row_view, view_first), args.reps),
                  "merge": timed(lambda: view_merge.view_merge(inter, cnt, best, cls_all, sc_all, row_view, 0.5, mv), args.reps),
                  "assemble": timed(lambda: view_merge.view_assemble(bits, merged, row_view, G, N, 0.5), args.reps),
                  "read_G": timed(lambda: merged["G"].item(), args.reps),
                  "merge_views": timed(lambda: postprocess.merge_views(dev, N), args.reps)},
           "host_ms": round(host_s * 1e3, 1), "overlap_pairs": pairs}
    out["us"]["five_calls_median_sum"] = round(sum(out["us"][k][1] for k in ("pack", "overlaps", "best", "merge", "assemble")), 1)
    rate = pairs / (out["us"]["overlaps"][1] * 1e-6)
    out["overlap_Gpairs_per_s"] = round(rate / 1e9, 1)
    out["overlap_fraction_of_valu_bound"] = round(rate / VALU_PAIRS_PER_S, 4)
    print(json.dumps(out))


def loop(args):
    import bench
    from geoformer_amd import batch_eval, scene

    dev = torch.device("cuda")
    items = [(f"synthetic{i:04d}", scene.make_raw_scene(args.points, 500 + i)) for i in range(args.scenes)]
    probe = scene.make_batch([batch_eval.scene_dict(items[0][1])])
    model = bench.build_model(dev, probe_batch=bench.to_device(probe, dev))
    views = batch_eval.Views(rotations=4)
    expanded = batch_eval.view_items(items, views)

    def run(its, **kw):
        if args.nms_score is not None:
            kw["final_score_thresh"] = args.nms_score
        np.random.seed(0)
        n = sum(int(pick.numel()) for *_, pick in batch_eval.predict_batches(model, its, args.batch_size, **kw))
        torch.cuda.synchronize()
        return n

    configs = [("plain", lambda: run(items)), ("views4", lambda: run(items, views=views)),
               ("views4_without_the_join", lambda: run(expanded))]
    picks = {name: fn() for name, fn in configs}
    times = {name: [] for name, _ in configs}
    for _ in range(args.reps):
        for name, fn in configs:
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t)
    med = {k: float(np.median(v)) for k, v in times.items()}
    print(json.dumps({"tool": "view_merge_trace", "what": "loop", "scenes": args.scenes, "points": args.points,
                      "batch_size": args.batch_size, "reps": args.reps, "nms_score": args.nms_score, "picks": picks,
                      "scenes_per_s": {k: round(args.scenes / v, 3) for k, v in med.items()},
                      "s_per_pass_all_reps": {k: [round(x, 3) for x in v] for k, v in times.items()},
                      "views4_over_plain": round(med["plain"] / med["views4"], 4),
                      "join_ms_per_scene": round(1e3 * (med["views4"] - med["views4_without_the_join"]) / args.scenes, 2)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=("chain", "loop"), default="chain")
    ap.add_argument("--points", type=int, default=150_000)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--picks", type=int, default=50)
    ap.add_argument("--scenes", type=int, default=8)
    ap.add_argument("--batch-size", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--nms-score", type=float, default=None)
    args = ap.parse_args()

    import geoformer_amd

    geoformer_amd.configure_runtime()
    (chain if args.what == "chain" else loop)(args)


if __name__ == "__main__":
    main()
