"""Scenes per second of the batched eval forward (forward(..., all_scenes=True) + postprocess.matrix_nms_batched) for
B in {1, 2, 4, 8} against the one-scene path (forward + postprocess.matrix_non_max_suppression per scene), on distinct
150k-point synthetic scenes (scene.make_scene) and the benchmark model (bench.build_model).  The batches are uploaded
before the clock starts.  The configurations alternate within every repetition, in one process; each pass covers the
same scenes and is timed with device events (from the first launch to the last pick on the host).  Prints one JSON line.

    timeout -k 10 600 python tools/batched_eval.py [--points 150000] [--scenes 8] [--reps 5] [--warmup 2]
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
    ap.add_argument("--scenes", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="1,2,4,8")
    args = ap.parse_args()

    import geoformer_amd

    geoformer_amd.configure_runtime()
    import bench
    from geoformer_amd import evaluation, postprocess, scene

    dev = torch.device("cuda")
    sizes = [int(s) for s in args.sizes.split(",")]
    scenes = [scene.make_scene(args.points, 500 + i) for i in range(args.scenes)]

    def to_dev(b):
        return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in b.items()}

    probe = to_dev(scene.make_batch(scenes[:1]))
    model = bench.build_model(dev, probe_batch=probe)
    cvfold = model.cfg.cvfold
    batches = {B: [to_dev(scene.make_batch(scenes[i:i + B])) for i in range(0, len(scenes), B)] for B in sizes}
    torch.cuda.synchronize()

    def one_scene_pass():
        n = 0
        for b in batches[1]:
            out = model(b, 300, training=False)
            cls, sc, masks = out.get("proposal_scores", ([], [], []))
            if torch.is_tensor(cls):
                ids = evaluation.benchmark_label_ids(cls, cvfold)
                n += int(postprocess.matrix_non_max_suppression(masks, sc, ids, final_score_thresh=0.5).numel())
        return n

    def batched_pass(B):
        n = 0
        for b in batches[B]:
            per = model(b, 300, training=False, all_scenes=True).get("proposal_scores_per_scene", [])
            ids = [evaluation.benchmark_label_ids(c, cvfold) if torch.is_tensor(c) else [] for c, _, _ in per]
            picks = postprocess.matrix_nms_batched([m for _, _, m in per], [s for _, s, _ in per], ids,
                                                   final_score_thresh=0.5)
            n += sum(int(p.numel()) for p in picks)
        return n

    configs = [("one_scene_path", one_scene_pass)] + [(f"B{B}", (lambda B=B: batched_pass(B))) for B in sizes]
    picks = {}
    for _ in range(args.warmup):
        for name, fn in configs:
            np.random.seed(0)
            picks[name] = fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in configs}
    for _ in range(args.reps):
        for name, fn in configs:
            np.random.seed(0)
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            h0 = time.perf_counter()
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            times[name].append((t0.elapsed_time(t1) / 1e3, time.perf_counter() - h0))
    res = {}
    for name, ts in times.items():
        dev_s = float(np.median([t[0] for t in ts]))
        res[name] = {"scenes_per_s": round(args.scenes / dev_s, 2), "ms_per_scene": round(1e3 * dev_s / args.scenes, 3),
                     "ms_per_scene_all_reps": [round(1e3 * t[0] / args.scenes, 3) for t in ts],
                     "host_wall_ms_per_scene": round(1e3 * float(np.median([t[1] for t in ts])) / args.scenes, 3),
                     "picks": picks[name]}
    print(json.dumps({"tool": "batched_eval", "points": args.points, "scenes": args.scenes, "reps": args.reps,
                      "warmup": args.warmup, "timing": "median over reps of one pass, device events; configs "
                      "alternate within each rep", "results": res}))


if __name__ == "__main__":
    main()
