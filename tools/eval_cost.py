"""Per-scene cost of the instance evaluation's scene step (InstanceEvaluator.add_scene): device tensors (one
gf_instance_overlaps call + one device-to-host copy of the tables) against the host path (the picked masks copied to
the host, then the numpy overlap count), on S150k synthetic scenes with 40 picked masks of 64 proposals and about 40
ground-truth instances.  Prints one JSON line.

    timeout -k 10 300 python tools/eval_cost.py [--points 150000] [--scenes 8] [--reps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def synthetic_scene(rng, N, n_inst=40, n_prop=64, n_pick=40):
    from geoformer_amd import evaluation as E

    cls = np.asarray(E.FOLD_CLASS_IDS[0], dtype=np.int64)
    owner = rng.integers(-1, n_inst, N)  # -1: void (unannotated / floor / wall)
    inst_id = cls[rng.integers(0, len(cls), n_inst)] * 1000 + np.arange(1, n_inst + 1)
    gt = np.where(owner >= 0, inst_id[np.maximum(owner, 0)], rng.choice(np.array([0, 1001, 2002]), N))
    masks = np.zeros((n_prop, N), dtype=np.int32)
    for r in range(n_prop):  # a proposal: most of one instance and a sprinkle of other points
        masks[r] = (owner == r % n_inst) & (rng.random(N) < 0.8) | (rng.random(N) < 0.01)
    labels = np.where(rng.random(n_prop) < 0.9, inst_id[np.arange(n_prop) % n_inst] // 1000, 1)
    scores = rng.random(n_prop).astype(np.float32)
    pick = rng.permutation(n_prop)[:n_pick]
    return gt.astype(np.int64), masks, labels.astype(np.int64), scores, pick


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=150_000)
    ap.add_argument("--scenes", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()

    import torch

    import geoformer_amd
    from geoformer_amd import evaluation as E

    geoformer_amd.configure_runtime()
    if not torch.cuda.is_available():
        raise SystemExit("eval_cost.py measures the GPU path: no GPU")
    torch.cuda.set_device(0)
    rng = np.random.default_rng(0)
    host = [synthetic_scene(rng, args.points) for _ in range(args.scenes)]
    dev = [tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in s) for s in host]
    torch.cuda.synchronize()

    def device_pass():
        ev = E.InstanceEvaluator(classes=0)
        for i, (gt, masks, labels, scores, pick) in enumerate(dev):
            ev.add_scene(f"s{i}", gt, labels, scores, masks, pick=pick)  # ends in the tables' device-to-host copy
        return ev

    def host_pass():
        ev = E.InstanceEvaluator(classes=0)
        copy = 0.0
        for i, (gt, masks, labels, scores, pick) in enumerate(dev):
            t = time.perf_counter()
            m = masks[pick].cpu().numpy()  # what test.py copies: masks_final[pick].cpu().numpy()
            s, lab, g = scores[pick].cpu().numpy(), labels[pick].cpu().numpy(), gt.cpu().numpy()
            copy += time.perf_counter() - t
            ev.add_scene(f"s{i}", g, lab, s, m)
        return ev, copy

    device_pass(), host_pass()  # warm-up: code objects, allocator blocks, pinned staging
    torch.cuda.synchronize()
    k = args.scenes
    td, th, tc = [], [], []
    for _ in range(args.reps):
        t = time.perf_counter()
        evd = device_pass()
        td.append(time.perf_counter() - t)
        t = time.perf_counter()
        evh, copy = host_pass()
        th.append(time.perf_counter() - t)
        tc.append(copy)
    apd, aph = evd.evaluate()[0], evh.evaluate()[0]
    same = bool(np.array_equal(apd, aph, equal_nan=True))
    t = time.perf_counter()
    evd.evaluate()
    t_eval = time.perf_counter() - t
    print(json.dumps({
        "metric": "instance evaluation, per-scene step (add_scene)", "points": args.points, "scenes": k,
        "picked_masks": 40, "gt_instances": 40, "reps": args.reps,
        "device_ms_per_scene_median": round(float(np.median(td)) / k * 1e3, 3),
        "device_ms_per_scene_min": round(float(np.min(td)) / k * 1e3, 3),
        "host_ms_per_scene_median": round(float(np.median(th)) / k * 1e3, 3),
        "host_copy_ms_per_scene_median": round(float(np.median(tc)) / k * 1e3, 3),
        "speedup_median": round(float(np.median(th)) / float(np.median(td)), 1),
        "dataset_matching_ms_for_all_scenes": round(t_eval * 1e3, 3),
        "ap_device_equals_host": same,
        "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
