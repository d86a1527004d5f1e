#!/usr/bin/env python3
"""Few-shot test (the reference's test_fs.py) on the GPU: geoformer_amd.fs_eval.evaluate_fs.

    python tools/test_fs.py --config config/test_geoformer_fs_scannet.yaml --data-root DATA/scannetv2 \
        --checkpoint model.pth [--test-combs DATA/scannetv2/test_combinations_fold1.pkl] \
        [--support-sets DATA/scannetv2/support_sets/fullscene_fold1_1shot_10sets.pkl]
    python tools/test_fs.py --synthetic 8 [--points 150000] [--runs 10]

The data root holds scenes/*.npy (raw [N, 8] scenes) and scannetv2_val.txt; without pickles the tables are generated
(class2instances from class2instances.pkl, or built from every scene as the reference's builder does).  Prints the
per-run and averaged AP / AP50 / AP25 (evaluation.format_results).

--synthetic N: N S150k-like val scenes (make_raw_scene, boxes of fold 1's classes) with their tables and the FS
golden's synthetic weights; times evaluate_fs (one forward + one requery_many per scene) against the sequential
reference-shaped loop in the same process (one forward per (label, run), then NMS and the evaluator per run), both
with the same support vectors, and prints one JSON line with the scenes/s of both.
"""
import argparse
import json
import os
import pickle
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import geoformer_amd  # noqa: E402

geoformer_amd.configure_runtime()

from geoformer_amd import augment, evaluation, fs_eval  # noqa: E402
from geoformer_amd.postprocess import matrix_non_max_suppression  # noqa: E402


def sequential(m, scenes, ts, vectors, run_num, cvfold):
    """test_fs.py:114-259 as the reference runs it: per (label, run) one forward(remember=(j, k) != (0, 0))."""
    evs = [evaluation.InstanceEvaluator(classes=cvfold) for _ in range(run_num)]
    for n in ts.names:
        ok, _, q, infos = augment.test_merge_fs(scenes, ts, n, fix_support=True, cvfold=cvfold, device="cuda")
        if not ok:
            continue
        cl = [[[], [], []] for _ in range(run_num)]
        for j, l in enumerate(infos["active_label"]):
            for k in range(run_num):
                o = m(None, q, training=False, remember=not (j == 0 and k == 0),
                      support_embeddings=vectors[k][l].unsqueeze(0))["proposal_scores"]
                if o is None or isinstance(o[0], list):
                    continue
                cl[k][0].append(o[1])
                cl[k][1].append(o[0])
                cl[k][2].append(torch.full((o[0].shape[0],), evaluation.BENCHMARK_SEMANTIC_LABELS[l], device="cuda"))
        r = torch.as_tensor(scenes[n], device="cuda")
        gt = evaluation.gt_ids_from_labels(r[:, 6].long(), r[:, 7].long())
        for k in range(run_num):
            if cl[k][0]:
                masks, scores, labels = (torch.cat(x) for x in cl[k])
                pick = matrix_non_max_suppression(masks, scores, labels, final_score_thresh=0.5)
                evs[k].add_scene(n, gt, labels, scores, masks, pick)
    runs = [e.evaluate()[1] for e in evs]
    return runs, evaluation.average_over_runs(runs)


def synthetic(args):
    from geoformer_amd import scene
    from geoformer_amd.model import GeoFormerFS, load_config
    from tests.util import synthetic_state_dict

    z = np.load(os.path.join(ROOT, "tests", "golden", "geoformer_fs_s8k_eval.npz"))
    m = GeoFormerFS(load_config("test_geoformer_fs_scannet.yaml"))
    m.load_state_dict(synthetic_state_dict(m.state_dict(), int(z["weight_seed"])))
    m.semantic_linear.bias.data[3] += float(z["semantic_bias3_shift"])
    m.cuda().eval()
    cv = 1
    cls = augment.FOLD[cv]
    scenes = {}
    for i in range(args.synthetic):
        r = scene.make_raw_scene(args.points, 100 + i)
        on = r[:, 7] >= 0
        ids = np.unique(r[on, 7])
        for k, iid in enumerate(ids):  # the boxes take fold 1's classes in turn
            r[r[:, 7] == iid, 6] = cls[(i + k) % len(cls)]
        scenes[f"scene{800 + i:04d}_00"] = torch.from_numpy(r).cuda()
    index = augment.FSIndex.build(scenes)
    sizes = {}
    for n, r in scenes.items():
        ins = r[:, 7].long()
        for iid in torch.unique(ins[ins >= 0]).tolist():
            sizes[(n, iid)] = int((ins == iid).sum())
    big = max(sizes, key=sizes.get)
    sets = [{c: [list(max(((s, i) for s, i in index.class2instances.get(c, [])), key=lambda t: sizes[tuple(t)],
                          default=big))] for c in cls} for _ in range(args.runs)]
    ts = fs_eval.FSTestSet.build(scenes, list(scenes), index, cv, 1, args.runs, support_sets=sets)
    with torch.no_grad():
        vec = fs_eval.support_vectors(m, scenes, ts, cvfold=cv, run_num=args.runs, k_shot=1)
        first = ts.names[:1]
        fs_eval.evaluate_fs(m, scenes, ts, cvfold=cv, run_num=args.runs, fix_support=True, vectors=vec, names=first)
        torch.cuda.synchronize()
        t = time.perf_counter()
        res = fs_eval.evaluate_fs(m, scenes, ts, cvfold=cv, run_num=args.runs, fix_support=True, vectors=vec)
        torch.cuda.synchronize()
        t_drv = time.perf_counter() - t
        t = time.perf_counter()
        seq_runs, seq_avg = sequential(m, scenes, ts, vec, args.runs, cv)
        torch.cuda.synchronize()
        t_seq = time.perf_counter() - t
    labels = sum(len(ts.combination(n)["active_label"]) for n in ts.names)
    out = {"scenes": len(ts.names), "points": args.points, "runs": args.runs, "label_runs": labels * args.runs,
           "driver_scenes_per_s": len(ts.names) / t_drv, "sequential_scenes_per_s": len(ts.names) / t_seq,
           "speedup": t_seq / t_drv,
           "driver_ap": [res["average"][k] for k in ("all_ap", "all_ap_50%", "all_ap_25%")],
           "sequential_ap": [seq_avg[k] for k in ("all_ap", "all_ap_50%", "all_ap_25%")]}
    print(json.dumps({k: (float(v) if isinstance(v, (np.floating, float)) else v) for k, v in out.items()}))


def real(args):
    from geoformer_amd.model import GeoFormerFS, load_config

    cfg = load_config(args.config)
    root = args.data_root
    with open(os.path.join(root, "scannetv2_val.txt")) as f:
        val = set(f.read().splitlines())
    scenes = {}
    for fn in sorted(os.listdir(os.path.join(root, "scenes"))):
        n = fn.split(".")[0]
        if fn.endswith(".npy"):
            scenes[n] = np.load(os.path.join(root, "scenes", fn), mmap_mode="r")
    names = [n for n in scenes if n in val]
    sets = None
    if args.support_sets and os.path.exists(args.support_sets):
        with open(args.support_sets, "rb") as f:
            sets = pickle.load(f)
    if args.test_combs and os.path.exists(args.test_combs):
        with open(args.test_combs, "rb") as f:
            ts = fs_eval.FSTestSet.from_tables(pickle.load(f), sets)
    else:
        c2i_file = os.path.join(root, "class2instances.pkl")
        if os.path.exists(c2i_file):
            with open(c2i_file, "rb") as f:
                index = augment.FSIndex.from_tables({}, pickle.load(f), {n: 0 for n in scenes})
        else:
            index = augment.FSIndex.build(scenes)
        ts = fs_eval.FSTestSet.build(scenes, names, index, cfg.cvfold, cfg.k_shot, cfg.run_num,
                                     test_seed=getattr(cfg, "test_seed", 567), support_sets=sets)
    m = GeoFormerFS(cfg)
    state = torch.load(args.checkpoint, map_location="cpu")
    sd = state.get("state_dict", state)
    m.load_state_dict({k[len("module."):] if k.startswith("module.") else k: v for k, v in sd.items()}, strict=False)
    m.cuda().eval()
    res = fs_eval.evaluate_fs(m, scenes, ts)
    for k, s in enumerate(res["runs"]):
        print(f"run {k}")
        print(evaluation.format_results(s))
    print(f"average over {len(res['runs'])} runs")
    print(evaluation.format_results(res["average"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="test_geoformer_fs_scannet.yaml")
    ap.add_argument("--data-root")
    ap.add_argument("--test-combs")
    ap.add_argument("--support-sets")
    ap.add_argument("--checkpoint")
    ap.add_argument("--synthetic", type=int, default=0)
    ap.add_argument("--points", type=int, default=150_000)
    ap.add_argument("--runs", type=int, default=10)
    args = ap.parse_args()
    if args.synthetic:
        synthetic(args)
    else:
        if not (args.data_root and args.checkpoint):
            ap.error("--data-root and --checkpoint (or --synthetic N)")
        real(args)


if __name__ == "__main__":
    main()
