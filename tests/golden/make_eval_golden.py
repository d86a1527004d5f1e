"""Generates tests/golden/scannet_eval.npz by running the REFERENCE's own util/eval.py (ScanNet instance evaluation) on
synthetic scenes.  Run in the build container only (needs /root/reference):
    python tests/golden/make_eval_golden.py
One child process per class set (util/config.py parses argv and util/eval.py picks its class globals from cfg.cvfold at
import): fold 0 and fold 1 from the reference's test yamls, "all" with the module's class globals patched to the 18
benchmark classes.  numpy >= 1.24 lacks np.float, which util/eval.py uses: a `np.float = float` shim stands in.

Stored (data only): the scenes' inputs -- gt_ids, the picked masks as index lists, their labels and float32 scores --
and per class set the AP array [1, C, n_overlaps], compute_averages' numbers, a JSON digest of every scene's
assign_instances_for_scan result, and the run average of two "runs" (all predictions, every other prediction).
The scenes cover: a mask below 100 points, a label outside the class set, two and three predictions on one instance,
a prediction mostly over void, a prediction over an instance below 100 points, an IoU of exactly 0.5 (and an ignore
proportion of exactly 0.5), confidences tied within and across scenes, a scene without predictions, per class set a
class with instances but no prediction and a class with neither, gt ids of 0, of labels outside the class set and
negative ids.
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
OUT = os.path.join(HERE, "scannet_eval.npz")
CLASS_SETS = {"0": "config/test_geoformer_scannet.yaml", "1": "config/test_geoformer_fs_scannet.yaml",
              "all": "config/test_geoformer_scannet.yaml"}
ALL_IDS = [3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39]
ALL_NAMES = ["cabinet", "bed", "chair", "sofa", "table", "door", "window", "bookshelf", "picture", "counter", "desk",
             "curtain", "refrigerator", "shower curtain", "toilet", "sink", "bathtub", "otherfurniture"]
GT_ONLY = (36, 39)    # instances, never predicted
NEVER = (16, 28)      # neither instances nor predictions
PRED_LABELS = [c for c in ALL_IDS if c not in GT_ONLY + NEVER]


def make_scenes():
    """[(name, gt_ids int64 [N], masks uint8 [n, N], labels int64 [n], scores float32 [n])]"""
    rng = np.random.default_rng(20261015)
    scenes = []
    for si, N in enumerate((5000, 9000, 12000, 16000, 20000, 7000)):
        ids = np.zeros(N, dtype=np.int64)  # 0: unannotated
        insts = []  # (id, first, size)

        def put(label, size):
            first = insts[-1][1] + insts[-1][2] if insts else 0
            iid = label * 1000 + len(insts) + 1
            ids[first:first + size] = iid
            insts.append((iid, first, size))
            return len(insts) - 1

        for _ in range(rng.integers(6, 12)):
            put(int(rng.choice(PRED_LABELS)), int(rng.integers(150, max(200, N // 14))))
        small_gt = put(5, 60)                # an instance below 100 points
        half = put(4, 200)                   # an IoU of exactly 0.5
        gt_only = put(GT_ONLY[si % 2], 300)  # a class with instances and no prediction
        wall = put(1, 400)                   # a label outside every class set
        cur = insts[-1][1] + insts[-1][2]
        floor = int(N * 0.05)
        ids[cur:cur + floor] = 2000 + si
        cur += floor
        ids[cur:cur + 40] = rng.choice(np.array([-1, -999, -1000, -3001, -36001]), 40)  # negative ids: void
        void_lo = cur + 40  # the rest stays 0 (unannotated)
        special = (small_gt, half, gt_only, wall)

        preds = []  # (member indices in the unpermuted scene, label, score)

        def score():
            return np.float32(rng.integers(1, 33) / 32.0)  # few distinct values: ties within and across scenes

        for j, (iid, first, size) in enumerate(insts):
            if j in special or rng.random() < 0.25:
                continue
            for _ in range(1 if rng.random() < 0.7 else int(rng.integers(2, 4))):  # two or three on one instance
                keep = rng.random(size) < rng.uniform(0.35, 1.0)
                mem = first + np.nonzero(keep)[0]
                extra = rng.choice(N, int(rng.integers(0, size // 2 + 1)), replace=False)
                lab = iid // 1000 if rng.random() < 0.85 else int(rng.choice(PRED_LABELS))
                preds.append((np.union1d(mem, extra), lab, score()))
        if si != 5:
            _, f, s = insts[half]
            preds.append((np.arange(f, f + s // 2), 4, score()))                       # IoU 100 / 200 = 0.5
            _, f, s = insts[small_gt]
            preds.append((np.concatenate([np.arange(f, f + s), np.arange(void_lo, void_lo + 50)]), 5, score()))
            _, f, s = insts[0]
            preds.append((np.arange(f, f + 60), int(ids[f] // 1000), score()))          # a mask below 100 points
            _, f, s = insts[wall]
            preds.append((np.arange(f, f + s), 1, score()))                             # label outside the class set
            _, f, s = insts[1]
            preds.append((np.concatenate([np.arange(void_lo, void_lo + 250), np.arange(f, f + 50)]),
                          int(ids[f] // 1000), score()))                                # mostly over void
            preds.append((np.concatenate([np.arange(void_lo + 300, void_lo + 400), np.arange(f + 50, f + 150)]),
                          int(ids[f] // 1000), score()))                                # ignore proportion 0.5
            preds.append((np.arange(0, 0), 3, score()))                                 # an empty mask
        else:
            preds = []  # a scene without predictions
        perm = rng.permutation(N)
        inv = np.empty(N, dtype=np.int64)
        inv[perm] = np.arange(N)
        gt = ids[perm]
        masks = np.zeros((len(preds), N), dtype=np.uint8)
        for i, (mem, _, _) in enumerate(preds):
            masks[i, inv[np.asarray(mem, dtype=np.int64)]] = 1
        order = rng.permutation(len(preds))
        masks = masks[order]
        labels = np.array([preds[i][1] for i in order], dtype=np.int64)
        scores = np.array([preds[i][2] for i in order], dtype=np.float32)
        scenes.append((f"scene{si:04d}_00", gt, masks, labels, scores))
    return scenes


def pack(scenes):
    d = {"scene_names": np.array([s[0] for s in scenes])}
    for i, (name, gt, masks, labels, scores) in enumerate(scenes):
        r, p = np.nonzero(masks)
        d[f"s{i}_gt_ids"] = gt
        d[f"s{i}_mask_offsets"] = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=masks.shape[0]))]).astype(np.int32)
        d[f"s{i}_mask_points"] = p.astype(np.int32)
        d[f"s{i}_labels"] = labels
        d[f"s{i}_scores"] = scores
    return d


def child(which, out_path):
    sys.argv = ["make_eval_golden", "--config", os.path.join(REF, CLASS_SETS[which])]
    np.float = float  # util/eval.py: np.zeros(..., np.float)
    sys.path.insert(0, REF)
    os.chdir(REF)
    import util.eval as ev

    if which == "all":
        ev.CLASS_LABELS = list(ALL_NAMES)
        ev.VALID_CLASS_IDS = np.array(ALL_IDS)
        ev.ID_TO_LABEL = dict(zip(ev.VALID_CLASS_IDS, ev.CLASS_LABELS))
        ev.LABEL_TO_ID = dict(zip(ev.CLASS_LABELS, ev.VALID_CLASS_IDS))
    else:
        assert ev.cfg.cvfold == int(which)
    scenes = make_scenes()

    def run(keep_every):
        matches, digest = {}, {}
        for name, gt, masks, labels, scores in scenes:
            sel = np.arange(0, masks.shape[0], keep_every)
            info = {"conf": scores[sel], "label_id": labels[sel], "mask": masks[sel].astype(np.int64)}
            gt2pred, pred2gt = ev.assign_instances_for_scan(name, info, gt)
            matches[name] = {"gt": gt2pred, "pred": pred2gt}
            digest[name] = {
                "gt": {lab: [[int(g["instance_id"]), int(g["vert_count"]),
                              [[p["pred_id"], int(p["intersection"])] for p in g["matched_pred"]]] for g in v]
                       for lab, v in gt2pred.items()},
                "pred": {lab: [[p["pred_id"], int(p["label_id"]), int(p["vert_count"]), float(p["confidence"]),
                                int(p["void_intersection"]),
                                [[int(g["instance_id"]), int(g["intersection"])] for g in p["matched_gt"]]] for p in v]
                         for lab, v in pred2gt.items()}}
        ap = ev.evaluate_matches(matches)
        return ap, ev.compute_averages(ap), digest

    ap, avgs, digest = run(1)
    ap2, avgs2, _ = run(2)
    runs = ev.compute_averages_over_runs(ev.accumulate_averages_over_runs(ev.accumulate_averages_over_runs({}, avgs), avgs2))

    def flat(a, keys=("all_ap", "all_ap_50%", "all_ap_25%")):
        return np.array([a[k] for k in keys] + [a["classes"][c][k] for c in ev.CLASS_LABELS for k in ("ap", "ap50%", "ap25%")])

    np.savez(out_path, ap=ap, averages=flat(avgs), ap_half=ap2,
             run_average=flat(runs, ("all_ap", "all_ap_50%", "all_ap_25%", "all_ap_std", "all_ap_50%_std", "all_ap_25%_std")),
             class_names=np.array(ev.CLASS_LABELS), class_ids=np.array(ev.VALID_CLASS_IDS),
             digest=np.array(json.dumps(digest)))


def main():
    d = pack(make_scenes())
    with tempfile.TemporaryDirectory() as tmp:
        for which in CLASS_SETS:
            path = os.path.join(tmp, f"{which}.npz")
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", which, path], check=True)
            z = np.load(path)
            for k in z.files:
                d[f"{which}_{k}"] = z[k]
    np.savez_compressed(OUT, **d)
    print(OUT, os.path.getsize(OUT), "bytes")
    for which in CLASS_SETS:
        print(which, d[f"{which}_averages"][:3], "nan classes:", int(np.isnan(d[f"{which}_ap"][0, :, 0]).sum()))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3])
    else:
        main()
