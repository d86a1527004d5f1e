"""geoformer_amd.evaluation (numpy path) against the reference's own ScanNet instance evaluation, run on synthetic scenes
by tests/golden/make_eval_golden.py: AP arrays, averages, run averages and the per-scene assignment, for cvfold 0 / 1 and
the 18-class set."""
import json
import os

import numpy as np
import pytest

from geoformer_amd import evaluation as E

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scannet_eval.npz")
SETS = {"0": 0, "1": 1, "all": "all"}


@pytest.fixture(scope="module")
def golden():
    return np.load(G)


def scenes(z):
    """[(name, gt_ids, masks int32 [n, N], labels, scores)] of the fixture."""
    out = []
    for i, name in enumerate(z["scene_names"]):
        gt = z[f"s{i}_gt_ids"]
        off, pts = z[f"s{i}_mask_offsets"], z[f"s{i}_mask_points"]
        masks = np.zeros((len(off) - 1, gt.shape[0]), dtype=np.int32)
        for r in range(len(off) - 1):
            masks[r, pts[off[r]:off[r + 1]]] = 1
        out.append((str(name), gt, masks, z[f"s{i}_labels"], z[f"s{i}_scores"]))
    return out


def flat(avgs, names, keys=("all_ap", "all_ap_50%", "all_ap_25%")):
    return np.array([avgs[k] for k in keys] + [avgs["classes"][c][k] for c in names for k in ("ap", "ap50%", "ap25%")])


def same(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    assert (np.isnan(got) == np.isnan(want)).all()
    ok = ~np.isnan(want)
    assert np.abs(got[ok] - want[ok]).max(initial=0.0) <= 1e-12


@pytest.mark.parametrize("which", list(SETS))
def test_instance_evaluator_host_path(golden, which):
    ev = E.InstanceEvaluator(classes=SETS[which])
    assert list(ev.class_names) == list(golden[f"{which}_class_names"])
    assert (ev.class_ids == golden[f"{which}_class_ids"]).all()
    for name, gt, masks, labels, scores in scenes(golden):
        ev.add_scene(name, gt, labels, scores, masks)
    ap, avgs = ev.evaluate()
    same(ap, golden[f"{which}_ap"][0])
    same(flat(avgs, ev.class_names), golden[f"{which}_averages"])
    assert np.isnan(ap).any() and (ap == 0).any()  # a class with neither, and one with instances but no prediction
    text = ev.format_results(avgs)
    assert "average" in text and ev.class_names[0] in text


@pytest.mark.parametrize("which", list(SETS))
def test_pick_and_run_average(golden, which):
    """Every other prediction selected through `pick` (unsorted rows of a larger mask set) reproduces the reference's
    second run; average_over_runs of the two reproduces compute_averages_over_runs."""
    runs = []
    for half in (False, True):
        ev = E.InstanceEvaluator(classes=SETS[which])
        for name, gt, masks, labels, scores in scenes(golden):
            if half:
                sel = np.arange(0, masks.shape[0], 2)
                perm = np.random.default_rng(len(name)).permutation(masks.shape[0])
                pos = np.argsort(perm)  # row of original mask r in the shuffled set
                ev.add_scene(name, gt, labels[perm], scores[perm], masks[perm], pick=pos[sel])
            else:
                ev.add_scene(name, gt, labels, scores, masks)
        ap, avgs = ev.evaluate()
        runs.append(avgs)
    same(ap, golden[f"{which}_ap_half"][0])
    avg = E.average_over_runs(runs)
    keys = ("all_ap", "all_ap_50%", "all_ap_25%", "all_ap_std", "all_ap_50%_std", "all_ap_25%_std")
    same(flat(avg, list(golden[f"{which}_class_names"]), keys), golden[f"{which}_run_average"])


@pytest.mark.parametrize("which", list(SETS))
def test_compatibility_functions_layer_by_layer(golden, which):
    digest = json.loads(str(golden[f"{which}_digest"]))
    matches = {}
    for name, gt, masks, labels, scores in scenes(golden):
        gt2pred, pred2gt = E.assign_instances_for_scan(name, {"conf": scores, "label_id": labels, "mask": masks}, gt,
                                                       classes=SETS[which])
        want = digest[name]
        got_gt = {lab: [[g["instance_id"], g["vert_count"], [[p["pred_id"], p["intersection"]] for p in g["matched_pred"]]]
                        for g in v] for lab, v in gt2pred.items()}
        got_pred = {lab: [[p["pred_id"], p["label_id"], p["vert_count"], float(p["confidence"]), p["void_intersection"],
                           [[g["instance_id"], g["intersection"]] for g in p["matched_gt"]]] for p in v]
                    for lab, v in pred2gt.items()}
        assert got_gt == want["gt"], name
        assert got_pred == want["pred"], name
        matches[name] = {"gt": gt2pred, "pred": pred2gt}
    ap = E.evaluate_matches(matches, classes=SETS[which])
    same(ap, golden[f"{which}_ap"])
    same(flat(E.compute_averages(ap, classes=SETS[which]), list(golden[f"{which}_class_names"])),
         golden[f"{which}_averages"])


def test_fixture_covers_the_edge_cases(golden):
    sc = scenes(golden)
    assert any(m.shape[0] == 0 for _, _, m, _, _ in sc)  # a scene without predictions
    gt = np.concatenate([g for _, g, _, _, _ in sc])
    assert (gt == 0).any() and (gt < 0).any() and ((gt // 1000 == 1) | (gt // 1000 == 2)).any()
    scores = [s for _, _, _, _, s in sc if len(s)]
    assert len(np.intersect1d(scores[0], scores[1])) > 0  # confidences tied across scenes
    sizes = np.concatenate([m.sum(1) for _, _, m, _, _ in sc])
    assert (sizes < 100).any()


def test_benchmark_label_ids():
    # test.py:65-68: FOLD[cvfold][cls - 4] -> BENCHMARK_SEMANTIC_LABELS
    assert E.benchmark_label_ids(np.array([4, 5, 12]), 0).tolist() == [3, 4, 36]
    assert E.benchmark_label_ids(np.array([4, 8, 12]), 1).tolist() == [6, 24, 39]
    assert E.FOLD_CLASS_IDS[0] == (3, 4, 5, 8, 10, 12, 14, 16, 36)
    assert E.FOLD_CLASS_IDS[1] == (6, 7, 9, 11, 24, 28, 33, 34, 39)
    assert sorted(E.FOLD_CLASS_IDS[0] + E.FOLD_CLASS_IDS[1]) == list(E.VALID_CLASS_IDS)
    torch = pytest.importorskip("torch")
    t = E.benchmark_label_ids(torch.tensor([12, 4, 6]), 0)
    assert torch.is_tensor(t) and t.tolist() == [36, 3, 5]


def test_gt_ids_from_labels():
    sem = np.array([0, 1, 5, 5, -100, 19, 19, 3, 7, 2])
    inst = np.array([-100, -100, 0, 0, -100, 2, 2, 0, 3, -100])
    # instance 0: first point has label 5 -> nyu 6; instance 2: label 19 -> 39; instance 3: label 7 -> 8; no instance 1
    want = [0, 0, 6001, 6001, 0, 39003, 39003, 6001, 8004, 0]
    assert E.gt_ids_from_labels(sem, inst).tolist() == want
    # an instance whose first point is unlabelled takes label 0 (nyu 1, wall)
    assert E.gt_ids_from_labels(np.array([-100, 4]), np.array([0, 0])).tolist() == [1001, 1001]
    assert E.gt_ids_from_labels(np.array([1, 2]), np.array([-100, -100])).tolist() == [0, 0]
    torch = pytest.importorskip("torch")
    t = E.gt_ids_from_labels(torch.from_numpy(sem), torch.from_numpy(inst))
    assert t.tolist() == want


def test_class_sets():
    ids, names = E.class_set("all")
    assert len(ids) == 18 and names[12] == "refrigerator"
    assert E.class_set(1)[1][:2] == ["sofa", "table"]
    with pytest.raises(ValueError):
        E.class_set(2)
    with pytest.raises(ValueError):
        E.class_set([3, 3])
