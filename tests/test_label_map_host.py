"""Scene labelling on the host: postprocess.label_points (numpy path) against a literal restatement of the reference's
painting loop (util/visualize.py:219-227), the val_gt encoding of the ids, and the files of geoformer_amd.export."""
import os

import numpy as np
import pytest

SIZES = [(0, 1000), (1, 5000), (37, 20000), (128, 150000), (256, 60000), (5, 70)]
SEED = 11


def _nms_case(rng, n, N, n_cls=3):
    """n overlapping proposals over N points: random runs of the points with holes, distinct scores, a few categories
    (the construction of tests/test_gpu_batched_eval.py::_nms_case)."""
    masks = np.zeros((n, N), np.int32)
    for i in range(n):
        ln = int(rng.integers(N // 50 + 1, N // 4 + 2))
        s = int(rng.integers(0, N - ln + 1))
        masks[i, s:s + ln] = 1
        if i % 3 == 0 and n > 0:  # holes
            masks[i, s + ln // 3:s + ln // 3 + ln // 10] = 0
    scores = ((rng.permutation(n) + 1) / (n + 1)).astype(np.float32)
    cats = rng.integers(0, n_cls, n).astype(np.int64)
    return masks, scores, cats


def label_case(rng, n, N):
    """(masks, scores, label_ids, pick, xyz): pick = the best three quarters by score, descending; label ids from the
    benchmark's; xyz in [-8, 8] m."""
    from geoformer_amd import evaluation

    masks, scores, cats = _nms_case(rng, n, N)
    label_ids = np.asarray(evaluation.BENCHMARK_SEMANTIC_LABELS, np.int64)[cats + 2]
    pick = np.argsort(-scores, kind="stable")[:(3 * n + 3) // 4].astype(np.int64)
    xyz = rng.uniform(-8.0, 8.0, (N, 3)).astype(np.float32)
    return masks, scores, label_ids, pick, xyz


def all_cases():
    rng = np.random.default_rng(SEED)
    return [label_case(rng, n, N) for n, N in SIZES]


def restated(masks, scores, label_ids, pick, xyz, min_score):
    """The reference's loop, literally, and the table by definition (float64 centroid)."""
    N, p = xyz.shape[0], len(pick)
    owner = np.full(N, -1, np.int64)
    for r in range(p - 1, -1, -1):
        if scores[pick[r]] < min_score:
            continue
        mask = masks[pick[r]]
        owner[mask == 1] = r
    ids = np.zeros(N, np.int64)
    for i in range(N):
        if owner[i] >= 0:
            ids[i] = label_ids[pick[owner[i]]] * 1000 + owner[i] + 1
    m = masks[pick].astype(np.float64).reshape(p, N)
    count = m.sum(1).astype(np.int64)
    cen = np.zeros((p, 3))
    lo = np.zeros((p, 3), np.float32)
    hi = np.zeros((p, 3), np.float32)
    for r in range(p):
        if count[r]:
            cen[r] = m[r] @ xyz.astype(np.float64) / count[r]
            lo[r], hi[r] = xyz[m[r] == 1].min(0), xyz[m[r] == 1].max(0)
    return {"owner": owner, "ids": ids, "count": count, "owned": np.array([(owner == r).sum() for r in range(p)], np.int64),
            "kept": np.array([scores[pick[r]] >= min_score for r in range(p)], bool), "centroid": cen, "box_min": lo,
            "box_max": hi, "index": pick, "label_id": label_ids[pick], "score": scores[pick]}


def check_against(lab, want, xyz, centroid_eps=32):
    """lab (host SceneLabels) against restated(): integers and boxes equal, centroid within centroid_eps fp32 eps of
    max|xyz| of the float64 value."""
    t = lab.table
    assert lab.owner.dtype == np.int32 and lab.ids.dtype == np.int32
    assert np.array_equal(lab.owner, want["owner"]) and np.array_equal(lab.ids, want["ids"])
    for k in ("count", "owned", "kept", "index", "label_id"):
        assert np.array_equal(np.asarray(getattr(t, k)), want[k]), k
    assert np.array_equal(t.score, want["score"])
    assert np.array_equal(t.box_min, want["box_min"]) and np.array_equal(t.box_max, want["box_max"])
    assert t.centroid.shape == want["centroid"].shape
    if t.centroid.size:
        bound = centroid_eps * np.finfo(np.float32).eps * float(np.abs(xyz).max())
        err = float(np.abs(t.centroid.astype(np.float64) - want["centroid"]).max())
        assert err <= bound, (err, bound)
        return err / (np.finfo(np.float32).eps * float(np.abs(xyz).max()))
    return 0.0


@pytest.mark.parametrize("min_score", [0.0, 0.09, 0.5])
def test_numpy_path_equals_reference_loop(min_score):
    from geoformer_amd import postprocess

    for (n, N), case in zip(SIZES, all_cases()):
        masks, scores, label_ids, pick, xyz = case
        want = restated(*case, min_score)
        if n >= 37:  # the inputs exercise the rule (asserted on the restatement alone)
            kept = want["kept"]
            cover = masks[pick[kept]].sum(0)
            assert (cover >= 2).mean() >= 0.10 and (cover == 0).mean() >= 0.01, (n, N)
            assert ((want["owned"] == 0) & kept).any()
            if min_score == 0.5:
                assert (~kept).any()
        lab = postprocess.label_points(masks, scores, label_ids, pick, xyz, min_score)
        check_against(lab, want, xyz)
        assert int((lab.table.owned).sum()) == int((lab.owner >= 0).sum())


def test_default_min_score_and_empty_scene():
    from geoformer_amd import postprocess

    assert postprocess.MIN_SCORE == 0.09
    xyz = np.zeros((50, 3), np.float32)
    lab = postprocess.label_points([], [], [], np.zeros(0, np.int64), xyz)  # as predict_batches yields it
    assert (lab.owner == -1).all() and (lab.ids == 0).all() and lab.owner.shape == (50,)
    assert all(len(c) == 0 for c in lab.table) and lab.table.centroid.shape == (0, 3)
    # the default threshold is the reference's 0.09
    m = np.ones((2, 50), np.int32)
    lab = postprocess.label_points(m, np.array([0.08, 0.091], np.float32), np.array([3, 4]), np.array([1, 0]), xyz)
    assert lab.table.kept.tolist() == [True, False] and (lab.ids == 4001).all()


def test_torch_cpu_inputs_take_the_numpy_path():
    import torch

    from geoformer_amd import postprocess

    case = all_cases()[2]
    a = postprocess.label_points(*case)
    b = postprocess.label_points(*[torch.from_numpy(x) for x in case])
    assert np.array_equal(a.owner, b.owner) and np.array_equal(a.ids, b.ids)
    assert all(np.array_equal(x, y) for x, y in zip(a.table, b.table))


def gt_case(n_points=20000, seed=3):
    """Ground truth of a labelled synthetic scene as predictions: one mask per instance id (ids the scene does not use
    give empty masks), score 1, pick = instance order."""
    from geoformer_amd import evaluation, scene

    raw = scene.make_raw_scene(n_points, seed)
    sem, inst = raw[:, 6].astype(np.int64), raw[:, 7].astype(np.int64)
    n = int(inst.max()) + 1
    masks = (inst[None, :] == np.arange(n)[:, None]).astype(np.int32)
    label_ids = np.zeros(n, np.int64)
    for i in range(n):
        pts = np.nonzero(masks[i])[0]
        if pts.size:
            s = sem[pts[0]]
            label_ids[i] = evaluation.BENCHMARK_SEMANTIC_LABELS[0 if s == -100 else s]
    return raw, masks, np.ones(n, np.float32), label_ids, np.arange(n, dtype=np.int64)


def test_ids_of_ground_truth_masks_equal_val_gt():
    from geoformer_amd import evaluation, postprocess

    raw, masks, scores, label_ids, pick = gt_case()
    lab = postprocess.label_points(masks, scores, label_ids, pick, raw[:, :3].astype(np.float32))
    gt = evaluation.gt_ids_from_labels(raw[:, 6], raw[:, 7])
    has = raw[:, 7] >= 0
    assert has.sum() > 1000 and (~has).sum() > 100
    assert np.array_equal(lab.ids[has], gt[has]) and (lab.ids[~has] == 0).all() and (gt[~has] == 0).all()


@pytest.mark.parametrize("full", [False, True])
def test_scannet_files_round_trip(tmp_path, full):
    from geoformer_amd import export, postprocess

    masks, scores, label_ids, pick, xyz = all_cases()[2]
    lab = postprocess.label_points(masks, scores, label_ids, pick, xyz, 0.5)
    kept = np.nonzero(lab.table.kept)[0]
    assert 0 < len(kept) < len(pick)
    path = export.write_scannet_predictions(str(tmp_path), "scene0000_00", lab, masks[pick] if full else None)
    assert path == os.path.join(str(tmp_path), "scene0000_00.txt")
    got_ids, got_scores, got_masks = export.read_scannet_predictions(str(tmp_path), "scene0000_00")
    assert np.array_equal(got_ids, label_ids[pick][kept])
    assert export.SCORE_FORMAT == "%.6f" and np.abs(got_scores - scores[pick][kept]).max() <= 1e-6
    want = masks[pick][kept] if full else np.stack([lab.owner == r for r in kept])
    assert got_masks.dtype == np.uint8 and np.array_equal(got_masks, want)
    if not full:
        assert got_masks.sum(0).max() == 1
    # the reference's reader (util/visualize.py:212-227)
    with open(path) as f:
        lines = [line.rstrip().split() for line in f.readlines()]
    assert len(lines) == len(kept)
    for r, line in zip(kept, lines):
        mask_path = os.path.join(os.path.dirname(path), line[0])
        assert line[0] == f"predicted_masks/scene0000_00_{r:03d}.txt" and os.path.isfile(mask_path)
        assert int(line[1]) == label_ids[pick[r]] and abs(float(line[2]) - scores[pick[r]]) <= 1e-6
    m0 = np.loadtxt(os.path.join(os.path.dirname(path), lines[0][0]))
    assert m0.shape == (xyz.shape[0],) and np.array_equal(m0.astype(np.uint8), want[0])


def test_npz_round_trip(tmp_path):
    from geoformer_amd import export, postprocess

    lab = postprocess.label_points(*all_cases()[2])
    p = str(tmp_path / "scene.npz")
    export.save_labels(p, lab)
    back = export.load_labels(p)
    assert np.array_equal(back.owner, lab.owner) and np.array_equal(back.ids, lab.ids) and back.masks is None
    for k, a, b in zip(lab.table._fields, lab.table, back.table):
        assert a.dtype == b.dtype and np.array_equal(a, b), k


def test_ap_from_read_back_masks_equals_ap_from_memory(tmp_path):
    from geoformer_amd import evaluation, export, postprocess

    raw, masks, scores, label_ids, pick = gt_case(30000, 5)
    rng = np.random.default_rng(2)
    masks = masks * (rng.random(masks.shape) < 0.9)  # imperfect predictions with distinct scores
    scores = ((rng.permutation(len(scores)) + 1) / (len(scores) + 1)).astype(np.float32)
    pick = np.argsort(-scores, kind="stable").astype(np.int64)
    lab = postprocess.label_points(masks, scores, label_ids, pick, raw[:, :3].astype(np.float32), 0.0)
    assert lab.table.kept.all()
    export.write_scannet_predictions(str(tmp_path), "s", lab, masks[pick])
    got_ids, got_scores, got_masks = export.read_scannet_predictions(str(tmp_path), "s")
    gt = evaluation.gt_ids_from_labels(raw[:, 6], raw[:, 7])
    res = []
    for l, s, m in ((label_ids[pick], scores[pick], masks[pick]),
                    (got_ids, got_scores, got_masks)):
        ev = evaluation.InstanceEvaluator(classes="all")
        ev.add_scene("s", gt, l, s, m)
        res.append(ev.evaluate())
    assert np.array_equal(res[0][0], res[1][0], equal_nan=True)
    assert np.isfinite(res[0][1]["all_ap"]) and res[0][1]["all_ap"] > 0
    assert res[0][1]["all_ap"] == res[1][1]["all_ap"]
