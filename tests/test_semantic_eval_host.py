"""Semantic-segmentation evaluation on the host: the numpy statements of gf_semantic_confusion (the GPU tests' yardstick),
the label table, the metrics, the benchmark file.  No GPU."""
import inspect
import math
from fractions import Fraction as Fr

import numpy as np
import pytest
import torch

NAN, INF = float("nan"), float("inf")
# rows whose arg-max needs the rule spelled out: (row, first maximal class with '>' from class 0 upwards)
EDGE_ROWS = [
    ([1.0, 3.0, 3.0, 2.0], 1),       # a tie: the lowest class wins
    ([2.0, 2.0, 2.0, 2.0], 0),
    ([NAN, 5.0, 1.0, 0.0], 0),       # NaN in column 0 wins: nothing is > NaN
    ([1.0, NAN, 0.5, 0.0], 0),       # NaN in column k > 0 never wins
    ([0.0, NAN, 2.0, 1.0], 2),
    ([0.0, 1.0, NAN, NAN], 1),
    ([0.0, INF, 3.0, INF], 1),       # +inf twice
    ([-INF, -INF, -INF, -INF], 0),   # all -inf
    ([-INF, -INF, -1e30, -INF], 2),
    ([NAN, NAN, NAN, NAN], 0),
]


def one_hot(preds, C):
    s = np.zeros((len(preds), C), np.float32)
    s[np.arange(len(preds)), preds] = 1.0
    return s


def test_hand_written_case():
    """3 classes, 2 scenes of 6 + 4 points, one ignored label, class 2 in neither prediction nor ground truth."""
    from geoformer_amd import evaluation as E

    gt = np.array([0, 0, 1, 1, -100, 0, 1, 0, 1, 1])
    pred = np.array([0, 1, 1, 1, 0, 0, 0, 0, 1, 1])
    offsets = np.array([0, 6, 10], np.int32)
    want = np.array([[[2, 1, 0], [0, 2, 0], [0, 0, 0], [1, 0, 0]],
                     [[1, 0, 0], [1, 2, 0], [0, 0, 0], [0, 0, 0]]], np.int64)
    p, conf = E.semantic_confusion_host(one_hot(pred, 3), gt, offsets)
    assert p.dtype == np.int32 and (p == pred).all()
    assert conf.dtype == np.int64 and conf.shape == (2, 4, 3) and (conf == want).all()

    ev = E.SemanticEvaluator(n_classes=3, raw_labels=False, fg_class=1, candidate_class=0)
    got = ev.add_batch(one_hot(pred, 3), gt, offsets, ["a", "b"])
    assert (got == pred).all()
    assert (ev.confusion() == want.sum(0)).all()
    per = ev.scene_confusions()
    assert list(per) == ["a", "b"] and (per["a"] == want[0]).all() and (per["b"] == want[1]).all()
    res = ev.evaluate()
    # total: [[3, 1, 0], [1, 4, 0], [0, 0, 0]] + one ignored point predicted as class 0 (in no fp)
    assert res["iou"][0] == float(Fr(3, 5)) and res["iou"][1] == float(Fr(4, 6)) and math.isnan(res["iou"][2])
    assert res["miou"] == pytest.approx(float((Fr(3, 5) + Fr(2, 3)) / 2), rel=1e-15)
    assert res["miou_fold"] == pytest.approx(float(Fr(2, 3)), rel=1e-15)  # classes 1..2, class 2 is nan
    assert res["acc"] == float(Fr(7, 9))
    assert res["macc"] == pytest.approx(float((Fr(3, 4) + Fr(4, 5)) / 2), rel=1e-15)
    assert res["points"] == 9 and res["ignored"] == 1
    assert res["foreground"] == {"precision": float(Fr(4, 5)), "recall": float(Fr(4, 5)), "iou": float(Fr(4, 6))}
    assert res["candidate"] == {"precision": float(Fr(3, 4)), "recall": float(Fr(3, 4)), "iou": float(Fr(3, 5))}
    text = ev.format_results(res)
    assert "mIoU" in text and "foreground" in text and "nan" in text
    # the dataset total alone, two calls: the same numbers
    ev2 = E.SemanticEvaluator(n_classes=3, raw_labels=False, keep_scenes=False, fg_class=1, candidate_class=0)
    ev2.add_batch(one_hot(pred[:6], 3), gt[:6])
    ev2.add_batch(one_hot(pred[6:], 3), gt[6:])
    assert (ev2.confusion() == want.sum(0)).all() and ev2.evaluate()["miou"] == res["miou"]
    with pytest.raises(ValueError):
        ev2.scene_confusions()


def test_argmax_equals_torch_without_ties():
    from geoformer_amd import evaluation as E

    rng = np.random.default_rng(5)
    for C in (1, 2, 13, 20, 64):
        s = rng.permuted(np.tile(np.arange(C, dtype=np.float32), (777, 1)), axis=1) * 0.37 - 3.0  # no ties in a row
        assert (E.semantic_preds_host(s) == torch.from_numpy(s).max(1)[1].numpy()).all()
    s = rng.standard_normal((5000, 13)).astype(np.float32)
    assert (np.sort(s, 1)[:, -1] > np.sort(s, 1)[:, -2]).all()
    assert (E.semantic_preds_host(s) == torch.from_numpy(s).max(1)[1].numpy()).all()


def test_argmax_edge_rows():
    from geoformer_amd import evaluation as E

    s = np.array([r for r, _ in EDGE_ROWS], np.float32)
    assert E.semantic_preds_host(s).tolist() == [w for _, w in EDGE_ROWS]


@pytest.mark.parametrize("fold", [0, 1])
def test_label_table_equals_the_augmentation(fold):
    """semantic_label_lut against the relabelling train_merge_numpy does to a scene that holds every label."""
    from geoformer_amd import evaluation as E
    from tests.augment_numpy import train_merge_numpy

    raw = np.array([-100, -1] + list(range(20)) + [25], np.int64)
    rng = np.random.default_rng(fold)
    data = np.zeros((len(raw), 8))
    data[:, :3] = rng.uniform(0.0, 1.0, (len(raw), 3))
    data[:, 3:6] = rng.uniform(-1.0, 1.0, (len(raw), 3))
    data[:, 6] = raw
    data[:, 7] = -100
    np.random.seed(3)
    torch.manual_seed(3)
    batch, _, _ = train_merge_numpy([data], cvfold=fold, voxelise=False)
    want = batch["labels"]
    assert want.shape == raw.shape  # (nothing was cropped: the order is the scene's)
    lut, map_ignore, map_other = E.semantic_label_lut(fold)
    assert lut.dtype == np.int32 and lut.shape == (20,)
    got = E.map_semantic_labels(raw, 13, lut, -100, map_ignore, map_other)
    assert (got == want).all()
    assert got[0] == 2 and got[1] == 3 and got[-1] == 3  # -100 is trained as a class, not ignored
    names = E.SEMANTIC_CLASS_NAMES(fold)
    assert len(names) == 13 and names[:4] == ("wall", "floor", "unannotated", "candidate")
    assert names[4:] == tuple(E.class_set(fold)[1])
    # identity mode: 0..C-1 stay, everything else is ignored (row C)
    assert E.map_semantic_labels(raw, 13).tolist() == [13, 13] + list(range(13)) + [13] * 8


@pytest.mark.parametrize("fold", [0, 1])
def test_semantic_file_round_trip(tmp_path, fold):
    from geoformer_amd import evaluation as E
    from geoformer_amd import export

    preds = np.array(list(range(13)) * 3 + [2, 3, 3, 2], np.int32)
    path = export.write_scannet_semantic(str(tmp_path / "semantic"), "scene0000_00", preds, fold)
    assert path.endswith("scene0000_00.txt")
    got = export.read_scannet_semantic(str(tmp_path / "semantic"), "scene0000_00")
    want = np.array([1, 2, 0, 0] + list(E.FOLD_CLASS_IDS[fold]), np.int64)[preds]
    assert got.dtype == np.int64 and (got == want).all()
    assert (got[(preds == 2) | (preds == 3)] == 0).all() and (got[preds >= 4] > 2).all()
    with open(path) as f:
        assert f.read() == "".join(f"{v}\n" for v in want)
    assert (export.read_scannet_semantic(str(tmp_path / "semantic"), "scene0000_00") ==
            export.semantic_benchmark_ids(fold)[preds]).all()
    with pytest.raises(ValueError):
        export.write_scannet_semantic(str(tmp_path), "bad", np.array([13]), fold)


def test_new_keywords_default_to_the_old_behaviour():
    from geoformer_amd import batch_eval

    assert inspect.signature(batch_eval.predict_batches).parameters["semantic"].default is None
    p = inspect.signature(batch_eval.semantic_batches).parameters
    assert p["evaluator"].default is None and p["evaluator"].kind is inspect.Parameter.KEYWORD_ONLY


def test_host_confusion_refuses_bad_offsets():
    from geoformer_amd import evaluation as E

    s = np.zeros((4, 3), np.float32)
    for off in ([0, 3], [1, 4], [0, 3, 2, 4]):
        with pytest.raises(ValueError):
            E.semantic_confusion_host(s, np.zeros(4, np.int64), np.array(off))
    _, conf = E.semantic_confusion_host(s, np.zeros(4, np.int64), np.array([0, 0, 4, 4]))
    assert conf.sum((1, 2)).tolist() == [0, 4, 0]
