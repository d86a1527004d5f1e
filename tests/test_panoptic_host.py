"""Panoptic labels and panoptic quality on the host: the numpy statement of gf_panoptic_overlaps (the GPU tests'
yardstick) against a brute-force count, the worked example of DESIGN.md section 14, the matching rules.  No GPU."""
import math

import numpy as np
import pytest

CLASSES = np.array([1, 3], np.int64)  # the worked example: stuff = {1}, things = {3}
IS_STUFF = np.array([True, False])


def worked_example():
    gt = np.array([3001] * 8 + [3002] * 4 + [1001] * 3 + [1002] * 3 + [0] * 2, np.int64)
    owner = np.full(20, -1, np.int64)
    owner[[0, 1, 2, 3, 4, 5, 18]] = 0
    owner[[8, 9]] = 1
    sem = np.full(20, 2, np.int64)  # class 2: nothing
    sem[[12, 13, 14, 15, 16, 19]] = 0  # wall
    ids = np.where(owner >= 0, 3000 + owner + 1, 0)
    return owner, ids, sem, gt


def brute_force(owner, sem, gt, offsets, class_ids, is_stuff, stuff_of_sem, P, ids=None):
    """The tables by their definition: one np.count_nonzero per (row, column) pair.  Returns per scene (gt_id, inter
    [R, G + 1] with void last) and pan."""
    cls = [int(c) for c in class_ids]
    stuff_cls = [c for c, s in zip(cls, is_stuff) if s]
    R = P + len(stuff_cls) + 1
    N = len(owner)
    row = np.empty(N, np.int64)
    pan = np.zeros(N, np.int64)
    for i in range(N):
        c = -1
        if 0 <= sem[i] < len(stuff_of_sem) and 0 <= stuff_of_sem[sem[i]] < len(cls):
            c = int(stuff_of_sem[sem[i]])
        if 0 <= owner[i] < P:
            row[i] = owner[i]
            pan[i] = 0 if ids is None else ids[i]
        elif c >= 0 and is_stuff[c]:
            row[i] = P + stuff_cls.index(cls[c])
            pan[i] = cls[c] * 1000
        else:
            row[i] = R - 1
    seg = np.empty(N, np.int64)  # the segment id of a point, -1 = void
    for i in range(N):
        q = int(gt[i]) // 1000  # (Python floors)
        if q not in cls:
            seg[i] = -1
        else:
            seg[i] = q * 1000 if is_stuff[cls.index(q)] else gt[i]
    out = []
    for s in range(len(offsets) - 1):
        lo, hi = int(offsets[s]), int(offsets[s + 1])
        r, g = row[lo:hi], seg[lo:hi]
        gt_id = sorted(set(g[g >= 0].tolist()))
        inter = np.zeros((R, len(gt_id) + 1), np.int64)
        for a in range(R):
            for b, gid in enumerate(gt_id + [-1]):
                inter[a, b] = np.count_nonzero((r == a) & (g == gid))
        out.append((np.array(gt_id, np.int64), inter))
    return out, pan


def compact(Gs, gt_id, inter, s):
    G = int(Gs[s])
    return gt_id[s, :G], np.concatenate([inter[s][:, :G], inter[s][:, -1:]], 1)


def test_worked_example():
    from geoformer_amd import evaluation as E

    owner, ids, sem, gt = worked_example()
    pan, Gs, gt_id, inter = E.panoptic_overlaps_host(owner, sem, gt, class_ids=CLASSES, is_stuff=IS_STUFF,
                                                     stuff_of_sem=[0, -1], P=2, ids=ids)
    assert pan.dtype == np.int32
    want_pan = np.zeros(20, np.int64)
    want_pan[[0, 1, 2, 3, 4, 5, 18]] = 3001
    want_pan[[8, 9]] = 3002
    want_pan[[12, 13, 14, 15, 16, 19]] = 1000
    assert np.array_equal(pan, want_pan)
    assert Gs.tolist() == [3] and gt_id[0].tolist() == [1000, 3001, 3002]
    #            wall 3001 3002 void
    want = [[0, 6, 0, 1],   # rank 0
            [0, 0, 2, 0],   # rank 1
            [5, 0, 0, 1],   # wall
            [1, 2, 2, 0]]   # unlabelled
    assert inter[0].tolist() == want
    (table,) = E.panoptic_tables(Gs, gt_id, inter, [[3, 3]], CLASSES, IS_STUFF, 2)
    res = E.panoptic_quality([table])
    assert res["tp"].tolist() == [1, 1] and res["fp"].tolist() == [0, 1] and res["fn"].tolist() == [0, 1]
    wall, thing = res["classes"]["wall"], res["classes"]["cabinet"]
    assert (thing["pq"], thing["sq"], thing["rq"]) == (0.375, 0.75, 0.5)  # 6/8 exactly; 2/4 = 0.5 is no match
    assert wall["pq"] == wall["sq"] == 5 / 6 and wall["rq"] == 1.0
    assert res["pq"] == (0.375 + 5 / 6) / 2 and abs(res["pq"] - 0.6041666666666666) < 1e-15
    assert res["pq_th"] == 0.375 and res["pq_st"] == 5 / 6
    assert (res["sq_th"], res["rq_th"], res["sq_st"], res["rq_st"]) == (0.75, 0.5, 5 / 6, 1.0)
    # the evaluator on the same arrays
    ev = E.PanopticEvaluator(classes=[3], stuff=(1,))
    assert np.array_equal(ev.add_scene("s", owner, ids, sem, gt, [3, 3]), want_pan)
    got = ev.evaluate()
    assert got["pq"] == res["pq"] and got["pq_th"] == 0.375 and got["pq_st"] == 5 / 6
    text = ev.format_results(got)
    assert "wall" in text and "0.604" in text and "things" in text
    with pytest.raises(ValueError):
        ev.add_scene("s", owner, ids, sem, gt, [3, 3])  # twice


def random_batch(rng, Ns, P, class_ids, L, wild=True):
    N = int(sum(Ns))
    owner = rng.integers(-1, max(P, 1), N)
    sem = rng.integers(0, max(L, 1), N)
    cls_pool = list(class_ids) + [0, 40, 17]  # evaluated and unevaluated classes
    gt = np.array([rng.choice(cls_pool) * 1000 + rng.integers(0, 6) for _ in range(N)], np.int64)
    if wild and N:
        k = max(N // 8, 1)
        owner[rng.integers(0, N, k)] = rng.choice([-5, P, P + 3, 2 ** 31 - 1, -2 ** 31], k)  # outside [-1, P)
        sem[rng.integers(0, N, k)] = rng.choice([-1, L, L + 7, 2 ** 31 - 1, -2 ** 31], k)  # outside [0, L)
        gt[rng.integers(0, N, k)] = rng.choice([-1, -999, -1000, -1001, -3001, -2 ** 40, 0, 999, 2 ** 40 + 3], k)
    ids = np.where((owner >= 0) & (owner < P), 3000 + owner + 1, 0)
    return owner, ids, sem, gt, np.concatenate([[0], np.cumsum(Ns)]).astype(np.int32)


@pytest.mark.parametrize("Ns,P", [((40,), 3), ((17, 0, 33), 5), ((25,), 0), ((0,), 2), ((30, 30), 1)])
def test_host_statement_equals_brute_force(Ns, P):
    from geoformer_amd import evaluation as E

    rng = np.random.default_rng(sum(Ns) + P)
    class_ids = np.array([5, 1, 9, 2, 3], np.int64)  # not sorted: the columns follow the ids, the stuff rows this order
    is_stuff = np.array([0, 1, 0, 1, 0], bool)
    sos = np.array([3, 1, -1, 0, 7, -4], np.int32)  # floor, wall, nothing, a thing class (no stuff), out of range twice
    owner, ids, sem, gt, off = random_batch(rng, Ns, P, class_ids, len(sos))
    pan, Gs, gt_id, inter = E.panoptic_overlaps_host(owner, sem, gt, off, class_ids=class_ids, is_stuff=is_stuff,
                                                     stuff_of_sem=sos, P=P, ids=ids)
    want, want_pan = brute_force(owner, sem, gt, off, class_ids, is_stuff, sos, P, ids)
    assert np.array_equal(pan, want_pan)
    assert inter.shape == (len(Ns), P + 3, int(Gs.max()) + 1)
    for s, (wid, wint) in enumerate(want):
        gid, it = compact(Gs, gt_id, inter, s)
        assert np.array_equal(gid, wid), s
        assert np.array_equal(it, wint), s
        assert it.sum() == Ns[s]
        assert not inter[s][:, int(Gs[s]):-1].any()  # the columns between G_s and void stay zero


def test_no_segments_and_no_rows():
    """G = 0 (every point void) and P = 0 with no stuff prediction: one unlabelled row, one void column."""
    from geoformer_amd import evaluation as E

    gt = np.array([0, 40003, -7, 17001], np.int64)
    pan, Gs, gt_id, inter = E.panoptic_overlaps_host([-1, 0, 5, -1], [2, 2, 2, 2], gt, class_ids=CLASSES,
                                                     is_stuff=IS_STUFF, stuff_of_sem=[0], P=0, ids=np.zeros(4, np.int64))
    assert Gs.tolist() == [0] and gt_id.shape == (1, 0) and inter.tolist() == [[[0], [4]]] and not pan.any()
    (t,) = E.panoptic_tables(Gs, gt_id, inter, [[]], CLASSES, IS_STUFF, 0)
    res = E.panoptic_quality([t])
    assert math.isnan(res["pq"]) and math.isnan(res["pq_th"]) and math.isnan(res["pq_st"])


def test_overflow_reports_g_alone():
    from geoformer_amd import evaluation as E

    gt = np.array([3001, 3002, 3003, 3001, 3002], np.int64)
    off = np.array([0, 3, 5])
    _, Gs, gt_id, inter = E.panoptic_overlaps_host([0] * 5, [0] * 5, gt, off, class_ids=CLASSES, is_stuff=IS_STUFF,
                                                   stuff_of_sem=[0], P=1, max_gt=2)
    assert Gs.tolist() == [3, 2] and not inter[0].any() and inter[1, 0].tolist() == [1, 1, 0]
    assert gt_id[1].tolist() == [3001, 3002]


def table_of(inter, gt_id, label_id):
    from geoformer_amd import evaluation as E

    return E.PanopticTable(np.array(gt_id, np.int64), np.array(inter, np.int64), np.array(label_id, np.int64), CLASSES,
                           IS_STUFF)


def test_mostly_void_prediction_is_no_false_positive():
    from geoformer_amd import evaluation as E

    #                 3001 void
    res = E.panoptic_quality([table_of([[1, 3],    # 3 of 4 points void: ignored
                                        [1, 1],    # exactly half void: a false positive
                                        [0, 0],    # wall: empty, no segment
                                        [8, 0]], [3001], [3, 3])])
    assert res["fp"].tolist() == [0, 1] and res["fn"].tolist() == [0, 1] and res["tp"].tolist() == [0, 0]
    assert res["classes"]["cabinet"]["sq"] == 0.0 and res["pq_th"] == 0.0  # SQ is 0 without a match


def test_void_leaves_the_union_and_half_is_no_match():
    from geoformer_amd import evaluation as E

    # I = 3, prediction 3 + 2 void, segment 5: union 5 + 5 - 3 - 2 = 5, IoU 0.6; without the void rule 3/7: no match
    res = E.panoptic_quality([table_of([[3, 2], [0, 0], [2, 0]], [3001], [3])])
    assert res["tp"].tolist() == [0, 1] and res["iou_sum"][1] == 0.6
    # I = 2 of prediction 3 and segment 3: union 4, exactly one half
    res = E.panoptic_quality([table_of([[2, 1, 0], [0, 0, 0], [1, 0, 0]], [3001, 3002], [3])])
    assert res["tp"].tolist() == [0, 0] and res["fp"].tolist() == [0, 1] and res["fn"].tolist() == [0, 2]
    # a match needs the same class: the wall row on a thing segment is an FP and an FN
    res = E.panoptic_quality([table_of([[0, 0], [5, 0], [0, 0]], [3001], [3])])
    assert res["tp"].tolist() == [0, 0] and res["fp"].tolist() == [1, 0] and res["fn"].tolist() == [0, 1]


def test_absent_class_is_left_out_of_the_means():
    from geoformer_amd import evaluation as E

    cls, st = np.array([1, 2, 3, 4], np.int64), np.array([1, 1, 0, 0], bool)
    t = E.PanopticTable(np.array([1000, 3001]), np.array([[0, 4, 0], [4, 0, 0], [0, 0, 0], [0, 0, 1]]), np.array([3]),
                        cls, st)
    res = E.panoptic_quality([t])
    assert res["pq"] == 1.0 and res["pq_th"] == 1.0 and res["pq_st"] == 1.0  # floor and class 4 appear nowhere
    assert math.isnan(res["classes"]["floor"]["pq"]) and math.isnan(res["classes"]["bed"]["rq"])
    assert res["classes"]["wall"]["pq"] == 1.0


def test_thing_row_outside_the_class_set():
    from geoformer_amd import evaluation as E

    with pytest.raises(ValueError):
        E.panoptic_quality([table_of([[3, 0], [0, 0], [0, 0]], [3001], [7])])
    E.panoptic_quality([table_of([[0, 0], [0, 0], [3, 0]], [3001], [7])])  # an empty row's class does not matter


def test_evaluator_over_two_scenes_is_the_sum():
    from geoformer_amd import evaluation as E

    rng = np.random.default_rng(5)
    ev = E.PanopticEvaluator(classes=[3, 5], stuff=(1, 2))
    parts = []
    for name, N in (("a", 300), ("b", 200)):
        owner = np.repeat(rng.integers(-1, 4, N // 10), 10)
        sem = np.repeat(rng.integers(0, 4, N // 10), 10)
        gt = np.repeat(rng.choice([1001, 2001, 3001, 3002, 5001, 0], N // 10), 10)
        lab = np.array([3, 5, 3, 5])
        ids = np.where(owner >= 0, lab[np.maximum(owner, 0)] * 1000 + owner + 1, 0)
        one = E.PanopticEvaluator(classes=[3, 5], stuff=(1, 2))
        one.add_scene(name, owner, ids, sem, gt, lab)
        parts.append(one.evaluate())
        ev.add_scene(name, owner, ids, sem, gt, lab)
    res = ev.evaluate()
    assert sum(int(res[k].sum()) for k in ("tp", "fp", "fn")) > 0
    for k in ("tp", "fp", "fn"):
        assert np.array_equal(res[k], parts[0][k] + parts[1][k])
    assert np.array_equal(res["iou_sum"], parts[0]["iou_sum"] + parts[1]["iou_sum"])
    tp, fp, fn = (res[k].astype(float) for k in ("tp", "fp", "fn"))
    seen = (tp + fp + fn) > 0
    assert res["pq"] == float((res["iou_sum"][seen] / (tp + fp / 2 + fn / 2)[seen]).mean())
    assert list(ev.scene_tables()) == ["a", "b"]


def test_save_labels_writes_panoptic_only_when_given(tmp_path):
    from geoformer_amd import export, postprocess

    lab = postprocess.label_points(np.ones((1, 4), np.int32), np.ones(1, np.float32), np.array([3]), np.array([0]),
                                   np.zeros((4, 3), np.float32))
    export.save_labels(tmp_path / "a.npz", lab)
    export.save_labels(tmp_path / "b.npz", lab, panoptic=np.array([3001, 3001, 1000, 0], np.int32))
    with np.load(tmp_path / "a.npz") as a, np.load(tmp_path / "b.npz") as b:
        assert "panoptic" not in a.files and b["panoptic"].tolist() == [3001, 3001, 1000, 0]
        assert sorted(set(b.files) - {"panoptic"}) == sorted(a.files)
    assert np.array_equal(export.load_labels(tmp_path / "b.npz").ids, lab.ids)
