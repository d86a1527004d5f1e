"""CPU: the numpy statements of csrc/boxes.hip (postprocess.instance_boxes_host / id_boxes_host / box_iou_host) against
hand-derived values, the box AP protocol of evaluation.BoxEvaluator on hand-made scenes, the table builders, the text
file of export.write_boxes and the edge points of render.box_points."""
import numpy as np
import pytest

from tests.box_cases import (UNIT, box_rows, host_rows, iou_pairs, lattice, member_count_ids_case,
                             member_count_rows_case, mixed_iou_case, table_entry)

EPS32 = 2.0 ** -23


# ---- boxes ----------------------------------------------------------------------------------------------------------------
def test_lattice_turned_by_table_entry_30():
    from geoformer_amd import postprocess

    xyz = lattice(30)
    b = postprocess.id_boxes(np.zeros(15, np.int32), 1, xyz, oriented=True)
    assert b.angle_index.tolist() == [30] and b.count.tolist() == [15] and b.angle_index.dtype == np.int32
    # the coordinates are fp32 roundings of values below 8: half an ulp of 8 each, a few of them per extent
    tol = 8 * 4 * EPS32
    assert np.abs(b.size[0] - [2.0, 0.5, 1.0]).max() < tol
    c, s = table_entry(30)
    centre = np.array([1.0 * c - 0.25 * s + 3.0, 1.0 * s + 0.25 * c - 1.0, 0.75])
    assert np.abs(b.center[0] - centre).max() < tol
    assert (b.cos[0], b.sin[0]) == (c, s) and b.yaw[0] == 30 * (np.pi / 2 / 90)
    assert b.rows.shape == (1, 10) and b.rows.dtype == np.float64


def test_one_angle_is_the_aligned_box_exactly():
    from geoformer_amd import postprocess

    rng = np.random.default_rng(3)
    case = member_count_ids_case(rng, 64, (0, 1, 7, 130))
    count, aligned, oriented = host_rows(case, 1)
    assert np.array_equal(aligned, oriented)
    xyz, g = case["xyz"], case["group"]
    for r in (1, 2, 3):
        q = xyz[g == r].astype(np.float64)
        assert np.array_equal(aligned[r, 3:6], q.max(0) - q.min(0))
        assert np.array_equal(aligned[r, 0:3], (q.max(0) + q.min(0)) / 2)
        assert aligned[r, 6:].tolist() == [1.0, 0.0, 0.0, float((g == r).sum())]
    b = postprocess.id_boxes(g, 4, xyz)  # oriented=False
    assert np.array_equal(b.rows, aligned) and np.array_equal(b.count, count) and (b.yaw == 0).all()


def test_single_point_and_empty_group():
    from geoformer_amd import postprocess

    xyz = np.array([[1.5, -2.25, 0.125], [9.0, 9.0, 9.0]], np.float32)
    for oriented in (False, True):
        b = postprocess.id_boxes(np.array([1, -1]), 2, xyz, oriented=oriented)
        assert b.count.tolist() == [0, 1]
        assert not b.rows[0].any()  # an empty group: a row of zeros
        assert np.array_equal(b.size[1], [0.0, 0.0, 0.0]) and b.angle_index[1] == 0
        assert np.allclose(b.center[1], xyz[0], rtol=0, atol=4 * EPS32) and b.center[1, 2] == 0.125
    # rows form: a pick outside the masks is an empty group; no masks at all: every pick is
    masks = np.array([[3, 0], [0, 0]], np.int32)
    b = postprocess.instance_boxes(masks, [0, 5, -1, 1], xyz)
    assert b.count.tolist() == [1, 0, 0, 0] and np.array_equal(b.center[0], xyz[0].astype(np.float64))
    assert postprocess.instance_boxes([], [0, 1], xyz).count.tolist() == [0, 0]
    assert postprocess.instance_boxes(masks, [], xyz).rows.shape == (0, 10)


def test_diamond_takes_entry_45_and_ties_take_the_lowest_index():
    from geoformer_amd import postprocess

    d = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0]], np.float32)
    assert postprocess.id_boxes(np.zeros(4, np.int32), 1, d, oriented=True).angle_index.tolist() == [45]
    # two points above each other: the footprint is 0 at every heading
    pair = np.array([[0.3, -0.7, 0.0], [0.3, -0.7, 2.0]], np.float32)
    b = postprocess.id_boxes(np.zeros(2, np.int32), 1, pair, oriented=True)
    assert b.angle_index.tolist() == [0] and np.array_equal(b.size[0], [0.0, 0.0, 2.0])


def test_overlapping_masks_and_other_mask_values():
    from geoformer_amd import postprocess

    rng = np.random.default_rng(5)
    case = member_count_rows_case(rng, 64)
    count, aligned, oriented = host_rows(case, 90)
    n = case["masks"].shape[0]
    want = [(case["masks"][r] != 0).sum() if 0 <= r < n else 0 for r in case["pick"]]
    assert count.tolist() == want and count.dtype == np.int32
    # the same groups through 0 / 1 masks and through the public call
    b = postprocess.instance_boxes((case["masks"] != 0).astype(np.uint8), case["pick"], case["xyz"], oriented=True)
    assert np.array_equal(b.rows, oriented) and np.array_equal(b.count, count)
    # no other heading of the table has a smaller footprint
    t = postprocess.box_angle_table(90)
    r = int(np.argmax(count))
    q = case["xyz"][case["masks"][case["pick"][r]] != 0]
    u = q[:, 0:1] * t[None, :, 0] + q[:, 1:2] * t[None, :, 1]
    v = q[:, 1:2] * t[None, :, 0] - q[:, 0:1] * t[None, :, 1]
    area = (u.max(0) - u.min(0)) * (v.max(0) - v.min(0))
    assert int(oriented[r, 8]) == int(np.argmin(area)) and oriented[r, 3] * oriented[r, 4] == pytest.approx(area.min(), rel=1e-6)


def test_angles_outside_the_range_raise():
    from geoformer_amd import evaluation, postprocess

    xyz = np.zeros((3, 3), np.float32)
    for bad in (0, -1, postprocess.BOX_MAX_ANGLES + 1, 2.5):
        with pytest.raises(ValueError):
            postprocess.box_angle_table(bad)
        with pytest.raises(ValueError):
            postprocess.id_boxes(np.zeros(3, np.int32), 1, xyz, oriented=True, angles=bad)
        with pytest.raises(ValueError):
            postprocess.instance_boxes(np.ones((1, 3), np.int32), [0], xyz, angles=bad)
        with pytest.raises(ValueError):
            evaluation.BoxEvaluator(kind="oriented", angles=bad)
    t = postprocess.box_angle_table(postprocess.BOX_MAX_ANGLES)
    assert t.shape == (postprocess.BOX_MAX_ANGLES, 2) and t.dtype == np.float32 and t[0].tolist() == [1.0, 0.0]
    assert postprocess.box_angle_table(1).tolist() == [[1.0, 0.0]]
    with pytest.raises(ValueError):
        evaluation.BoxEvaluator(kind="tilted")


# ---- IoU ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(iou_pairs())))
def test_iou_of_hand_derived_pairs(i):
    from geoformer_amd import postprocess

    a, b, want, tol = iou_pairs()[i]
    got = postprocess.box_iou(a, b)
    assert got.shape == (1, 1) and got.dtype == np.float64
    if tol == 0.0:
        assert got[0, 0] == want
    else:
        assert abs(got[0, 0] - want) < tol


def test_iou_of_random_oriented_boxes_against_sampling():
    """The clipped area against a count of grid samples inside both rectangles (a check of the geometry, to the grid's
    resolution), symmetry, and the Boxes / rows forms of the call."""
    from geoformer_amd import postprocess

    a, b = mixed_iou_case(np.random.default_rng(8))
    iou = postprocess.box_iou_host(a, b)
    assert iou.shape == (7, 5) and (iou >= 0).all() and (iou <= 1).all() and (iou > 0.01).sum() >= 5
    assert np.abs(iou - postprocess.box_iou_host(b, a).T).max() < 1e-6

    def inside(r, x, y):
        dx, dy = x - r[0], y - r[1]
        return (np.abs(dx * r[6] + dy * r[7]) <= r[3] / 2) & (np.abs(dy * r[6] - dx * r[7]) <= r[4] / 2)

    g = np.linspace(-4.0, 5.0, 1801)
    x, y = np.meshgrid(g, g, indexing="ij")
    cell = (g[1] - g[0]) ** 2
    for i, j in [(0, 0), (3, 4), (6, 4), (2, 1)]:
        ra, rb = a[i], b[j]
        area = (inside(ra, x, y) & inside(rb, x, y)).sum() * cell
        oz = max(0.0, min(ra[2] + ra[5] / 2, rb[2] + rb[5] / 2) - max(ra[2] - ra[5] / 2, rb[2] - rb[5] / 2))
        inter = area * oz
        want = inter / (ra[3] * ra[4] * ra[5] + rb[3] * rb[4] * rb[5] - inter)
        assert abs(iou[i, j] - want) < 0.01, (i, j, iou[i, j], want)
    boxes = postprocess._boxes_from_rows(a, a[:, 9].astype(np.int32), 90)
    assert np.array_equal(postprocess.box_iou(boxes, b), iou)
    assert np.array_equal(postprocess.box_iou(boxes._replace(rows=None), b), iou)
    assert postprocess.box_iou(a[:0], b).shape == (0, 5) and postprocess.box_iou(a, b[:0]).shape == (7, 0)


# ---- AP -------------------------------------------------------------------------------------------------------------------
def _corners(lo, size):
    lo, size = np.asarray(lo, np.float64), np.asarray(size, np.float64)
    return np.array([[lo[0] + i * size[0], lo[1] + j * size[1], lo[2] + k * size[2]]
                     for i in (0, 1) for j in (0, 1) for k in (0, 1)], np.float32)


def _scene(gt, preds):
    """gt: [(val_gt id, lo, size)], preds: [(label, score, lo, size)]: every box is the 8 corner points of a cuboid."""
    xyz = np.concatenate([_corners(lo, sz) for _, lo, sz in gt] + [_corners(lo, sz) for *_, lo, sz in preds])
    gt_ids = np.zeros(xyz.shape[0], np.int64)
    masks = np.zeros((len(preds), xyz.shape[0]), np.int32)
    for i, (gid, _, _) in enumerate(gt):
        gt_ids[8 * i:8 * i + 8] = gid
    for r in range(len(preds)):
        masks[r, 8 * (len(gt) + r):8 * (len(gt) + r) + 8] = 1
    return gt_ids, [p[0] for p in preds], [p[1] for p in preds], masks, None, xyz


CUBE = (1.0, 1.0, 1.0)


@pytest.mark.parametrize("kind", ["aligned", "oriented"])
def test_ap_of_tp_fp_tp_is_five_sixths(kind):
    from geoformer_amd import evaluation

    cid = int(evaluation.class_set(0)[0][0])
    name = evaluation.class_set(0)[1][0]
    gt = [(cid * 1000 + 1, (0, 0, 0), CUBE), (cid * 1000 + 2, (5, 0, 0), CUBE)]
    for second in ((0, 5, 0), (0.0, 0.125, 0.0)):  # off every instance / on the instance that .9 has claimed
        ev = evaluation.BoxEvaluator(classes=0, kind=kind)
        ev.add_scene("s", *_scene(gt, [(cid, 0.9, (0.125, 0, 0), CUBE), (cid, 0.8, second, CUBE),
                                      (cid, 0.7, (5, 0, 0.25), CUBE)]))
        res = ev.evaluate()
        for t in ("0.25", "0.5"):
            assert res["classes"][name]["ap@" + t] == pytest.approx(5 / 6, abs=1e-12)
            assert res["classes"][name]["recall@" + t] == 1.0
            assert res["mAP@" + t] == pytest.approx(5 / 6, abs=1e-12) and res["mAR@" + t] == 1.0
        # a class without ground truth is nan and left out of the means
        assert np.isnan(res["ap"][1:]).all() and np.isnan(res["recall"][1:]).all()
        assert res["ap"].shape == (9, 2) and res["kind"] == kind and res["overlaps"] == (0.25, 0.5)
        text = evaluation.format_box_results(res)
        assert "AP@0.25" in text and "AR@0.5" in text and "box " + kind in text and "0.833" in text and name in text
    with pytest.raises(ValueError):  # a scene's name is taken once
        ev.add_scene("s", *_scene(gt, []))


def test_an_iou_equal_to_the_threshold_is_no_match():
    from geoformer_amd import evaluation

    cid = int(evaluation.class_set(0)[0][0])
    gt = [(cid * 1000 + 1, (0, 0, 0), CUBE)]
    for depth, at in ((0.5, "0.5"), (0.25, "0.25")):
        ev = evaluation.BoxEvaluator(classes=0)
        ev.add_scene("s", *_scene(gt, [(cid, 0.9, (0, 0, 0), (1.0, 1.0, depth))]))
        assert ev.scene_tables()[0]["iou"].tolist() == [[depth]]  # exactly the threshold
        res = ev.evaluate()
        assert res["mAP@" + at] == 0.0 and res["mAR@" + at] == 0.0
        if at == "0.5":
            assert res["mAP@0.25"] == 1.0 and res["mAR@0.25"] == 1.0


def test_scenes_classes_and_min_points_keep_apart():
    from geoformer_amd import evaluation

    ids = evaluation.class_set(0)[0]
    c0, c1 = int(ids[0]), int(ids[1])
    # scene a: a prediction where scene b has its instance; a's own instance is elsewhere
    ev = evaluation.BoxEvaluator(classes=0)
    ev.add_scene("a", *_scene([(c0 * 1000 + 1, (9, 9, 9), CUBE)], [(c0, 0.9, (0, 0, 0), CUBE)]))
    ev.add_scene("b", *_scene([(c0 * 1000 + 1, (0, 0, 0), CUBE)], []))
    res = ev.evaluate()
    assert res["mAP@0.25"] == 0.0 and res["mAR@0.25"] == 0.0
    # a prediction of another class on the instance is no match either; both classes then have ground truth
    ev = evaluation.BoxEvaluator(classes=0)
    ev.add_scene("a", *_scene([(c0 * 1000 + 1, (0, 0, 0), CUBE), (c1 * 1000 + 2, (3, 0, 0), CUBE), (1000 + 3, (6, 0, 0), CUBE)],
                              [(c1, 0.9, (0, 0, 0), CUBE), (c1, 0.5, (3, 0, 0), CUBE)]))
    res = ev.evaluate()
    assert res["ap"][0, 0] == 0.0 and res["ap"][1, 0] == 0.5 and res["mAP@0.25"] == 0.25
    t = ev.scene_tables()[0]
    assert t["gt_id"].tolist() == [c0 * 1000 + 1, c1 * 1000 + 2]  # ascending; wall (class 1) is not in the set
    assert t["gt_count"].tolist() == [8, 8] and t["count"].tolist() == [8, 8] and t["iou"].shape == (2, 2)
    # min_points drops instances and predictions below it
    ev = evaluation.BoxEvaluator(classes=0, min_points=9)
    ev.add_scene("a", *_scene([(c0 * 1000 + 1, (0, 0, 0), CUBE)], [(c0, 0.9, (0, 0, 0), CUBE)]))
    assert np.isnan(ev.evaluate()["mAP@0.25"])


def test_ties_in_score_keep_scene_order_then_pick_rank():
    from geoformer_amd import evaluation

    cid = int(evaluation.class_set(0)[0][0])
    ev = evaluation.BoxEvaluator(classes=0)
    gt = [(cid * 1000 + 1, (0, 0, 0), CUBE)]
    # equal scores: the first in pick order claims the instance although the second overlaps it more
    ev.add_scene("a", *_scene(gt, [(cid, 0.5, (0.25, 0, 0), CUBE), (cid, 0.5, (0, 0, 0), CUBE)]))
    res = ev.evaluate()
    assert res["ap"][0].tolist() == [1.0, 1.0]  # TP then FP: precision 1 at recall 1


# ---- tables, files, edges -------------------------------------------------------------------------------------------------
def test_scene_table_builders():
    from geoformer_amd import postprocess

    t, sizes = postprocess.box_scene_table(["rows", "ids", "rows"], [100, 0, 7], [5, 0, 0], [3, 0, 4], [11, 0, 0],
                                           [12, 0, 13], [14, 0, 15])
    assert t.shape == (3, postprocess.BOX_SCENE_FIELDS) and t.dtype == np.int64 and postprocess.BOX_SCENE_FIELDS == 8
    assert t[:, 0].tolist() == [postprocess.BOX_FORMS["rows"], postprocess.BOX_FORMS["ids"], postprocess.BOX_FORMS["rows"]]
    assert t[:, 1:4].tolist() == [[100, 5, 3], [0, 0, 0], [7, 0, 4]] and t[:, 4:7].tolist() == [[11, 12, 14], [0, 0, 0], [0, 13, 15]]
    assert t[:, 7].tolist() == [0, 3, 3] and sizes == {"rows": 7, "max_points": 100, "max_groups": 4}
    t, sizes = postprocess.box_scene_table([], [], [], [], [], [], [])
    assert t.shape == (0, 8) and sizes == {"rows": 0, "max_points": 0, "max_groups": 0}
    for bad in (([-1], [0], [0]), ([1], [-2], [0]), ([1], [0], [-3])):
        with pytest.raises(ValueError):
            postprocess.box_scene_table(["rows"], *bad, [0], [0], [0])
    with pytest.raises(ValueError):
        postprocess.box_scene_table(["ids"], [1], [0], [postprocess.BOX_MAX_GROUPS + 1], [0], [0], [0])
    t, sizes = postprocess.box_iou_table([7, 0, 2], [5, 3, 0])
    assert t.tolist() == [[7, 5, 0, 0, 0], [0, 3, 7, 5, 35], [2, 0, 7, 8, 35]]
    assert sizes == {"a": 9, "b": 8, "out": 35, "max_pairs": 35} and postprocess.BOX_FLOATS == 10
    with pytest.raises(ValueError):
        postprocess.box_iou_table([1], [-1])


def test_write_boxes_round_trips(tmp_path):
    from geoformer_amd import export, postprocess

    rng = np.random.default_rng(9)
    case = member_count_ids_case(rng, 64, (5, 0, 40), scale=30.0)
    b = postprocess.id_boxes(case["group"], 3, case["xyz"], oriented=True)
    path = export.write_boxes(str(tmp_path / "sub" / "scene.txt"), b, [3, 4, 39], [0.5, 0.0, 0.123456789])
    lines = open(path).read().splitlines()
    assert len(lines) == 3 and all(len(x.split()) == 9 for x in lines)
    a = np.array([[float(v) for v in x.split()] for x in lines])
    center, size, yaw, labels, scores = a[:, 0:3], a[:, 3:6], a[:, 6], a[:, 7].astype(np.int64), a[:, 8]
    assert np.allclose(center, b.center, rtol=1e-8, atol=1e-9) and np.allclose(size, b.size, rtol=1e-8, atol=1e-9)
    assert np.allclose(yaw, b.yaw, rtol=1e-8) and labels.tolist() == [3, 4, 39]
    assert np.allclose(scores, [0.5, 0.0, 0.123457], atol=1e-9)
    with pytest.raises(ValueError):
        export.write_boxes(path, b, [3, 4], [0.5, 0.0, 0.1])


def test_box_points_are_the_twelve_edges():
    from geoformer_amd import postprocess, render

    b = postprocess._boxes_from_rows(box_rows(((1.0, 2.0, 3.0), (2.0, 1.0, 0.5), table_entry(30)), UNIT),
                                     np.array([1, 1], np.int32), 90)
    corners = render.box_corners(b)
    assert corners.shape == (2, 8, 3)
    c, s = table_entry(30)
    want = {(round(1 + su * c - sv * 0.5 * s, 9), round(2 + su * s + sv * 0.5 * c, 9), 3 + sz * 0.25)
            for su in (-1, 1) for sv in (-1, 1) for sz in (-1, 1)}
    assert {(round(x, 9), round(y, 9), z) for x, y, z in corners[0].tolist()} == want
    xyz, rgb = render.box_points(b, step=0.5, rgb=[(255, 0, 0), (0, 0, 255)])
    assert xyz.dtype == np.float32 and rgb.dtype == np.uint8 and xyz.shape == rgb.shape
    # box 0: edges of 2.0, 1.0 and 0.5 at step 0.5: 5, 3 and 2 points, four edges each; box 1: 3 points on each of 12
    n0 = 4 * (5 + 3 + 2)
    assert xyz.shape[0] == n0 + 12 * 3 and (rgb[:n0] == (255, 0, 0)).all() and (rgb[n0:] == (0, 0, 255)).all()
    # every edge's end points are corners, and the 12 edges are the cuboid's: each corner ends three edges, four edges
    # of every length
    at, lengths, deg = 0, [], np.zeros(8, int)
    for i, j in render.BOX_EDGES:
        a, e = corners[0, i], corners[0, j]
        k = int(np.ceil(np.linalg.norm(e - a) / 0.5)) + 1
        assert np.allclose(xyz[at], a, atol=1e-6) and np.allclose(xyz[at + k - 1], e, atol=1e-6)
        at += k
        lengths.append(np.linalg.norm(e - a))
        deg[i] += 1
        deg[j] += 1
    assert at == n0 and (deg == 3).all() and np.allclose(sorted(lengths), [0.5] * 4 + [1.0] * 4 + [2.0] * 4, atol=1e-9)
    assert render.box_points(b._replace(center=b.center[:0], size=b.size[:0], cos=b.cos[:0], sin=b.sin[:0]))[0].shape == (0, 3)
    with pytest.raises(ValueError):
        render.box_points(b, step=0.0)
