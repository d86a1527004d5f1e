"""GPU: the box kernels (csrc/boxes.hip) against the numpy statements, np.array_equal on every output word -- counts,
both box kinds, IoU blocks -- at the smallest shapes that reach each regime (c = gf_box_chunk()); batched against
stand-alone; BoxEvaluator on the device against the numpy path; batch_eval.evaluate_boxes end to end."""
import numpy as np
import pytest
import torch

from tests.box_cases import (host_rows, ids_case, iou_pairs, lattice, member_count_ids_case, member_count_rows_case,
                             member_counts, mixed_iou_case, rows_case, scene_xyz)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def limits(hip):
    from geoformer_amd import pointops

    c, max_angles, max_groups = pointops.box_limits()
    assert c >= 256 and max_angles >= 90
    return c, max_angles


def _spec(case, dev="cuda"):
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    if case["form"] == "rows":
        masks = t(case["masks"]) if case["masks"].shape[0] else []  # no masks: a null pointer
        return ("rows", masks, t(case["pick"]), t(case["xyz"]))
    return ("ids", t(case["group"]), case["n_groups"], t(case["xyz"]))


def _device_rows(cases, angles):
    """One batched call over the cases: per case (count, aligned, oriented) as numpy arrays."""
    from geoformer_amd import postprocess

    table, count, aligned, oriented = postprocess._boxes_packed([_spec(c) for c in cases], angles)
    count, aligned, oriented = count.cpu().numpy(), aligned.cpu().numpy(), oriented.cpu().numpy()
    out = []
    for t in table:
        p, o = int(t[3]), int(t[7])
        out.append((count[o:o + p], aligned[o:o + p], oriented[o:o + p]))
    return out


def _same(got, want, what=""):
    for g, w, k in zip(got, want, ("count", "aligned", "oriented")):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k)
        assert np.array_equal(g, w), (what, k, np.argwhere(g != w)[:4].tolist())


def _regime_cases(c):
    rng = np.random.default_rng(17)
    counts = member_counts(c)
    return {
        "rows: member counts around the wave and the chunk, overlapping masks, other values, picks out of range":
            member_count_rows_case(rng, c),
        "ids: the same counts, disjoint and scattered": member_count_ids_case(rng, c, counts),
        "ids: magnitudes around 1e3": member_count_ids_case(rng, c, (65, c + 1, 3), scale=300.0, shift=(-900.0, 1100.0, 40.0)),
        "rows: magnitudes around 1e3, negative": member_count_rows_case(rng, 130, scale=200.0, shift=(-1500.0, -800.0, -30.0)),
        "ids: all -1": ids_case(np.full(c + 9, -1), 3, scene_xyz(rng, c + 9)),
        "ids: every point in one group": ids_case(np.zeros(2 * c + 5, np.int32), 1, scene_xyz(rng, 2 * c + 5)),
        "ids: ids outside [-1, p) name no group": ids_case(rng.integers(-3, 6, 300), 3, scene_xyz(rng, 300)),
        "rows: p = 0": rows_case(np.ones((2, 70)), [], scene_xyz(rng, 70)),
        "rows: n = 0, a null masks pointer": rows_case(np.zeros((0, 90)), [0, 1, -1], scene_xyz(rng, 90)),
        "ids: no points": ids_case(np.zeros(0), 2, np.zeros((0, 3))),
        "ids: a footprint of 0 at every heading": ids_case([0, 0, 1], 2, [[0.3, -0.7, 0.0], [0.3, -0.7, 2.0], [1, 2, 3]]),
        "ids: the lattice at entry 30 and the diamond": ids_case(
            [0] * 15 + [1] * 4, 2, np.concatenate([lattice(30), [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0]]])),
    }


def test_every_regime_equals_the_statement_alone_and_batched(limits):
    c, _ = limits
    cases = _regime_cases(c)
    alone = {k: _device_rows([case], 90)[0] for k, case in cases.items()}
    for k, case in cases.items():
        _same(alone[k], host_rows(case, 90), k)
    k = "ids: the lattice at entry 30 and the diamond"
    assert alone[k][2][:, 8].tolist() == [30.0, 45.0] and alone[k][0].tolist() == [15, 4]
    k = "ids: a footprint of 0 at every heading"
    assert alone[k][2][0, 8] == 0.0 and alone[k][2][0, 3:6].tolist() == [0.0, 0.0, 2.0]
    # all scenes in one call: the packed offsets; each scene equals its stand-alone call, and the call repeats itself
    batched = _device_rows(list(cases.values()), 90)
    again = _device_rows(list(cases.values()), 90)
    for k, b, a in zip(cases, batched, again):
        _same(b, alone[k], k)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(b, a)), k


def test_four_scenes_of_different_shapes_in_one_call(limits):
    c, _ = limits
    rng = np.random.default_rng(23)
    cases = [member_count_rows_case(rng, 64), ids_case(np.zeros(0), 0, np.zeros((0, 3))),
             member_count_ids_case(rng, c, (c + 1, 0, 5)), rows_case(rng.integers(0, 2, (3, c + 77)), [2, 2, 0, 7], scene_xyz(rng, c + 77))]
    batched = _device_rows(cases, 90)
    assert [b[0].shape[0] for b in batched] == [11, 0, 3, 4]
    for i, (case, b) in enumerate(zip(cases, batched)):
        _same(b, host_rows(case, 90), i)
        _same(b, _device_rows([case], 90)[0], i)


def test_angle_counts(limits):
    c, max_angles = limits
    rng = np.random.default_rng(29)
    turned = np.concatenate([lattice(1, 2), lattice(77, 90, (0.0, 9.0, 0.0)), lattice(150, 192, (9.0, 0.0, 0.0))])
    cases = [member_count_ids_case(rng, c, (1, 64, c + 1)), member_count_rows_case(rng, 96),
             ids_case(np.repeat([0, 1, 2], 15), 3, turned)]  # lattices at entries of the 2-, 90- and 192-angle tables
    for A in (1, 2, 90, max_angles):
        got = _device_rows(cases, A)
        for i, case in enumerate(cases):
            _same(got[i], host_rows(case, A), (A, i))
        if A > 1:
            assert got[2][2][{2: 0, 90: 1, 192: 2}.get(A, 2), 8] == {2: 1, 90: 77}.get(A, 150 * A // 192)
        if A == 1:  # one heading: the aligned box exactly
            assert all(np.array_equal(g[1], g[2]) for g in got)
        assert all((g[2][:, 8] < A).all() and (g[1][:, 8] == 0).all() for g in got)


def test_public_calls_stay_on_the_device(limits):
    from geoformer_amd import postprocess

    rng = np.random.default_rng(31)
    case = member_count_rows_case(rng, 80)
    _, masks, pick, xyz = _spec(case)
    for oriented in (False, True):
        want = postprocess.instance_boxes(case["masks"], case["pick"], case["xyz"], oriented=oriented)
        for m in (masks, masks != 0, (masks != 0).to(torch.uint8)):  # int32, bool and uint8 masks
            got = postprocess.instance_boxes(m, pick, xyz, oriented=oriented)
            assert got.center.is_cuda and got.count.dtype == torch.int32 and got.angle_index.dtype == torch.int32
            for g, w, k in zip(got, want, got._fields):
                assert np.array_equal(g.cpu().numpy(), w), (oriented, k)
    ids = member_count_ids_case(rng, 80, (3, 0, 200))
    got = postprocess.id_boxes_batched([torch.from_numpy(ids["group"]).cuda()] * 2, [3, 3],
                                       [torch.from_numpy(ids["xyz"]).cuda()] * 2, oriented=True, angles=45)
    want = postprocess.id_boxes(ids["group"], 3, ids["xyz"], oriented=True, angles=45)
    for b in got:
        for g, w, k in zip(b, want, b._fields):
            assert np.array_equal(g.cpu().numpy(), w), k
    with pytest.raises(ValueError):
        postprocess.instance_boxes(masks, pick, xyz, angles=0)


# ---- IoU ------------------------------------------------------------------------------------------------------------------
def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_iou_equals_the_statement(limits):
    from geoformer_amd import postprocess

    pairs = iou_pairs()
    for a, b, want, tol in pairs:
        got = postprocess.box_iou(_cuda(a), _cuda(b))
        assert got.is_cuda and got.dtype == torch.float64
        got = got.cpu().numpy()
        assert np.array_equal(got, postprocess.box_iou_host(a, b))
        assert got[0, 0] == want if tol == 0.0 else abs(got[0, 0] - want) < tol
    # every hand-made box against every other in one block: both rules and pairs with exactly one s == 0
    every = np.concatenate([p[0] for p in pairs] + [p[1] for p in pairs])
    assert np.array_equal(postprocess.box_iou(_cuda(every), _cuda(every)).cpu().numpy(), postprocess.box_iou_host(every, every))
    # a 7 x 5 block of oriented boxes from the box kernel itself, the last of b axis-aligned
    rng = np.random.default_rng(8)
    a, b = mixed_iou_case(rng)
    one = ((a[:, 7] != 0)[:, None] != (b[:, 7] != 0)[None, :])
    assert one.any() and (~one).any()
    got = postprocess.box_iou(_cuda(a), _cuda(b)).cpu().numpy()
    want = postprocess.box_iou_host(a, b)
    assert got.shape == (7, 5) and np.array_equal(got, want) and (want > 0.01).sum() >= 5
    # P = 0, G = 0, and several scenes in one launch (one of them empty on either side)
    assert postprocess.box_iou(_cuda(a[:0]), _cuda(b)).shape == (0, 5)
    assert postprocess.box_iou(_cuda(a), _cuda(b[:0])).shape == (7, 0)
    blocks = postprocess.box_iou_batched([_cuda(a), _cuda(a[:0]), _cuda(b), _cuda(every)],
                                         [_cuda(b), _cuda(b), _cuda(a[:3]), _cuda(b[:0])])
    again = postprocess.box_iou_batched([_cuda(a), _cuda(a[:0]), _cuda(b), _cuda(every)],
                                        [_cuda(b), _cuda(b), _cuda(a[:3]), _cuda(b[:0])])
    assert [tuple(x.shape) for x in blocks] == [(7, 5), (0, 5), (5, 3), (every.shape[0], 0)]
    assert np.array_equal(blocks[0].cpu().numpy(), want)
    assert np.array_equal(blocks[2].cpu().numpy(), postprocess.box_iou_host(b, a[:3]))
    assert all(x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in zip(blocks, again))


def test_iou_of_boxes_from_the_box_kernel(limits):
    from geoformer_amd import postprocess

    rng = np.random.default_rng(37)
    case = member_count_ids_case(rng, 64, (40, 9, 33, 1, 70, 12, 25), scale=0.3)
    other = member_count_ids_case(rng, 64, (30, 50, 8, 21, 64), scale=0.3)
    a = postprocess.id_boxes(*_spec(case)[1:], oriented=True)
    b = postprocess.id_boxes(*_spec(other)[1:], oriented=True)
    got = postprocess.box_iou(a, b)  # Boxes in, the packed rows ride along
    assert got.is_cuda and got.shape == (7, 5)
    want = postprocess.box_iou_host(host_rows(case, 90)[2], host_rows(other, 90)[2])
    assert np.array_equal(got.cpu().numpy(), want) and (want > 0).sum() >= 10


# ---- evaluator and end to end -----------------------------------------------------------------------------------------------
def _eval_scene(rng, N, n_inst, n_pred, cid):
    """A scene of n_inst instances (clusters of points) and n_pred masks, each a noisy copy of an instance."""
    centres = rng.random((n_inst, 3)) * np.array([6.0, 6.0, 1.0])
    inst = rng.integers(-1, n_inst, N)
    xyz = (np.where(inst[:, None] >= 0, centres[np.maximum(inst, 0)], 3.0) + rng.standard_normal((N, 3)) * 0.3).astype(np.float32)
    gt = np.where(inst >= 0, np.asarray(cid)[np.maximum(inst, 0) % len(cid)] * 1000 + inst + 1, 0).astype(np.int64)
    gt[rng.random(N) < 0.05] = 1000 + 77  # wall: not in the class set
    of = rng.integers(0, n_inst, n_pred)
    masks = ((inst[None, :] == of[:, None]) & (rng.random((n_pred, N)) < 0.8)).astype(np.int32)
    masks[-1] = 0  # an empty mask
    labels = np.asarray(cid)[of % len(cid)].astype(np.int64)
    scores = rng.random(n_pred).astype(np.float32)
    pick = np.argsort(-scores, kind="stable")[:n_pred - 2].astype(np.int64)
    return gt, labels, scores, masks, pick, xyz


def _same_tables(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.keys() == y.keys() and x["name"] == y["name"]
        for k in x:
            if k != "name":
                assert x[k].dtype == y[k].dtype and np.array_equal(x[k], y[k]), (x["name"], k)


@pytest.mark.parametrize("kind", ["aligned", "oriented"])
def test_evaluator_on_the_device_keeps_the_same_tables(limits, kind):
    from geoformer_amd import evaluation

    rng = np.random.default_rng(41)
    cid = evaluation.class_set(0)[0][:3]
    scenes = [_eval_scene(rng, 3000, 6, 9, cid), _eval_scene(rng, 700, 2, 4, cid)]
    host, dev = evaluation.BoxEvaluator(0, kind, angles=30), evaluation.BoxEvaluator(0, kind, angles=30)
    for i, sc in enumerate(scenes):
        host.add_scene(f"s{i}", *sc)
        dev.add_scene(f"s{i}", *[torch.from_numpy(a).cuda() for a in sc])
    # a scene without proposals, as predict_batches yields it
    host.add_scene("none", scenes[1][0], [], [], [], np.zeros(0, np.int64), scenes[1][5])
    dev.add_scene("none", torch.from_numpy(scenes[1][0]).cuda(), [], [], [], torch.zeros(0, dtype=torch.int64),
                  torch.from_numpy(scenes[1][5]).cuda())
    _same_tables(host.scene_tables(), dev.scene_tables())
    np.testing.assert_equal(host.evaluate(), dev.evaluate())
    assert host.scene_tables()[0]["iou"].shape == (7, 6) and (host.scene_tables()[0]["iou"] > 0.25).any()
    assert 0.0 < host.evaluate()["mAR@0.25"] <= 1.0


@pytest.fixture(scope="module")
def model(hip):
    from geoformer_amd.model import GeoFormer, load_config
    from tests.util import synthetic_state_dict

    m = GeoFormer(load_config("test_geoformer_scannet.yaml"))
    m.load_state_dict(synthetic_state_dict(m.state_dict(), 0))
    m.cuda()
    m.eval()
    return m


def test_evaluate_boxes_end_to_end(model):
    """batch_eval.evaluate_boxes on two small synthetic scenes against the evaluator fed by hand, through the numpy
    path, from predict_batches' output; evaluate(boxes=) gives the same from the AP pass."""
    from geoformer_amd import batch_eval, evaluation, scene

    items = [(f"scene{i}", scene.make_raw_scene(5000 + 1500 * i, 60 + i, n_boxes=1, room=(1.6, 1.6, 0.6))) for i in range(2)]
    _, hb = batch_eval.collate_batches(items, 1)
    kw = dict(spatial_shape=np.max([b["spatial_shape"] for b in hb], axis=0), final_score_thresh=0.0)
    cvfold = model.cfg.cvfold
    np.random.seed(21)
    res = batch_eval.evaluate_boxes(model, items, 2, classes=cvfold, kind="oriented", angles=45, **kw)
    np.random.seed(21)
    ev = evaluation.BoxEvaluator(cvfold, "oriented", angles=45)
    picked = 0
    for name, cls, sc, masks, pick in batch_eval.predict_batches(model, items, 2, **kw):
        if not torch.is_tensor(cls):
            continue
        raw = dict(items)[name]
        gt = evaluation.gt_ids_from_labels(raw[:, 6].astype(np.int64), raw[:, 7].astype(np.int64))
        ev.add_scene(name, gt, evaluation.benchmark_label_ids(cls, cvfold).cpu().numpy(), sc.cpu().numpy(),
                     masks.cpu().numpy(), pick.cpu().numpy(), raw[:, :3].astype(np.float32))
        picked += int(pick.numel())
    print(f"evaluate_boxes: {len(ev.scenes)} scenes, {picked} picked masks")
    assert len(ev.scenes) >= 1
    np.testing.assert_equal(res, ev.evaluate())
    np.random.seed(21)
    both = evaluation.BoxEvaluator(cvfold, "oriented", angles=45)
    batch_eval.evaluate(model, items, 2, classes=cvfold, boxes=both, **kw)
    np.testing.assert_equal(both.evaluate(), res)
    _same_tables(both.scene_tables(), ev.scene_tables())
