"""gf_semantic_confusion (csrc/semantic_eval.hip) against its numpy statement (evaluation.semantic_confusion_host), the
evaluator on device tensors, and the batched loops of batch_eval that feed it.  All comparisons are exact."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
RAW_VALUES = np.array([-100, -1] + list(range(20)) + [25], np.int64)
BIG = 150_269


def limits():
    from geoformer_amd import pointops

    return pointops.semantic_confusion_limits()


def make_scores(rng, N, C, kind):
    """normal: floats without ties; ties: values from {-1, 0, 1}, so most rows tie.  Both carry the rows whose arg-max
    needs the rule: NaN in column 0, NaN in a later column, +inf twice, all -inf, all equal."""
    if kind == "normal":
        s = rng.standard_normal((N, C)).astype(np.float32)
    else:
        s = rng.integers(-1, 2, (N, C)).astype(np.float32)
    last = C - 1
    for j, i in enumerate(range(0, N, 7)):
        k = j % 6
        if k == 0:
            s[i, 0] = NAN
        elif k == 1:
            s[i, last] = NAN  # (C = 1: column 0)
        elif k == 2:
            s[i, rng.integers(0, C)] = INF
            s[i, rng.integers(0, C)] = INF
        elif k == 3:
            s[i, :] = -INF
        elif k == 4:
            s[i, :] = s[i, 0]
        else:
            s[i, C // 2] = NAN
            s[i, 0] = -INF
    return s


def splits(rng, N, run):
    """Scene offsets over N points: one scene; empty scenes first, in the middle and last; 40 scenes of 0-3 points inside
    one run; boundaries exactly on a run's edge and one point either side of it."""
    out = {"one": [0, N], "empties": [0, 0, N // 2, N // 2, N // 2, N, N]}
    start = min(N, (N // 2 // run) * run + 7)
    tiny = np.minimum(start + np.cumsum(rng.integers(0, 4, 40)), N)
    out["tiny40"] = [0, start] + tiny.tolist() + [N]
    edge = sorted(min(N, e) for e in (run - 1, run, run + 1, 2 * run, 2 * run + 1, (N // run) * run, (N // run) * run - 1)
                  if e >= 0)
    out["run_edges"] = [0] + edge + [N]
    return {k: np.asarray(v, np.int32) for k, v in out.items()}


def label_kinds(rng, N, C):
    from geoformer_amd import evaluation as E

    raw = RAW_VALUES[rng.integers(0, len(RAW_VALUES), N)]
    ident = np.array([-100, -1, C, 25] + list(range(C)), np.int64)[rng.integers(0, C + 4, N)]
    out = {}
    for fold in (0, 1):
        lut, mi, mo = E.semantic_label_lut(fold)
        out[f"raw{fold}"] = (raw, lut, mi, mo)
    out["identity"] = (ident, None, -1, -1)
    return out


def native(scores_d, labels, offsets, lut, mi, mo, calls=1, want_preds=True):
    from geoformer_amd import pointops

    N, C = scores_d.shape
    off_h = torch.from_numpy(np.ascontiguousarray(offsets))
    conf = torch.zeros((len(offsets) - 1, C + 1, C), dtype=torch.int64, device="cuda")
    lut_d = None if lut is None else torch.from_numpy(lut).cuda()
    for _ in range(calls):
        preds = pointops.semantic_confusion(scores_d, torch.from_numpy(labels).cuda(), off_h.cuda(), conf, lut=lut_d,
                                            ignore_label=-100, map_ignore=mi, map_other=mo, want_preds=want_preds,
                                            offsets_host=off_h)
    return preds, conf


@pytest.mark.parametrize("n", ["0", "1", "63", "64", "65", "run-1", "run", "run+1", str(BIG)])
@pytest.mark.parametrize("c", ["2", "13", "20", "bound"])
def test_kernel_equals_numpy(hip, c, n):
    from geoformer_amd import evaluation as E

    max_c, run = limits()
    C = max_c if c == "bound" else int(c)
    N = {"run-1": run - 1, "run": run, "run+1": run + 1}.get(n) or int(n)
    rng = np.random.default_rng(1000 * C + N % 997)
    labs = label_kinds(rng, N, C)
    offs = splits(rng, N, run)
    for kind in ("normal", "ties"):
        scores = make_scores(rng, N, C, kind)
        want_preds = E.semantic_preds_host(scores)
        scores_d = torch.from_numpy(scores).cuda()
        for lname, (labels, lut, mi, mo) in labs.items():
            for sname, offsets in offs.items():
                preds, conf = native(scores_d, labels, offsets, lut, mi, mo)
                p2, want = E.semantic_confusion_host(scores, labels, offsets, lut=lut, map_ignore=mi, map_other=mo)
                what = (kind, lname, sname)
                assert preds.dtype == torch.int32 and (preds.cpu().numpy() == want_preds).all(), what
                assert (p2 == want_preds).all()
                got = conf.cpu().numpy()
                assert (got == want).all(), what
                assert (got.sum((1, 2)) == np.diff(offsets)).all(), what


def test_every_point_in_one_bin(hip):
    """All points of four runs and a bit in bin (0, 0): LDS and global atomics under full contention."""
    _, run = limits()
    N = 4 * run + 17
    scores_d = torch.zeros((N, 13), device="cuda")  # every row ties: class 0
    preds, conf = native(scores_d, np.zeros(N, np.int64), np.array([0, N], np.int32), None, -1, -1)
    assert int(conf[0, 0, 0]) == N and int(conf.sum()) == N and int(preds.abs().sum()) == 0
    # the same points spread over three scenes whose boundaries sit inside runs
    off = np.array([0, run + 3, run + 3, 3 * run - 1, N], np.int32)
    _, conf = native(scores_d, np.zeros(N, np.int64), off, None, -1, -1)
    assert conf[:, 0, 0].tolist() == np.diff(off).tolist() and int(conf.sum()) == N


def test_accumulation_and_optional_outputs(hip):
    from geoformer_amd import evaluation as E
    from geoformer_amd import pointops

    _, run = limits()
    rng = np.random.default_rng(11)
    N, C = 3 * run + 5, 13
    scores = make_scores(rng, N, C, "ties")
    labels, lut, mi, mo = label_kinds(rng, N, C)["raw0"]
    offsets = splits(rng, N, run)["tiny40"]
    _, want = E.semantic_confusion_host(scores, labels, offsets, lut=lut, map_ignore=mi, map_other=mo)
    scores_d = torch.from_numpy(scores).cuda()
    for calls in (1, 2, 3):
        _, conf = native(scores_d, labels, offsets, lut, mi, mo, calls=calls)
        assert (conf.cpu().numpy() == calls * want).all()
        assert (conf.sum((1, 2)).cpu().numpy() == calls * np.diff(offsets)).all()
    # no preds wanted: none allocated, the counts are the same
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    conf = torch.zeros((len(offsets) - 1, C + 1, C), dtype=torch.int64, device="cuda")
    labels_d, off_d, lut_d = torch.from_numpy(labels).cuda(), torch.from_numpy(offsets).cuda(), torch.from_numpy(lut).cuda()
    held = torch.cuda.memory_allocated()
    none = pointops.semantic_confusion(scores_d, labels_d, off_d, conf, lut=lut_d, map_ignore=mi, map_other=mo,
                                       want_preds=False)
    assert none is None and torch.cuda.memory_allocated() == held > before
    assert (conf.cpu().numpy() == want).all()
    # labels=None: preds only, conf is not touched (the native entry is given the matrix all the same)
    conf.fill_(7)
    preds = torch.full((N,), -1, dtype=torch.int32, device="cuda")
    rc = hip.gf_semantic_confusion(scores_d.data_ptr(), None, off_d.data_ptr(), None, len(offsets) - 1, N, C, None, 0, -100,
                                   -1, -1, preds.data_ptr(), conf.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0 and (conf == 7).all() and (preds.cpu().numpy() == E.semantic_preds_host(scores)).all()
    p2 = pointops.semantic_confusion(scores_d, None, None, None)
    assert torch.equal(p2, preds)


def test_argument_checks(hip):
    max_c, _ = limits()
    N, C = 100, 13
    scores = torch.zeros((N, max_c + 1), device="cuda")
    labels = torch.zeros(N, dtype=torch.int64, device="cuda")
    off = torch.tensor([0, 40, 100], dtype=torch.int32)
    off_d = off.cuda()
    preds = torch.full((N,), -1, dtype=torch.int32, device="cuda")
    conf = torch.zeros((2, max_c + 2, max_c + 1), dtype=torch.int64, device="cuda")

    def call(scores_p=scores.data_ptr(), n=N, c=C, host=off, labels_p=labels.data_ptr(), off_p=off_d.data_ptr(),
             conf_p=conf.data_ptr(), s=2):
        return hip.gf_semantic_confusion(scores_p, labels_p, off_p, None if host is None else host.data_ptr(), s, n, c,
                                         None, 0, -100, -1, -1, preds.data_ptr(), conf_p, None)

    assert call() == 0
    bad = {"C above the bound": dict(c=max_c + 1), "C = 0": dict(c=0), "N < 0": dict(n=-1),
           "descending offsets": dict(host=torch.tensor([0, 120, 100], dtype=torch.int32)),
           "offsets[S] != N": dict(host=torch.tensor([0, 40, 99], dtype=torch.int32)),
           "offsets[0] != 0": dict(host=torch.tensor([1, 40, 100], dtype=torch.int32)),
           "null scores": dict(scores_p=None), "null offsets": dict(off_p=None), "null conf": dict(conf_p=None),
           "no scene": dict(s=0, host=None)}
    torch.cuda.synchronize()
    conf.zero_()
    preds.fill_(-1)
    for what, kw in bad.items():
        assert call(**kw) < 0, what
        assert b"gf_semantic_confusion" in hip.gf_last_error(), what
    torch.cuda.synchronize()
    assert int(conf.sum()) == 0 and (preds == -1).all()  # nothing was launched
    assert call(scores_p=None, n=0, host=torch.tensor([0, 0, 0], dtype=torch.int32)) == 0  # no points: no scores needed


@pytest.mark.parametrize("cls,equal", [(4, False), (3, True)])
def test_same_points_as_the_forwards_filter(hip, cls, equal):
    """The foreground the instance stage is given (gf_fg_select) is `preds >= 4` (`preds == 3` across folds), on rows
    full of ties, NaNs and infinities."""
    from geoformer_amd import pointops

    rng = np.random.default_rng(4097)
    N, C = 4097, 13
    scores = torch.from_numpy(make_scores(rng, N, C, "ties")).cuda()
    locs = torch.rand((N, 3), device="cuda")
    bidx = torch.zeros(N, dtype=torch.int32, device="cuda")
    feats = torch.rand((N, 16), device="cuda")
    fg = pointops.select_foreground(scores, cls, equal, locs, bidx, feats)[0]
    preds = pointops.semantic_confusion(scores, None, None, None)
    want = torch.nonzero(preds == cls if equal else preds >= cls).flatten()
    assert 0 < want.numel() < N and torch.equal(fg, want)


def test_add_batch_reads_nothing_back(hip):
    """SemanticEvaluator.add_batch on device tensors queues its work and returns: under torch's sync debug mode, which
    raises on every synchronising call (a device-to-host copy among them), two batches go through; evaluate() is the
    one place the host reads."""
    from geoformer_amd import evaluation as E

    rng = np.random.default_rng(3)
    N, C = 5000, 13
    scores = make_scores(rng, N, C, "normal")
    raw = RAW_VALUES[rng.integers(0, len(RAW_VALUES), N)]
    off = np.array([0, 1234, 1234, N], np.int32)
    sd, ld, od = torch.from_numpy(scores).cuda(), torch.from_numpy(raw).cuda(), torch.from_numpy(off).cuda()
    ev = E.SemanticEvaluator(train_fold=1)
    tot = E.SemanticEvaluator(train_fold=1, keep_scenes=False)
    for e in (ev, tot):
        e.add_batch(sd, ld, od, ["a", "b", "c"])  # (the label table is uploaded by the first call)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for e in (ev, tot):
            preds = e.add_batch(sd, ld, od, ["d", "e", "f"])
        with pytest.raises(RuntimeError):
            preds.cpu()  # (the mode is armed: a read-back raises)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    lut, mi, mo = E.semantic_label_lut(1)
    p, want = E.semantic_confusion_host(scores, raw, off, lut=lut, map_ignore=mi, map_other=mo)
    assert preds.is_cuda and (preds.cpu().numpy() == p).all()
    per = ev.scene_confusions()
    assert list(per) == list("abcdef") and all((per[k] == want[i % 3]).all() for i, k in enumerate("abcdef"))
    assert (ev.confusion() == 2 * want.sum(0)).all() and (tot.confusion() == 2 * want.sum(0)).all()
    assert ev.evaluate()["miou"] == E.semantic_metrics(2 * want.sum(0))["miou"]
    # host arrays through the same evaluator interface: the numpy path, the same integers
    hv = E.SemanticEvaluator(train_fold=1)
    hv.add_batch(scores, raw, off, ["a", "b", "c"])
    assert all((hv.scene_confusions()[k] == per[k]).all() for k in "abc")


# ---- through the model ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(hip):
    from geoformer_amd.model import GeoFormer, load_config
    from tests.util import synthetic_state_dict

    m = GeoFormer(load_config("test_geoformer_scannet.yaml"))
    m.load_state_dict(synthetic_state_dict(m.state_dict(), 0))
    m.cuda()
    m.eval()
    return m


@pytest.fixture(scope="module")
def scenes():
    from geoformer_amd import batch_eval, scene

    items = [(f"scene{i:02d}", scene.make_raw_scene(7000 + 1000 * i, 60 + i, n_boxes=1, room=(1.6, 1.6, 0.6)))
             for i in range(3)]
    shape = np.max([b["spatial_shape"] for B in (1, 3) for b in batch_eval.collate_batches(items, B)[1]], axis=0)
    return items, shape


def _same(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)


def test_evaluate_semantic_equals_numpy_on_the_forwards_scores(model, scenes):
    """evaluate_semantic runs the fused voxel-row semantic head (forward_backbone(want_preds=False)); the scores it is
    compared with come from the unfused head of the early-return forward.  The exact comparison rests on the two routes
    giving the same bits (tests/test_gpu_heads.py test_pointwise_mlp_row_indirection asserts that of the operator): if
    that ever stops holding, this test fails on near-tied rows without the evaluation being wrong."""
    from geoformer_amd import batch_eval
    from geoformer_amd import evaluation as E
    from geoformer_amd.feeder import DeviceFeeder

    items, shape = scenes
    fold = model.cfg.train_fold
    ev = E.SemanticEvaluator(n_classes=model.cfg.classes, train_fold=fold)
    res = batch_eval.evaluate_semantic(model, items, 3, spatial_shape=shape, reserve=False, evaluator=ev)
    _, hb = batch_eval.collate_batches(items, 3, shape)
    batch = next(iter(DeviceFeeder(hb, "cuda")))
    with torch.no_grad():
        out = model(batch, model.prepare_epochs, training=False)
    assert set(out) == {"semantic_scores"}  # the early return of the pretrain stage
    scores = out["semantic_scores"].cpu().numpy()
    lut, mi, mo = E.semantic_label_lut(fold)
    preds, want = E.semantic_confusion_host(scores, batch["labels"].cpu().numpy(), hb[0]["offsets"].numpy(), lut=lut,
                                            map_ignore=mi, map_other=mo)
    per = ev.scene_confusions()
    assert list(per) == [n for n, _ in items]
    for i, (name, raw) in enumerate(items):
        assert (per[name] == want[i]).all() and per[name].sum() == raw.shape[0], name
    ref = E.semantic_metrics(want.sum(0), E.SEMANTIC_CLASS_NAMES(fold))
    assert _same(res["iou"], ref["iou"])
    for k in ("miou", "miou_fold", "acc", "macc"):
        assert _same(res[k], ref[k]), k
    assert res["foreground"].keys() == res["candidate"].keys() == {"precision", "recall", "iou"}
    assert len(np.unique(preds)) > 1  # (the synthetic head does decide between classes)
    # the per-scene predictions of the loop are the same integers
    got = list(batch_eval.semantic_batches(model, items, 3, spatial_shape=shape, reserve=False))
    assert [n for n, _ in got] == [n for n, _ in items]
    assert (torch.cat([p for _, p in got]).cpu().numpy() == preds).all() and got[0][1].dtype == torch.int32


def test_evaluate_with_semantic_leaves_ap_alone(model, scenes):
    from geoformer_amd import batch_eval
    from geoformer_amd import evaluation as E

    items, shape = scenes
    kw = dict(classes=0, spatial_shape=shape, reserve=False, final_score_thresh=0.0, epoch=300)
    np.random.seed(21)
    ap0, avg0 = batch_eval.evaluate(model, items, 3, **kw)
    ev = E.SemanticEvaluator(n_classes=model.cfg.classes, train_fold=model.cfg.train_fold)
    np.random.seed(21)
    ap1, avg1 = batch_eval.evaluate(model, items, 3, semantic=ev, **kw)
    assert _same(ap0, ap1)
    for k in ("all_ap", "all_ap_50%", "all_ap_25%"):
        assert _same(avg0[k], avg1[k]), k
    per = ev.scene_confusions()
    assert {n: int(c.sum()) for n, c in per.items()} == {n: raw.shape[0] for n, raw in items}
    assert ev.evaluate()["points"] == sum(raw.shape[0] for _, raw in items)


def test_batch_size_does_not_change_a_scenes_matrix(model, scenes):
    from geoformer_amd import batch_eval
    from geoformer_amd import evaluation as E

    items, shape = scenes
    per = {}
    for B in (1, 3):
        ev = E.SemanticEvaluator(n_classes=model.cfg.classes, train_fold=model.cfg.train_fold)
        batch_eval.evaluate_semantic(model, items, B, spatial_shape=shape, reserve=False, evaluator=ev)
        per[B] = ev.scene_confusions()
    for name, _ in items:
        assert (per[1][name] == per[3][name]).all(), name
