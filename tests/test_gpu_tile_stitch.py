"""GPU: the tile stitch kernel (csrc/tile_stitch.hip) bit for bit against the host statement
(postprocess.stitch_tiles_host) at the shapes where it can go wrong, its argument checks, and stitch= end to end through
predict_batches, panoptic_batches, evaluate_panoptic and semantic_batches."""
import numpy as np
import pytest
import torch

from tests.tile_stitch_cases import (MODES, edge_plan, gap_plan, hand_plan_in_range, random_scores, scan, uniform_plan)

pytestmark = pytest.mark.gpu


def _dev(scores):
    return [None if x is None else torch.from_numpy(x).cuda() for x in scores]


def _check(plan, scores):
    """Both modes of the kernel against the host statement, bit patterns, each run twice."""
    from geoformer_amd import postprocess

    out = {}
    for mode in MODES:
        want = torch.from_numpy(postprocess.stitch_tiles_host(plan, scores, mode))
        runs = [postprocess.stitch_tiles(plan, _dev(scores), mode) for _ in range(2)]
        torch.cuda.synchronize()
        for got in runs:
            assert got.is_cuda and got.dtype == torch.float32 and got.shape == want.shape and got.is_contiguous()
            assert torch.equal(got.cpu().view(torch.int32), want.view(torch.int32)), mode
        assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32)), mode
        out[mode] = want.numpy()
    return out


@pytest.mark.parametrize("C", [1, 13, 20, 64])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257, 4000])
def test_kernel_equals_statement(hip, N, C):
    """N * C floats end inside a wave, on a wave, past a workgroup (256 points) and, at 4000, over 16 workgroups on the
    3 x 3 plan; at C = 13 and 20 a point's row straddles waves."""
    from geoformer_amd import pointops

    assert pointops.tile_stitch_limits() == 64
    plan = uniform_plan(n=N)
    assert plan.N == N and (N < 4000 or plan.T == 9)
    out = _check(plan, random_scores(plan, C, seed=N + C))
    if N == 4000:
        assert not np.array_equal(out["core"], out["mean"])


def test_one_tile_zero_halo_empty_tile_and_edges(hip):
    plan = uniform_plan(n=700, tile=100.0)
    assert plan.T == 1
    scores = random_scores(plan, 13, seed=1)
    out = _check(plan, scores)
    assert np.array_equal(out["core"], scores[0]) and np.array_equal(out["mean"], scores[0])
    plan = uniform_plan(n=1500, halo=0.0)
    out = _check(plan, random_scores(plan, 13, seed=2))
    assert np.array_equal(out["core"].view(np.int32), out["mean"].view(np.int32))
    plan = gap_plan()
    for empty in ("none", "zero"):
        _check(plan, random_scores(plan, 20, seed=3, empty=empty))
    _check(edge_plan()[0], random_scores(edge_plan()[0], 20, seed=4))


def test_hand_table_count_3_and_no_slot(hip):
    """A point in three tiles: the sequential sum and the correctly rounded division by 3; a point without a slot."""
    plan = hand_plan_in_range()
    for seed in range(8):  # 8 x 13 quotients by 3
        scores = random_scores(plan, 13, seed=seed)
        out = _check(plan, scores)
        want = ((scores[0][1] + scores[1][2]) + scores[2][0]) / np.float32(3)
        assert np.array_equal(out["mean"][0].view(np.int32), want.view(np.int32))
        assert not out["mean"][1].any() and not out["core"][1].any()


def test_no_points_and_argument_checks_launch_nothing(hip):
    from geoformer_amd import _lib, pointops, postprocess

    plan = uniform_plan(n=300, extent=(6.0, 3.0))
    assert plan.T == 2
    scores = _dev(random_scores(plan, 13, seed=5))
    st = _lib.stream_ptr()
    table = np.array([[scores[0].data_ptr(), scores[0].shape[0]], [scores[1].data_ptr(), scores[1].shape[0]]], np.int64)
    table_d = torch.from_numpy(table).cuda()
    tile_of, local_of = torch.from_numpy(plan.tile_of).cuda(), torch.from_numpy(plan.local_of).cuda()
    core_of = torch.from_numpy(plan.core_of).cuda()
    out = torch.full((plan.N, 13), 7.0, device="cuda")

    def call(th=table, T=2, N=plan.N, C=13, mode=0):
        return hip.gf_tile_stitch_scores(table_d.data_ptr(), th.ctypes.data, T, tile_of.data_ptr(), local_of.data_ptr(),
                                         core_of.data_ptr(), N, C, mode, out.data_ptr(), st)

    # N == 0 returns at once and writes nothing
    assert call(N=0) == 0
    empty = plan._replace(tile_of=plan.tile_of[:0], local_of=plan.local_of[:0], core_of=plan.core_of[:0],
                          offsets=np.zeros(3, np.int64), index=np.zeros(0, np.int64))
    got = postprocess.stitch_tiles(empty, [x[:0] for x in scores], "mean")
    assert got.shape == (0, 13) and got.is_cuda
    bad = table.copy()
    bad[1, 1] = -1
    assert call(th=bad) == -1  # a negative n_s
    bad = table.copy()
    bad[0, 0] = 0
    assert call(th=bad) == -1  # NULL scores with n_s > 0
    assert call(T=0) == -1 and call(T=65536) == -1
    assert call(C=0) == -1 and call(C=65) == -1
    assert call(mode=2) == -1 and call(mode=-1) == -1
    assert call(N=-1) == -1
    torch.cuda.synchronize()
    assert (out == 7.0).all()  # none of them launched
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), torch.from_numpy(postprocess.stitch_tiles_host(plan, [x.cpu().numpy() for x in scores],
                                                                                 "core")))
    # the wrappers, before any launch
    short = [scores[0][:-1], scores[1]]
    with pytest.raises(ValueError, match="tile 0"):
        postprocess.stitch_tiles(plan, short, "core")
    with pytest.raises(ValueError, match="contiguous"):
        postprocess.stitch_tiles(plan, [scores[0].t().contiguous().t(), scores[1]], "core")
    with pytest.raises(RuntimeError, match="C = 65"):
        pointops.tile_stitch_scores(table_d, table, tile_of, local_of, core_of, 65, "core")
    with pytest.raises(RuntimeError, match="core_of"):
        pointops.tile_stitch_scores(table_d, table, tile_of, local_of, core_of[:-1], 13, "core")
    with pytest.raises(RuntimeError, match="table"):
        pointops.tile_stitch_scores(table_d[:1], table, tile_of, local_of, core_of, 13, "core")


# ---- end to end ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(hip):
    from geoformer_amd.model import GeoFormer, load_config
    from tests.util import synthetic_state_dict

    m = GeoFormer(load_config("test_geoformer_scannet.yaml"))
    m.load_state_dict(synthetic_state_dict(m.state_dict(), 0))
    m.cuda()
    m.eval()
    return m


KW = dict(reserve=False, final_score_thresh=0.0)


class _Capture:
    """Stands where the loops take a SemanticEvaluator: keeps a copy of every scene's scores by name."""

    def __init__(self):
        self.scores = {}

    def add_batch(self, scores, labels, offsets, names, offsets_host=None):
        from geoformer_amd import pointops

        off = offsets_host.tolist()
        for i, n in enumerate(names):
            self.scores[n] = scores[off[i]:off[i + 1]].clone()
        return pointops.semantic_confusion(scores.contiguous(), None, None, None)


@pytest.fixture(scope="module")
def case():
    from geoformer_amd import batch_eval

    items = [("room", scan(1)), ("scan", scan(4))]
    tiling = batch_eval.Tiling(tile=3.5, halo=0.3, max_points=10000, min_shared=10)
    expanded, plans = batch_eval.tile_items(items, tiling)
    plan = plans["scan"]
    assert plan.T == 2 and [n for n, _ in expanded] == ["room", ("scan", 0), ("scan", 1)]
    assert (plan.tile_of[:, 1] >= 0).sum() > 500
    return dict(items=items, tiling=tiling, expanded=expanded, plan=plan, ref={})


def _predict(model, items, batch_size, **kw):
    from geoformer_amd import batch_eval

    np.random.seed(21)
    out = list(batch_eval.predict_batches(model, items, batch_size, **KW, **kw))
    torch.cuda.synchronize()
    return out


def _same(a, b):
    return all(torch.is_tensor(x) == torch.is_tensor(y) and (not torch.is_tensor(x) or torch.equal(x, y))
               for x, y in zip(a[1:], b[1:])) and a[0] == b[0]


def _reference(model, case, batch_size):
    """The reference leg: the untiled loop over the expanded list with the capturing object; per scene name the host
    copies of the captured scores (computed once per batch size)."""
    if batch_size not in case["ref"]:
        cap = _Capture()
        _predict(model, case["expanded"], batch_size, semantic=cap)
        case["ref"][batch_size] = {n: s.cpu().numpy() for n, s in cap.scores.items()}
    return case["ref"][batch_size]


def _stitched(case, ref, mode):
    from geoformer_amd import postprocess

    return postprocess.stitch_tiles_host(case["plan"], [ref[("scan", s)] for s in range(case["plan"].T)], mode)


@pytest.mark.parametrize("batch_size", [2, 1])
def test_predict_batches_stitch_counts_the_scan_once(model, case, batch_size):
    """batch_size 1: the scan's two tiles come out of different forwards (the kept scores must not alias the forward's
    buffers)."""
    from geoformer_amd import evaluation

    ref = _reference(model, case, batch_size)
    raws = dict(case["items"])
    base = _predict(model, case["items"], batch_size, tiles=case["tiling"])
    assert [r[0] for r in base] == ["room", "scan"]
    differ = int((evaluation.semantic_preds_host(_stitched(case, ref, "core"))
                  != evaluation.semantic_preds_host(_stitched(case, ref, "mean"))).sum())
    print(f"batch_size {batch_size}: core and mean differ in the class of {differ} of the scan's points")
    for mode in MODES:
        ev = evaluation.SemanticEvaluator(n_classes=model.cfg.classes, train_fold=model.cfg.train_fold)
        tiled = _predict(model, case["items"], batch_size, tiles=case["tiling"], stitch=mode, semantic=ev)
        assert sorted(ev.names) == ["room", "scan"]
        confs = ev.scene_confusions()
        want = {"scan": _stitched(case, ref, mode), "room": ref["room"]}
        for name in ("scan", "room"):
            _, conf = evaluation.semantic_confusion_host(want[name], raws[name][:, 6].astype(np.int64), lut=ev.lut,
                                                         **ev._map_kw())
            assert confs[name].shape == conf[0].shape and np.array_equal(confs[name], conf[0]), (mode, name)
            assert conf[0].sum() == raws[name].shape[0]
        assert len(tiled) == 2 and all(_same(a, b) for a, b in zip(base, tiled))  # the instances are untouched


def test_panoptic_loops_accept_stitch(model, case):
    from geoformer_amd import batch_eval
    from geoformer_amd import evaluation as E

    ref = _reference(model, case, 2)
    sem = {"scan": E.semantic_preds_host(_stitched(case, ref, "core")), "room": E.semantic_preds_host(ref["room"])}
    np.random.seed(21)
    got = list(batch_eval.panoptic_batches(model, case["items"], 2, tiles=case["tiling"], stitch="core", min_score=0.0,
                                           **KW))
    torch.cuda.synchronize()
    assert [n for n, *_ in got] == ["room", "scan"]
    ev = E.PanopticEvaluator(model.cfg.cvfold)
    for (name, lab, pan), (_, raw) in zip(got, case["items"]):
        N = raw.shape[0]
        assert isinstance(pan, np.ndarray) and pan.dtype == np.int32 and pan.shape == (N,) and lab.owner.shape == (N,)
        gt = E.gt_ids_from_labels(raw[:, 6].astype(np.int64), raw[:, 7].astype(np.int64))
        want = E.panoptic_overlaps_host(lab.owner, sem[name], gt, class_ids=ev.class_ids, is_stuff=ev.is_stuff,
                                        stuff_of_sem=ev.stuff_of_sem, P=len(lab.table.label_id), ids=lab.ids)[0]
        assert np.array_equal(pan, want), name
    np.random.seed(21)
    res = batch_eval.evaluate_panoptic(model, case["items"], 2, classes=model.cfg.cvfold, tiles=case["tiling"],
                                       stitch="core", min_score=0.0, **KW)
    assert "pq" in res


def test_semantic_batches_stitch(model, case):
    from geoformer_amd import batch_eval
    from geoformer_amd import evaluation as E

    cap = _Capture()
    names = [n for n, _ in batch_eval.semantic_batches(model, case["expanded"], 2, reserve=False, evaluator=cap)]
    assert names == ["room", ("scan", 0), ("scan", 1)]
    ref = {n: s.cpu().numpy() for n, s in cap.scores.items()}
    raws = dict(case["items"])
    for mode in MODES:
        ev = E.SemanticEvaluator(n_classes=model.cfg.classes, train_fold=model.cfg.train_fold)
        got = list(batch_eval.semantic_batches(model, case["items"], 2, reserve=False, evaluator=ev, tiles=case["tiling"],
                                               stitch=mode))
        assert [n for n, _ in got] == ["room", "scan"] and ev.names == ["room", "scan"]
        want = {"room": ref["room"], "scan": _stitched(case, ref, mode)}
        confs = ev.scene_confusions()
        for name, preds in got:
            assert preds.dtype == torch.int32 and preds.shape == (raws[name].shape[0],)
            assert np.array_equal(preds.cpu().numpy(), E.semantic_preds_host(want[name])), (mode, name)
            _, conf = E.semantic_confusion_host(want[name], raws[name][:, 6].astype(np.int64), lut=ev.lut, **ev._map_kw())
            assert np.array_equal(confs[name], conf[0]), (mode, name)
    res = batch_eval.evaluate_semantic(model, case["items"], 2, reserve=False, tiles=case["tiling"], stitch="core")
    assert "miou" in res
