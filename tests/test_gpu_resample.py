"""GPU: csrc/resample.hip against the host statements (postprocess.grid_subsample_host, nearest_point_host), integer
arrays and float bit patterns, every call run twice with identical results, at the shapes where the kernels can go wrong;
their argument checks; and density= end to end through the loops of batch_eval against the same loops over the scenes
subsampled by hand."""
import numpy as np
import pytest
import torch

from tests import resample_cases as rc

pytestmark = pytest.mark.gpu


def _same_ints(got, want):
    return got.is_cuda and got.dtype == torch.int32 and got.shape == want.shape and np.array_equal(got.cpu().numpy(), want)


def _check_sub(x, cell, origin=None, modes=rc.MODES):
    """The kernel against the statement in both modes, each run twice; returns the statement's results by mode."""
    from geoformer_amd import pointops, postprocess

    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    od = None if origin is None else torch.from_numpy(origin).cuda()
    out = {}
    for mode in modes:
        want = postprocess.grid_subsample_host(x, cell, mode, origin)
        runs = [pointops.grid_subsample(xd, cell, mode, od) for _ in range(2)]
        torch.cuda.synchronize()
        for got in runs:
            assert all(_same_ints(g, w) for g, w in zip(got, want)), (mode, cell, x.shape)
        out[mode] = want
    assert np.array_equal(out[modes[0]][1], out[modes[-1]][1])
    return out


@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_subsample_small_sizes(hip, N):
    from geoformer_amd import pointops

    assert pointops.resample_limits() == (1 << 29, 1 << 21, float(1 << 30))
    for cell in rc.CELLS:
        _check_sub(rc.prefix(N), cell)


@pytest.mark.parametrize("scene", sorted(rc.SCENES))
def test_subsample_scenes(hip, scene):
    x = rc.room(*scene)
    for cell in rc.CELLS:
        out = _check_sub(x, cell)
        M, most = rc.SCENES[scene][cell]
        assert out["first"][0].shape[0] == M and out["first"][2].max() == most
    assert not np.array_equal(out["first"][0], out["center"][0])


def test_subsample_contention_carry_and_order(hip):
    x = rc.one_cell()
    out = _check_sub(x, 1.0, np.zeros(3, np.float32))
    assert out["center"][0].shape == (1,) and out["center"][2][0] == x.shape[0]
    x = rc.carry()
    out = _check_sub(x, 0.1)
    assert x.shape[0] > 65536 and (out["first"][0] > 65536).sum() > 100  # cells numbered past the scan's carry
    x = rc.shuffled()
    out = _check_sub(x, 0.25)
    k = rc.keys_of(x, 0.25)[out["first"][0]]
    assert (np.diff(k) < 0).any() and (np.diff(k) > 0).any()  # first-occurrence numbering is not key order


def test_subsample_faces_copies_translation_and_origin(hip):
    x, origin = rc.faces()
    _check_sub(x, 0.125, origin)
    x, where = rc.copies(200)
    for cell in (0.05, 0.25):
        out = _check_sub(x, cell)
        assert not np.isin(out["center"][0], where[1:]).any()  # among equal (d2) the lowest index
    _check_sub(np.repeat(x[where[:1]], 300, 0), 0.1)
    _check_sub(rc.translated(100.0), 0.1)
    x = rc.room(4000, 1)
    _check_sub(x, 0.1, x.min(0) - np.array([0.31, 0.07, 1.5], np.float32))


def test_subsample_invalid_points_raise(hip):
    from geoformer_amd import pointops

    x = rc.prefix(257)
    bad = x.copy()
    bad[200, 2] = np.nan
    for arr, origin in ((bad, None), (bad, x.min(0)), (np.array([[0, 0, 0], [2100, 0, 0]], np.float32), None),
                        (x, x.min(0) + np.float32(0.5))):
        od = None if origin is None else torch.from_numpy(origin).cuda()
        for mode in rc.MODES:
            with pytest.raises(ValueError, match="outside the grid"):
                pointops.grid_subsample(torch.from_numpy(arr).cuda(), 0.001 if arr.shape[0] == 2 else 0.1, mode, od)
    inf = x.copy()
    inf[3, 0] = -np.inf
    with pytest.raises(ValueError, match="outside the grid"):
        pointops.grid_subsample(torch.from_numpy(inf).cuda(), 0.1)
    _check_sub(np.array([[0, 0, 0], [2090, 0, 0]], np.float32), 0.001)  # just inside 2^21 cells


def test_subsample_argument_errors_launch_nothing(hip):
    from geoformer_amd import _lib, pointops

    x = torch.from_numpy(rc.prefix(65)).cuda()
    N = x.shape[0]
    out = torch.full((3, N), 7, dtype=torch.int32, device="cuda")
    words = torch.full((2,), 7, dtype=torch.int32, device="cuda")
    ws = torch.zeros(hip.gf_grid_subsample_scratch_bytes(N) // 8 + 1, dtype=torch.int64, device="cuda")
    st = _lib.stream_ptr()

    def call(xyz=x.data_ptr(), N=N, cell=0.1, mode=1, rep=out[0].data_ptr()):
        return hip.gf_grid_subsample(xyz, N, cell, mode, None, ws.data_ptr(), rep, out[1].data_ptr(), out[2].data_ptr(),
                                     words.data_ptr(), st)

    assert call(N=-1) == -1 and call(cell=0.0) == -1 and call(cell=-1.0) == -1
    assert call(cell=float("inf")) == -1 and call(cell=float("nan")) == -1
    assert call(mode=2) == -1 and call(mode=-1) == -1
    assert call(xyz=None) == -1 and call(rep=None) == -1
    assert call(N=0) == 0 and call(N=0, xyz=None) == 0
    torch.cuda.synchronize()
    assert (out == 7).all() and (words == 7).all() and not ws.any()  # none of them launched, nothing was written
    assert call() == 0
    torch.cuda.synchronize()
    assert words.tolist()[1] == 0 and words.tolist()[0] == pointops.grid_subsample(x, 0.1)[0].shape[0]
    empty = pointops.grid_subsample(x[:0], 0.1)
    assert all(t.shape == (0,) and t.dtype == torch.int32 and t.is_cuda for t in empty)
    with pytest.raises(ValueError, match="contiguous float32"):
        pointops.grid_subsample(x.double(), 0.1)
    with pytest.raises(ValueError, match="origin"):
        pointops.grid_subsample(x, 0.1, origin=torch.zeros(3))  # on the host


# ---- nearest point ---------------------------------------------------------------------------------------------------
def _check_nearest(q, p, max_dist):
    from geoformer_amd import pointops, postprocess

    want = postprocess.nearest_point_host(q, p, max_dist)
    qd, pd = torch.from_numpy(np.ascontiguousarray(q)).cuda(), torch.from_numpy(np.ascontiguousarray(p)).cuda()
    runs = [pointops.nearest_point(qd, pd, max_dist) for _ in range(2)]
    torch.cuda.synchronize()
    for idx, d2 in runs:
        assert _same_ints(idx, want[0]), (q.shape, p.shape, max_dist)
        assert d2.is_cuda and d2.dtype == torch.float32
        assert np.array_equal(d2.cpu().numpy().view(np.int32), want[1].view(np.int32)), (q.shape, p.shape, max_dist)
    return want


@pytest.mark.parametrize("n", rc.NP_SIZES)
def test_nearest_sizes(hip, n):
    p = rc.cloud(n)
    for Q in rc.NP_SIZES:
        idx, _ = _check_nearest(rc.jittered(p, Q, 0.02, seed=Q), p, 0.05)
        assert Q < 63 or 0 < (idx >= 0).sum() < Q  # some jitters leave the radius


def test_nearest_equal_points_duplicates_and_far_queries(hip):
    p = rc.cloud(1000)
    p[500:600] = p[100:200]  # duplicates: the lower index
    idx, d2 = _check_nearest(p, p, 0.03)
    assert (d2 == 0).all() and np.array_equal(idx[500:600], np.arange(100, 200)) and np.array_equal(idx[:500], np.arange(500))
    far = np.concatenate([p[:200] + np.float32(30), p[:200] - np.array([0, 0.2, 0], np.float32), p[:5]])
    idx, d2 = _check_nearest(far, p, 0.03)
    assert (idx[:200] == -1).all() and np.isinf(d2[:200]).all() and (idx[-5:] >= 0).all()
    idx, _ = _check_nearest(p[:10], p[:0], 0.03)  # no points at all
    assert (idx == -1).all()


def test_nearest_lattice_ties_and_faces(hip):
    q, p = rc.lattice_with_holes()
    idx, d2 = _check_nearest(q, p, 0.25)
    assert ((d2 == np.float32(0.0625)) & (idx >= 0)).sum() > 50  # d2 == r2 exactly: the candidate counts
    idx, d2 = _check_nearest(rc.lattice_midpoints(), rc.lattice(), 0.25)
    assert (d2 == np.float32(0.015625)).all()  # equidistant pairs: the index decides
    q, p, partner = rc.straddling(0.05)
    idx, d2 = _check_nearest(q, p, 0.05)
    assert (idx >= 0).all() and (np.sqrt(d2) > 0.05 * 0.998).sum() > len(q) // 2


def test_nearest_non_finite_translated_and_range(hip):
    from geoformer_amd import pointops

    p = rc.cloud(1000)
    q = rc.jittered(p, 300, 0.01)
    q[5, 0], q[6, 1], q[7, 2] = np.nan, np.inf, -np.inf
    bad = p.copy()
    bad[::50, 1] = np.nan
    bad[7, 0] = np.inf
    idx, _ = _check_nearest(q, bad, 0.05)
    assert (idx[5:8] == -1).all() and not np.isin(idx, np.arange(0, 1000, 50)).any() and (idx >= 0).sum() > 200
    idx, _ = _check_nearest(q[:3], np.full((4, 3), np.nan, np.float32), 0.05)  # no valid point
    assert (idx == -1).all()
    _check_nearest(rc.jittered(p, 300, 0.01) + np.float32(100), p + np.float32(100), 0.05)
    # two points 1e6 apart at max_dist 1e-4: 1e10 cells between them, beyond the proven 2^30
    wide = torch.tensor([[0, 0, 0], [1e6, 0, 0]], dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError, match="proven"):
        pointops.nearest_point(wide, wide, 1e-4)
    idx, d2, flag = pointops.nearest_point(wide, wide, 1e-4, check=False, return_flag=True)
    assert flag.dtype == torch.int32 and flag.shape == (1,) and flag.item() == 1
    assert pointops.nearest_point(wide, wide, 1e-2, return_flag=True)[2].item() == 0  # 1e8 cells: inside
    _check_nearest(wide.cpu().numpy(), wide.cpu().numpy(), 1e-2)


def test_nearest_argument_errors_launch_nothing(hip):
    from geoformer_amd import _lib, pointops

    p = torch.from_numpy(rc.cloud(65)).cuda()
    idx = torch.full((65,), 7, dtype=torch.int32, device="cuda")
    d2 = torch.full((65,), 7.0, device="cuda")
    flag = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    ws = torch.zeros(hip.gf_nearest_point_scratch_bytes(65) // 8 + 1, dtype=torch.int64, device="cuda")
    st = _lib.stream_ptr()

    def call(q=p.data_ptr(), Q=65, xyz=p.data_ptr(), n=65, md=0.05, out=idx.data_ptr()):
        return hip.gf_nearest_point(q, Q, xyz, n, md, ws.data_ptr(), out, d2.data_ptr(), flag.data_ptr(), st)

    assert call(Q=-1) == -1 and call(n=-1) == -1 and call(md=0.0) == -1 and call(md=float("nan")) == -1
    assert call(md=float("inf")) == -1 and call(q=None) == -1 and call(xyz=None) == -1 and call(out=None) == -1
    assert call(Q=0) == 0
    torch.cuda.synchronize()
    assert (idx == 7).all() and (d2 == 7.0).all() and flag.item() == 7 and not ws.any()
    assert call() == 0
    torch.cuda.synchronize()
    assert idx.tolist() == list(range(65)) and flag.item() == 0
    got = pointops.nearest_point(p[:0], p, 0.05)
    assert got[0].shape == (0,) and got[1].shape == (0,) and got[0].is_cuda
    with pytest.raises(ValueError, match="expected a tensor on"):
        pointops.nearest_point(p, p.cpu(), 0.05)


@pytest.mark.parametrize("mode", rc.MODES)
def test_every_point_finds_a_representative(hip, mode):
    from geoformer_amd import pointops

    x = torch.from_numpy(rc.room(20000, 3)).cuda()
    for cell in (0.05, 0.25):
        rep, cell_of, _ = pointops.grid_subsample(x, cell, mode)
        idx, d2 = pointops.nearest_point(x, x[rep.long()].contiguous(), 2 * cell)
        assert (idx >= 0).all() and (d2 <= np.float32(2 * cell) ** 2).all()
        assert (d2[rep.long()] == 0).all()


# ---- end to end ------------------------------------------------------------------------------------------------------
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
            self.labels = labels.clone()
        return pointops.semantic_confusion(scores.contiguous(), None, None, None)


def _predict(model, items, batch_size, **kw):
    from geoformer_amd import batch_eval

    np.random.seed(21)
    out = list(batch_eval.predict_batches(model, items, batch_size, **KW, **kw))
    torch.cuda.synchronize()
    return out


def _by_hand(items, cell, mode):
    """(items subsampled by hand through the statement, {name: cell_of})."""
    from geoformer_amd import postprocess

    sub, parents = [], {}
    for name, raw in items:
        rep, cell_of, _ = postprocess.grid_subsample_host(raw[:, :3].astype(np.float32), cell, mode)
        assert rep.shape[0] < raw.shape[0]
        sub.append((name, raw[rep]))
        parents[name] = cell_of
    return sub, parents


def _assert_expanded(got, ref, parents, items):
    raws = dict(items)
    assert [g[0] for g in got] == [r[0] for r in ref] == [n for n, _ in items]
    for (name, cls, sc, masks, pick), (_, rcls, rsc, rmasks, rpick) in zip(got, ref):
        assert torch.is_tensor(masks) == torch.is_tensor(rmasks)
        assert torch.equal(pick, rpick)
        if not torch.is_tensor(masks):
            continue
        assert torch.equal(cls, rcls) and torch.equal(sc.view(torch.int32), rsc.view(torch.int32))
        assert masks.dtype == torch.int32 and masks.shape == (rmasks.shape[0], raws[name].shape[0])
        assert torch.equal(masks.cpu(), rmasks.cpu()[:, torch.from_numpy(parents[name]).long()]), name


@pytest.fixture(scope="module")
def rooms():
    return [("a", np.array(rc.raw_scene(4000, 1))), ("b", np.array(rc.raw_scene(20000, 3)))]


@pytest.mark.parametrize("mode", rc.MODES)
def test_predict_batches_density_equals_the_loop_by_hand(model, rooms, mode):
    from geoformer_amd import batch_eval

    sub, parents = _by_hand(rooms, 0.1, mode)
    ref_cap, cap = _Capture(), _Capture()
    ref = _predict(model, sub, 2, semantic=ref_cap)
    got = _predict(model, rooms, 2, density=batch_eval.Density(cell=0.1, mode=mode), semantic=cap)
    assert any(torch.is_tensor(r[3]) and r[3].shape[0] > 0 for r in ref)
    _assert_expanded(got, ref, parents, rooms)
    for name, raw in rooms:
        want = ref_cap.scores[name].cpu()[torch.from_numpy(parents[name]).long()]
        assert cap.scores[name].shape == (raw.shape[0], want.shape[1])
        assert torch.equal(cap.scores[name].cpu().view(torch.int32), want.view(torch.int32)), name
    assert np.array_equal(cap.labels.cpu().numpy(), rooms[-1][1][:, 6].astype(np.int64))  # the scene's own labels


def test_density_that_keeps_every_point_changes_nothing(model, rooms):
    from geoformer_amd import batch_eval

    items = rooms[:1]
    base = _predict(model, items, 1)
    got = _predict(model, items, 1, density=batch_eval.Density(cell=0.002))
    assert len(got) == len(base) == 1
    for x, y in zip(got[0][1:], base[0][1:]):
        assert torch.is_tensor(x) == torch.is_tensor(y) and (not torch.is_tensor(x) or torch.equal(x, y))
    assert torch.is_tensor(got[0][3]) and got[0][3].shape[1] == items[0][1].shape[0]


def test_density_with_tiles_and_stitch_equals_the_chain_by_hand(model):
    from geoformer_amd import batch_eval
    from tests.tile_stitch_cases import scan

    items = [("scan", scan(4))]
    tiling = batch_eval.Tiling(tile=3.5, halo=0.3, max_points=10000, min_shared=10)  # test_gpu_tile_stitch.py's
    sub, parents = _by_hand(items, 0.05, "center")
    assert batch_eval.tile_items(sub, tiling)[1]["scan"].T == 2  # the subsampled scan still runs as two tiles
    ref_cap, cap = _Capture(), _Capture()
    ref = _predict(model, sub, 2, tiles=tiling, stitch="core", semantic=ref_cap)
    got = _predict(model, items, 2, tiles=tiling, stitch="core", semantic=cap,
                   density=batch_eval.Density(cell=0.05, mode="center"))
    assert torch.is_tensor(ref[0][3]) and ref[0][3].shape[0] > 0
    _assert_expanded(got, ref, parents, items)
    want = ref_cap.scores["scan"].cpu()[torch.from_numpy(parents["scan"]).long()]
    assert list(cap.scores) == ["scan"] and torch.equal(cap.scores["scan"].cpu().view(torch.int32), want.view(torch.int32))


def test_the_other_loops_accept_density(model, rooms):
    from geoformer_amd import batch_eval
    from geoformer_amd import evaluation as E

    dens = batch_eval.Density(cell=0.1)
    sizes = {n: r.shape[0] for n, r in rooms}
    np.random.seed(21)
    labs = list(batch_eval.label_batches(model, rooms, 2, min_score=0.0, density=dens, **KW))
    assert [n for n, _ in labs] == ["a", "b"] and all(lab.owner.shape == (sizes[n],) == lab.ids.shape for n, lab in labs)
    np.random.seed(21)
    ap, avgs = batch_eval.evaluate(model, rooms, 2, density=dens, **KW)
    assert "all_ap" in avgs
    np.random.seed(21)
    pans = list(batch_eval.panoptic_batches(model, rooms, 2, min_score=0.0, density=dens, **KW))
    assert all(pan.shape == (sizes[n],) and lab.owner.shape == (sizes[n],) for n, lab, pan in pans)
    np.random.seed(21)
    assert "pq" in batch_eval.evaluate_panoptic(model, rooms, 2, classes=model.cfg.cvfold, min_score=0.0, density=dens, **KW)
    sub, parents = _by_hand(rooms, 0.1, "center")
    ref = dict((n, p.cpu().numpy()) for n, p in batch_eval.semantic_batches(model, sub, 2, reserve=False))
    ev = E.SemanticEvaluator(n_classes=model.cfg.classes, train_fold=model.cfg.train_fold)
    got = [(n, p.cpu().numpy()) for n, p in batch_eval.semantic_batches(model, rooms, 2, reserve=False, evaluator=ev,
                                                                        density=dens)]
    assert [n for n, _ in got] == ["a", "b"] and ev.names == ["a", "b"]
    for name, preds in got:
        assert preds.dtype == np.int32 and preds.shape == (sizes[name],)
        assert np.array_equal(preds, ref[name][parents[name]]), name
    assert sum(int(c.sum()) for c in ev.scene_confusions().values()) <= sum(sizes.values())
    assert "miou" in batch_eval.evaluate_semantic(model, rooms, 2, reserve=False, density=dens)
    with pytest.raises(ValueError, match="share their name|are named"):
        list(batch_eval.predict_batches(model, [rooms[0], rooms[0]], 2, density=dens, **KW))
