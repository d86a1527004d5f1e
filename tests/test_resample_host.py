"""CPU: the statements of the grid subsample and the nearest point (postprocess.grid_subsample_host,
nearest_point_host) against independent formulations, their invariants, the figures that prove the shared cases reach the
regimes they are named for, and the Python plumbing of density= (Density, density_items, expand_*, transfer) on CPU
tensors."""
import importlib.util
import os
from ctypes import c_double, c_float, c_int, c_size_t, c_void_p

import numpy as np
import pytest
import torch

from tests import resample_cases as rc

P, I = c_void_p, c_int


def _sub(x, cell, mode, origin=None):
    from geoformer_amd import postprocess

    return postprocess.grid_subsample_host(x, cell, mode, origin)


def _invariants(x, rep, cell_of, count, mode):
    N, M = x.shape[0], rep.shape[0]
    assert rep.dtype == cell_of.dtype == count.dtype == np.int32
    assert cell_of.shape == (N,) and count.shape == (M,) and int(count.sum()) == N
    assert np.array_equal(cell_of[rep], np.arange(M)) and np.array_equal(np.bincount(cell_of, minlength=M), count)
    if mode == "first":
        assert (np.diff(rep) > 0).all()


@pytest.mark.parametrize("scene", sorted(rc.SCENES))
def test_statement_equals_unique_formulation_and_the_table(scene):
    x = rc.room(*scene)
    assert x.shape == (rc.SCENE_POINTS[scene], 3)
    for cell, (M, most) in rc.SCENES[scene].items():
        first, cell_of, count = rc.unique_formulation(x, cell)
        for mode in rc.MODES:
            rep, co, cnt = _sub(x, cell, mode)
            _invariants(x, rep, co, cnt, mode)
            assert np.array_equal(co, cell_of) and np.array_equal(cnt, count)  # the numbering does not depend on the mode
            if mode == "first":
                assert np.array_equal(rep, first)
        assert (rep.shape[0], int(count.max())) == (M, most), (scene, cell)


@pytest.mark.parametrize("case", ["prefix257", "copies", "faces", "shuffled"])
def test_center_mode_equals_a_scalar_loop(case):
    origin = None
    if case == "prefix257":
        x, cell = rc.prefix(257), 0.25
    elif case == "copies":
        x, cell = rc.copies()[0], 0.25
    elif case == "faces":
        (x, origin), cell = rc.faces(), 0.125
    else:
        x, cell = rc.shuffled()[:1500], 0.25
    rep, cell_of, count = _sub(x, cell, "center", origin)
    _invariants(x, rep, cell_of, count, "center")
    assert count.max() > 1
    assert np.array_equal(rep, rc.center_loop(x, cell, cell_of, rep.shape[0], origin))


def test_ties_go_to_the_lowest_index():
    x, where = rc.copies(200)
    assert where.shape[0] == 201
    for cell in (0.05, 0.25):
        rep, cell_of, count = _sub(x, cell, "center")
        m = cell_of[where[0]]
        assert (cell_of[where] == m).all() and count[m] >= 201
        # were a copy the representative, it is the first of the copies; no other copy ever is
        assert not np.isin(rep, where[1:]).any()
    # a cell of copies alone: 201 equal (d2), the lowest index wins
    only = np.repeat(x[where[:1]], 50, 0)
    rep, _, count = _sub(np.concatenate([x[:10], only]), 0.001, "center", origin=x.min(0))
    assert count.max() == 50 + int((x[:10] == only[0]).all(1).sum()) and np.isin(rep, np.arange(10, 60)).sum() <= 1
    assert int(rep[np.isin(rep, np.arange(10, 60))].min(initial=10)) == 10


def test_the_cases_reach_their_regimes():
    x = rc.one_cell()
    rep, cell_of, count = _sub(x, 1.0, "center", np.zeros(3, np.float32))
    assert rep.shape == (1,) and count[0] == x.shape[0]
    x = rc.carry()
    rep, *_ = _sub(x, 0.1, "first")
    assert x.shape[0] > 65536 and np.searchsorted(rep, 65536) < rep.shape[0] - 100  # cells open past the 256th block sum
    x = rc.shuffled()
    rep, *_ = _sub(x, 0.25, "first")
    k = rc.keys_of(x, 0.25)[rep]
    assert (np.diff(k) < 0).any() and (np.diff(k) > 0).any()  # first occurrence is not key order
    x, origin = rc.faces()
    rep, cell_of, count = _sub(x, 0.125, "center", origin)
    assert rep.shape[0] <= 12 ** 3 and count.max() > 1
    x = rc.translated()
    a, b = _sub(x, 0.1, "center"), _sub(rc.room(4000, 1), 0.1, "center")
    assert a[0].shape[0] > 3000 and abs(a[0].shape[0] - b[0].shape[0]) < 200  # (the grid moved by a rounding, no more)


def test_invalid_points_and_arguments():
    x = rc.prefix(65)
    bad = x.copy()
    bad[40, 1] = np.nan
    with pytest.raises(ValueError, match="outside the grid"):  # (the default origin, xyz.min(0), is NaN with it)
        _sub(bad, 0.1, "first")
    with pytest.raises(ValueError, match="1 point.*point 40"):
        _sub(bad, 0.1, "first", origin=x.min(0))
    bad[40, 1] = np.inf
    with pytest.raises(ValueError, match="outside the grid"):
        _sub(bad, 0.1, "center")
    with pytest.raises(ValueError, match="outside the grid"):  # more than 2^21 cells along x
        _sub(np.array([[0, 0, 0], [2100, 0, 0]], np.float32), 0.001, "first")
    assert _sub(np.array([[0, 0, 0], [2090, 0, 0]], np.float32), 0.001, "first")[0].shape == (2,)
    with pytest.raises(ValueError, match="outside the grid"):  # below the caller's origin
        _sub(x, 0.1, "first", origin=x.min(0) + np.float32(0.5))
    for cell in (0.0, -1.0, np.inf, np.nan, 1e-50):
        with pytest.raises(ValueError, match="cell"):
            _sub(x, cell, "first")
    with pytest.raises(ValueError, match="mode"):
        _sub(x, 0.1, "mean")
    with pytest.raises(ValueError, match=r"\[n, 3\]"):
        _sub(x[:, :2], 0.1, "first")
    for mode in rc.MODES:
        out = _sub(np.zeros((0, 3), np.float32), 0.1, mode)
        assert all(a.shape == (0,) and a.dtype == np.int32 for a in out)


# ---- nearest point ---------------------------------------------------------------------------------------------------
def _nearest_loop(q, p, max_dist):
    r2 = np.float32(max_dist) * np.float32(max_dist)
    idx, out = np.full(len(q), -1, np.int32), np.full(len(q), np.inf, np.float32)
    with np.errstate(all="ignore"):
        for a in range(len(q)):
            if not np.isfinite(q[a]).all():
                continue
            for b in range(len(p)):
                d = q[a] - p[b]
                d2 = np.float32(np.float32(d[0] * d[0]) + np.float32(d[1] * d[1])) + np.float32(d[2] * d[2])
                if np.isfinite(p[b]).all() and d2 <= r2 and d2 < out[a]:
                    idx[a], out[a] = b, d2
    return idx, out


def test_nearest_statement_equals_a_scalar_loop():
    from geoformer_amd import postprocess

    p = rc.cloud(300)
    p[7] = p[3]  # a duplicate: the lower index wins
    p[11, 2] = np.nan
    q = np.concatenate([p[:40], rc.jittered(p, 80, 0.03), p[:3] + np.float32(50)])
    q[5, 0] = np.inf
    for max_dist in (0.02, 0.08):
        idx, d2 = postprocess.nearest_point_host(q, p, max_dist, chunk_elems=7 * 300)  # several chunks
        want = _nearest_loop(q, p, max_dist)
        assert idx.dtype == np.int32 and d2.dtype == np.float32
        assert np.array_equal(idx, want[0]) and np.array_equal(d2.view(np.int32), want[1].view(np.int32))
        assert idx[7] == 3 and d2[7] == 0 and idx[5] == -1 and idx[11] == -1 and (idx[-3:] == -1).all()
        assert np.isinf(d2[idx < 0]).all() and 10 < (idx >= 0).sum() < len(q)
    assert postprocess.nearest_point_host(q[:0], p, 0.1)[0].shape == (0,)
    idx, d2 = postprocess.nearest_point_host(q, p[:0], 0.1)
    assert (idx == -1).all() and np.isinf(d2).all()
    for md in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="max_dist"):
            postprocess.nearest_point_host(q, p, md)


def test_nearest_cases_reach_their_regimes():
    from geoformer_amd import postprocess

    q, p = rc.lattice_with_holes()
    idx, d2 = postprocess.nearest_point_host(q, p, 0.25)
    at_radius = d2 == np.float32(0.0625)
    assert at_radius.sum() > 50 and (idx[at_radius] >= 0).all()  # d2 == r2 exactly, and the candidate counts
    assert postprocess.nearest_point_host(q, p, np.nextafter(np.float32(0.25), np.float32(0)))[0][at_radius].max() == -1
    x = rc.lattice()
    idx, d2 = postprocess.nearest_point_host(rc.lattice_midpoints(), x, 0.25)
    assert (d2 == np.float32(0.015625)).all()
    assert np.array_equal(x[idx] + np.array([0.125, 0, 0], np.float32), rc.lattice_midpoints())  # the lower of the two
    q, p, partner = rc.straddling(0.05)
    cell = 0.05 * 1.001
    assert (np.floor(q / cell) != np.floor(p[partner] / cell)).any(1).all()  # on both sides of a face
    idx, d2 = postprocess.nearest_point_host(q, p, 0.05)
    assert (idx >= 0).all() and (np.sqrt(d2) > 0.05 * 0.998).sum() > len(q) // 2


# ---- the Python plumbing on CPU tensors ------------------------------------------------------------------------------
def test_wrappers_run_the_statements_on_cpu_tensors_and_check_their_arguments():
    from geoformer_amd import pointops, postprocess

    x = torch.from_numpy(rc.room(4000, 1))
    for mode in rc.MODES:
        got = pointops.grid_subsample(x, 0.25, mode)
        want = postprocess.grid_subsample_host(x.numpy(), 0.25, mode)
        assert all(g.dtype == torch.int32 and np.array_equal(g.numpy(), w) for g, w in zip(got, want))
    origin = x.min(0).values - 0.5
    assert np.array_equal(pointops.grid_subsample(x, 0.25, "first", origin)[1].numpy(),
                          postprocess.grid_subsample_host(x.numpy(), 0.25, "first", origin.numpy())[1])
    idx, d2 = pointops.nearest_point(x[:100] + 0.001, x, 0.05)
    want = postprocess.nearest_point_host(x[:100].numpy() + np.float32(0.001), x.numpy(), 0.05)
    assert np.array_equal(idx.numpy(), want[0]) and np.array_equal(d2.numpy().view(np.int32), want[1].view(np.int32))
    assert pointops.nearest_point(x[:5], x, 0.05, return_flag=True)[2] is None
    for bad in (x.double(), x[:, :2], x.t().contiguous().t(), x.numpy()):
        with pytest.raises(ValueError, match="contiguous float32"):
            pointops.grid_subsample(bad, 0.1)
        with pytest.raises(ValueError, match="contiguous float32"):
            pointops.nearest_point(x, bad, 0.1)
    with pytest.raises(ValueError, match="origin"):
        pointops.grid_subsample(x, 0.1, origin=origin.double())
    with pytest.raises(ValueError, match="mode"):
        pointops.grid_subsample(x, 0.1, mode="mean")
    with pytest.raises(ValueError, match="cell"):
        pointops.grid_subsample(x, 0.0)
    with pytest.raises(ValueError, match="max_dist"):
        pointops.nearest_point(x, x, 0.0)


def test_expand_and_transfer():
    from geoformer_amd import postprocess

    x = torch.from_numpy(rc.room(4000, 1))
    rep, cell_of, _ = (torch.from_numpy(a) for a in postprocess.grid_subsample_host(x.numpy(), 0.25, "center"))
    n, N = rep.shape[0], x.shape[0]
    rows = torch.arange(n * 3, dtype=torch.float32).reshape(n, 3)
    out = postprocess.expand_rows(rows, cell_of)
    assert out.shape == (N, 3) and torch.equal(out, rows[cell_of.long()]) and torch.equal(out[rep.long()], rows)
    masks = (torch.rand(5, n) > 0.5).int()
    big = postprocess.expand_masks(masks, cell_of)
    assert big.dtype == torch.int32 and big.shape == (5, N) and torch.equal(big[:, rep.long()], masks)
    parent = cell_of.clone()
    parent[::7] = -1
    assert (postprocess.expand_masks(masks, parent)[:, ::7] == 0).all()
    lab = postprocess.expand_rows(torch.arange(n), parent, fill=-100)
    assert lab.shape == (N,) and (lab[::7] == -100).all() and torch.equal(lab[1::7], cell_of[1::7].long())
    assert postprocess.expand_rows(rows[:0], torch.full((4,), -1, dtype=torch.int32), fill=2.0).tolist() == [[2.0] * 3] * 4
    with pytest.raises(ValueError, match="rows"):
        postprocess.expand_rows(rows[:10], cell_of)
    with pytest.raises(ValueError, match="parent"):
        postprocess.expand_masks(masks, cell_of.float())
    # every point finds its own cell's representative again, or a nearer one
    vals, idx = postprocess.transfer(torch.arange(n), x[rep.long()], x, 2 * 0.25, fill=-1)
    assert (idx >= 0).all() and torch.equal(vals, idx.long())
    far, idx = postprocess.transfer(rows, x[rep.long()], x[:10] + 100.0, 0.5, fill=-7.0)
    assert (idx == -1).all() and (far == -7.0).all()


def test_density_validation():
    from geoformer_amd.batch_eval import Density, _density

    assert Density().params == dict(cell=None, mode="center") and Density().cell() == 0.02 and Density().cell(20) == 0.05
    assert Density(cell=0.1, mode="first").cell() == 0.1 and "cell=0.1" in repr(Density(cell=0.1))
    with pytest.raises(TypeError, match="unknown parameter"):
        Density(size=0.1)
    for cell in (0, -0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="cell > 0"):
            Density(cell=cell)
    with pytest.raises(ValueError, match="mode"):
        Density(mode="mean")
    with pytest.raises(ValueError, match="density"):
        _density(0.02)


def test_density_items_on_the_cpu():
    from geoformer_amd import batch_eval, postprocess

    a, b = rc.raw_scene(4000, 1), rc.raw_scene(20000, 3)
    items = [("a", a), ("b", torch.from_numpy(b.copy()))]
    for mode in rc.MODES:
        sub, maps = batch_eval.density_items(items, batch_eval.Density(cell=0.1, mode=mode), "cpu")
        assert [n for n, _ in sub] == ["a", "b"] and sorted(maps) == ["a", "b"]
        for (name, small), raw in zip(sub, (a, b)):
            rep, cell_of, _ = postprocess.grid_subsample_host(raw[:, :3].astype(np.float32), 0.1, mode)
            assert np.array_equal(maps[name].rep, rep) and np.array_equal(maps[name].cell_of.numpy(), cell_of)
            assert np.array_equal(small, raw[rep])  # every column through one gather
    # a scene that keeps every point passes through, the object itself, with no map
    sub, maps = batch_eval.density_items(items, batch_eval.Density(cell=0.002), "cpu")
    assert not maps and sub[0][1] is a and sub[1][1] is items[1][1]
    sub, maps = batch_eval.density_items(items, batch_eval.Density(), "cpu")
    assert sub[0][1].shape[0] < a.shape[0] or not maps  # the default cell: 0.02
    with pytest.raises(ValueError, match="named 'a'|share their name"):
        batch_eval.density_items([("a", a), ("a", b)], batch_eval.Density(cell=0.1), "cpu")
    seg = batch_eval._density_segments({"a": np.arange(a.shape[0])}, batch_eval.density_items(
        items[:1], batch_eval.Density(cell=0.1), "cpu")[1])
    assert np.array_equal(seg["a"], postprocess.grid_subsample_host(a[:, :3].astype(np.float32), 0.1, "center")[0])


def test_density_semantics_hands_on_full_scenes():
    from geoformer_amd import batch_eval

    a = rc.raw_scene(4000, 1)
    b = a[:50].copy()
    b[:, :3] *= 100  # every point a cell of its own: passes through
    sub, maps = batch_eval.density_items([("a", a), ("b", b)], batch_eval.Density(cell=0.25), "cpu")
    assert sorted(maps) == ["a"]
    n = sub[0][1].shape[0]
    got = []

    class Inner:
        def add_batch(self, scores, labels, offsets, names, offsets_host=None):
            got.append((scores, labels, offsets_host.tolist(), names))

    scores = torch.rand(n + sub[1][1].shape[0], 4)
    labels = torch.zeros(scores.shape[0], dtype=torch.int64)
    off = torch.tensor([0, n, scores.shape[0]], dtype=torch.int32)
    batch_eval._DensitySemantics(Inner(), maps, {"a": a}).add_batch(scores, labels, off, ["a", "b"], offsets_host=off)
    assert [g[3] for g in got] == [["a"], ["b"]] and got[0][2] == [0, a.shape[0]]
    assert torch.equal(got[0][0], scores[:n][maps["a"].cell_of.long()])
    assert np.array_equal(got[0][1].numpy(), a[:, 6].astype(np.int64))
    assert torch.equal(got[1][0], scores[n:]) and got[1][2] == [0, 50]


def test_cli_flags():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "predict_scenes.py")
    spec = importlib.util.spec_from_file_location("predict_scenes_cli_density", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ap = mod.build_parser()
    args = ap.parse_args(["--density", "0.02", "--density-mode", "first", "x.npy"])
    assert args.density == 0.02 and args.density_mode == "first"
    assert ap.parse_args(["x.npy"]).density is None
    with pytest.raises(SystemExit):
        ap.parse_args(["--density-mode", "mean", "x.npy"])


def test_header_declares_the_entry_points():
    from geoformer_amd import _abi

    f = _abi.functions()
    assert f["gf_grid_subsample"] == (I, [P, I, c_float, I, P, P, P, P, P, P, P])
    assert f["gf_nearest_point"] == (I, [P, I, P, I, c_float, P, P, P, P, P])
    assert f["gf_grid_subsample_scratch_bytes"] == (c_size_t, [I]) and f["gf_nearest_point_scratch_bytes"] == (c_size_t, [I])
    assert f["gf_resample_max_points"] == (I, []) and f["gf_nearest_point_max_cells"] == (c_double, [])
