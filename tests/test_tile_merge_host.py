"""CPU: the tile plan of a large scan (scene.tile_plan) and the rule that joins the instances of its tiles
(postprocess.merge_tiles_host) against a brute-force restatement from set operations."""
import numpy as np
import pytest

from tests.tile_merge_cases import brute_merge, chain_case, hand_cases, random_case, wall_case


def _plan(xy, tile=4.0, halo=0.5):
    from geoformer_amd import scene

    xy = np.asarray(xy, np.float64)
    return scene.tile_plan(np.concatenate([xy, np.zeros((xy.shape[0], 1))], 1), tile, halo)


def _tiles(plan, g):
    return [int(t) for t in plan.tile_of[g] if t >= 0]


def _check_consistent(plan):
    N, T = plan.N, plan.T
    assert plan.tile_of.shape == plan.local_of.shape == (N, 4) and plan.tile_of.dtype == plan.local_of.dtype == np.int32
    assert plan.core_of.shape == (N,) and plan.core_of.dtype == np.int32
    assert plan.offsets.shape == (T + 1,) and plan.offsets.dtype == plan.index.dtype == np.int64
    assert plan.offsets[0] == 0 and plan.index.shape == (plan.offsets[-1],) and (np.diff(plan.offsets) >= 0).all()
    valid = plan.tile_of >= 0
    assert int(valid.sum()) == plan.index.size and valid[:, 0].all()
    for g in range(N):
        t = plan.tile_of[g][valid[g]]
        assert (np.diff(t) > 0).all() and (plan.tile_of[g][~valid[g]] == -1).all() and t.max() < T
        assert not valid[g, 1:][~valid[g, :-1]].any()  # -1 only behind the tiles
        assert plan.core_of[g] in t
        for k in range(t.size):
            assert plan.points(t[k])[plan.local_of[g, k]] == g
    for s in range(T):
        assert (np.diff(plan.points(s)) > 0).all()


def test_plan_borders_and_halo():
    # 8 x 8 m, tiles of 4 m: the core border of both axes at 4.0
    xy = [[0, 0], [8, 8],
          [4.0, 1.0],    # on the core border: core of column 1, and 0 m from it: also column 0
          [3.5, 1.0],    # exactly halo below the border: (ix + 1) * tx - u <= halo holds
          [4.5, 1.0],    # exactly halo above: u - ix * tx < halo does not
          [3.4999, 1.0], [4.4999, 1.0],
          [4.2, 3.9],    # a corner point: 4 tiles
          [1.0, 1.0]]
    p = _plan(xy)
    assert (p.nx, p.ny, p.T) == (2, 2, 4) and p.size == (4.0, 4.0)
    assert _tiles(p, 2) == [0, 1] and p.core_of[2] == 1
    assert _tiles(p, 3) == [0, 1] and p.core_of[3] == 0
    assert _tiles(p, 4) == [1] and p.core_of[4] == 1
    assert _tiles(p, 5) == [0] and _tiles(p, 6) == [0, 1]
    assert _tiles(p, 7) == [0, 1, 2, 3] and p.core_of[7] == 1
    assert _tiles(p, 8) == [0]
    # the closed upper edge of the last tile: the far corner's core is the last tile, not a tile behind it
    assert p.core_of[1] == 3 and _tiles(p, 1) == [3] and _tiles(p, 0) == [0]
    _check_consistent(p)


def test_plan_equalised_widths_and_ids():
    p = _plan([[0, 0], [9, 5], [4.4, 2.4], [4.6, 2.6], [8.9, 4.9]], tile=4.0, halo=0.25)
    assert (p.nx, p.ny) == (3, 2) and p.size == (3.0, 2.5)  # no sliver: 9 m is three tiles of 3 m
    assert p.core_of.tolist() == [0, 5, 1, 4, 5]  # id = iy * nx + ix
    assert _tiles(p, 2) == [1, 4] and _tiles(p, 3) == [1, 4]
    _check_consistent(p)


def test_plan_single_tile_and_zero_halo():
    rng = np.random.default_rng(0)
    xy = rng.uniform(0, 3, (500, 2))
    p = _plan(xy, tile=4.0, halo=0.5)
    assert (p.nx, p.ny, p.T) == (1, 1, 1)
    assert (p.tile_of[:, 0] == 0).all() and (p.tile_of[:, 1:] == -1).all()
    assert (p.local_of[:, 0] == np.arange(500)).all() and (p.index == np.arange(500)).all()
    xy = np.concatenate([[[0, 0], [9, 9], [3.0, 3.0], [6.0, 3.0]], rng.uniform(0, 9, (2000, 2))])
    p = _plan(xy, tile=3.0, halo=0.0)
    assert p.T == 9 and (p.tile_of[:, 1] == -1).all()  # no point in two tiles, border points included
    assert (p.tile_of[:, 0] == p.core_of).all() and p.offsets[-1] == xy.shape[0]
    _check_consistent(p)


def test_plan_random_consistent_and_halo_too_large():
    rng = np.random.default_rng(1)
    xy = np.concatenate([[[0, 0], [12, 12]], rng.uniform(0, 12, (3000, 2))])
    p = _plan(xy, tile=4.0, halo=2.0)  # the largest halo allowed: half a tile
    assert p.T == 9 and (p.tile_of >= 0).sum(1).max() == 4
    _check_consistent(p)
    # membership restated per tile from its extended box
    u = xy
    for s in range(p.T):
        ix, iy = s % 3, s // 3
        core = p.core_of
        want = np.zeros(xy.shape[0], bool)
        for g in range(xy.shape[0]):
            cx, cy = core[g] % 3, core[g] // 3
            okx = cx == ix or (cx == ix + 1 and u[g, 0] - cx * 4.0 < 2.0) or (cx == ix - 1 and (cx + 1) * 4.0 - u[g, 0] <= 2.0)
            oky = cy == iy or (cy == iy + 1 and u[g, 1] - cy * 4.0 < 2.0) or (cy == iy - 1 and (cy + 1) * 4.0 - u[g, 1] <= 2.0)
            want[g] = okx and oky
        assert np.array_equal(np.nonzero(want)[0], p.points(s))
    with pytest.raises(ValueError, match="halo"):
        _plan(xy, tile=4.0, halo=2.01)
    with pytest.raises(ValueError):
        _plan(xy, tile=0.0)
    with pytest.raises(ValueError):
        _plan(xy, halo=-0.1)
    e = _plan(np.zeros((0, 2)))
    assert e.T == 1 and e.N == 0 and e.offsets.tolist() == [0, 0]


def _check_against_brute(case):
    from geoformer_amd import postprocess

    plan, per_tile, kw = case["plan"], case["per_tile"], case["kw"]
    got = postprocess.merge_tiles_host(plan, per_tile, return_tables=True, **kw)
    want, tables = brute_merge(plan, per_tile, **kw)
    names = ("cls", "scores", "masks", "pick", "members")
    for name, g, w in zip(names, got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w), name
    for name in ("inter", "shared", "count"):
        assert got[5][name].dtype == np.int32 and np.array_equal(got[5][name], tables[name]), name
    assert np.array_equal(got[5]["inter"], got[5]["inter"].T)
    # comp: the smallest row of every component
    assert got[5]["comp"].tolist() == [g[0] for r in range(len(got[4])) for g in tables["groups"] if r in g]
    if "groups" in case:
        assert tables["groups"] == case["groups"]
    assert len(postprocess.merge_tiles_host(plan, per_tile, **kw)) == 5
    return got, tables


@pytest.mark.parametrize("name", sorted(hand_cases()))
def test_merge_hand_cases(name):
    case = hand_cases()[name]
    got, tables = _check_against_brute(case)
    cls, scores, masks, pick, members = got[:5]
    if name == "single_tile":
        # the picked rows in row order with their classes, scores and masks[pick]; pick is the stable score order
        c, s, m, p = case["per_tile"][0]
        assert np.array_equal(cls, c[p]) and np.array_equal(scores, s[p]) and np.array_equal(masks, (m[p] != 0).astype(np.int32))
        assert members.tolist() == [0, 1, 2, 3] and pick.tolist() == [1, 2, 0, 3]  # 0.9 twice: the first one first
    if name == "across_border":
        assert scores.tolist() == [np.float32(0.6), np.float32(0.8)] and pick.tolist() == [1, 0]
    if name == "truncated_part":
        part, whole = case["part"], case["whole"]
        assert part.size / whole.size < 0.5  # IoU of the two rows: below the threshold this rule applies to IoM
        assert tables["inter"][0, 1] == part.size == tables["shared"][0, 1] == tables["shared"][1, 0]
        assert masks.shape[0] == 1 and np.array_equal(np.nonzero(masks[0])[0], whole)
    if name.startswith("ratio"):
        assert tables["inter"][0, 1] == case["inter"]
        assert min(tables["shared"][0, 1], tables["shared"][1, 0]) == case["small"]
    if name.startswith("min_shared"):
        assert tables["inter"][0, 1] == int(name.rsplit("_", 1)[1])
    if name == "empty_tile":
        assert case["plan"].offsets[2] == case["plan"].offsets[1]  # tile 1 holds no point


def test_merge_random_wall_and_chain():
    _check_against_brute(random_case(3, 4000, (9.0, 9.0), 3.0, 0.4, [3, 0, 5, 1, 2]))
    got, _ = _check_against_brute(wall_case(3000))
    assert got[5]["inter"][0, 1] >= 3000
    got, _ = _check_against_brute(chain_case(links=12))
    assert got[0].shape == (1,) and (got[4] == 0).all()


def test_merge_accepts_tensors_and_checks_shapes():
    import torch

    from geoformer_amd import postprocess

    case = hand_cases()["across_border"]
    want = postprocess.merge_tiles_host(case["plan"], case["per_tile"], **case["kw"])
    as_t = [tuple(torch.from_numpy(x) for x in t) if len(t[3]) else ([], [], [], torch.zeros(0, dtype=torch.int64))
            for t in case["per_tile"]]
    got = postprocess.merge_tiles(case["plan"], as_t, **case["kw"])
    assert all(torch.is_tensor(g) and np.array_equal(g.numpy(), w) for g, w in zip(got, want))
    with pytest.raises(ValueError):
        postprocess.merge_tiles_host(case["plan"], case["per_tile"][:1])
    bad = list(case["per_tile"])
    bad[0] = (bad[0][0], bad[0][1], bad[0][2][:, :-1], bad[0][3])
    with pytest.raises(ValueError):
        postprocess.merge_tiles_host(case["plan"], bad)


def test_command_line_flags_and_derived_binding():
    import importlib.util
    import os
    from ctypes import c_double, c_int, c_longlong, c_void_p

    from geoformer_amd import _abi

    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "predict_scenes.py")
    spec = importlib.util.spec_from_file_location("predict_scenes_cli_tiles", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ap = mod.build_parser()
    a = ap.parse_args(["--synthetic", "1"])
    assert a.tile is None and a.halo is None and a.tile_max_points is None
    a = ap.parse_args(["--tile", "4", "--halo", "0.25", "--tile-max-points", "100000", "a.npy"])
    assert (a.tile, a.halo, a.tile_max_points) == (4.0, 0.25, 100000)
    fns = _abi.functions()
    assert fns["gf_tile_merge_max_rows"] == (c_int, []) and fns["gf_tile_merge_max_picks"] == (c_int, [])
    assert fns["gf_tile_pack_picks"] == (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p])
    assert fns["gf_tile_overlaps"] == (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_longlong, c_void_p, c_int,
                                               c_void_p, c_void_p, c_void_p])
    assert fns["gf_tile_merge"] == (c_int, [c_void_p] * 5 + [c_int, c_int, c_double, c_int] + [c_void_p] * 6)
    assert fns["gf_tile_assemble"] == (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_longlong, c_void_p,
                                               c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p])
    assert _abi.const("GF_TILE_SCENE_FIELDS") == 7


def test_tiling_and_tile_items():
    from geoformer_amd import batch_eval, scene

    with pytest.raises(TypeError, match="unknown"):
        batch_eval.Tiling(tiel=3.0)
    t = batch_eval.Tiling()
    assert t.params == dict(tile=4.0, halo=0.5, max_points=400_000, iom=0.5, min_shared=20)
    raw = np.zeros((1000, 8))
    raw[:, :3] = np.random.default_rng(0).uniform(0, 8, (1000, 3))
    items = [("small", raw[:100]), ("big", raw)]
    same, plans = batch_eval.tile_items(items, t)
    assert plans == {} and [n for n, _ in same] == ["small", "big"] and same[1][1] is raw
    out, plans = batch_eval.tile_items(items, batch_eval.Tiling(max_points=500))
    plan = plans["big"]
    assert list(plans) == ["big"] and plan.T == 4 and out[0][0] == "small"
    assert [n for n, _ in out[1:]] == [("big", s) for s in range(4)]
    for (_, s), r in out[1:]:
        assert np.array_equal(r, raw[plan.points(s)])
    assert np.array_equal(plan.tile_of, scene.tile_plan(raw[:, :3], 4.0, 0.5).tile_of)
