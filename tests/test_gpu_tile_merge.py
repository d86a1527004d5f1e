"""GPU: the kernels that join the instances of a scan's tiles (csrc/tile_merge.hip) bit for bit against the host statement
(postprocess.merge_tiles_host) at the shapes where they can go wrong, their caps, and predict_batches(tiles=...) end to
end."""
import numpy as np
import pytest
import torch

from tests.tile_merge_cases import build, chain_case, corners, hand_cases, in_box, random_case, strip, wall_case

pytestmark = pytest.mark.gpu


def _dev(per_tile):
    out = []
    for cls, scores, masks, pick in per_tile:
        if len(pick) == 0 and isinstance(masks, list):
            out.append(([], [], [], torch.zeros(0, dtype=torch.int64, device="cuda")))
        else:
            out.append(tuple(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (cls, scores, masks, pick)))
    return out


def _check(case):
    """Every kernel output of the case against the host statement, twice."""
    from geoformer_amd import postprocess

    plan, kw = case["plan"], case["kw"]
    want = postprocess.merge_tiles_host(plan, case["per_tile"], return_tables=True, **kw)
    dev = _dev(case["per_tile"])
    runs = [postprocess.merge_tiles(plan, dev, return_tables=True, **kw) for _ in range(2)]
    torch.cuda.synchronize()
    names = ("cls", "scores", "masks", "pick", "members")
    for got in runs:
        for name, g, w in zip(names, got, want):
            w = torch.from_numpy(w)
            assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g.cpu(), w), name
        for name in ("inter", "shared", "comp", "count", "row_tile"):
            w = torch.from_numpy(want[5][name])
            assert got[5][name].dtype == torch.int32 and torch.equal(got[5][name].cpu(), w), name
    for name, a, b in zip(names, runs[0], runs[1]):
        assert torch.equal(a, b), name
    for name in runs[0][5]:
        assert torch.equal(runs[0][5][name], runs[1][5][name]), name
    if "groups" in case:
        members = want[4].tolist()
        assert [[r for r, m in enumerate(members) if m == g] for g in range(len(case["groups"]))] == case["groups"]
    return want


@pytest.mark.parametrize("name", sorted(hand_cases()))
def test_hand_cases(hip, name):
    _check(hand_cases()[name])


@pytest.mark.parametrize("n", [1, 63, 65, 1000])
def test_tile_sizes_off_the_wave(hip, n):
    """Tile 1 holds exactly n points (n - 1 of them shared with tile 0, which holds 3001 + n - 1)."""
    xyz = np.concatenate([corners(0, 8), strip(n - 1, 3.6, 4.4, seed=n), strip(3000, 0, 3.4, seed=1)])
    zone = in_box(xyz, 3.6, 4.4)
    rows = [(0, np.concatenate([zone, in_box(xyz, 2, 3.4)]), 5, 0.5), (0, zone[::2], 6, 0.4),
            (1, np.arange(xyz.shape[0]), 5, 0.7), (1, zone[::2], 6, 0.3), (1, [1], 5, 0.2)]
    case = build(xyz, 4.0, 0.5, rows, kw=dict(min_shared=1, iom=0.5))
    assert case["plan"].offsets.tolist() == [0, 3000 + n, 3000 + 2 * n]
    want = _check(case)
    assert want[5]["inter"][0, 2] == n - 1


def test_pick_counts_at_the_word_boundaries_and_the_cap(hip):
    """3 x 3 tiles with p_s = 256, 0, 1, 32, 33, ...: the bitset's word boundaries, a tile without picks, the cap; halo
    0.4, so corner points lie in 4 tiles."""
    case = random_case(11, 20000, (9.0, 9.0), 3.0, 0.4, [256, 0, 1, 32, 33, 5, 64, 65, 2], n_objects=40)
    assert case["plan"].T == 9 and (case["plan"].tile_of[:, 3] >= 0).sum() > 50
    assert [len(t[3]) for t in case["per_tile"]] == [256, 0, 1, 32, 33, 5, 64, 65, 2]
    want = _check(case)
    assert want[0].shape[0] < 458 and (want[5]["inter"] > 0).sum() > 100  # something merged, much overlaps


def test_larger_scan_and_zero_halo(hip):
    want = _check(random_case(12, 50000, (12.0, 8.0), 4.0, 0.5, [20, 7, 33, 12, 9, 40], n_objects=30))
    assert want[0].shape[0] < 121
    case = random_case(13, 5000, (9.0, 6.0), 3.0, 0.0, 6)
    assert (case["plan"].tile_of[:, 1] == -1).all()
    want = _check(case)
    assert not want[5]["inter"].any() and want[0].shape[0] == 36


def test_one_row_and_one_tile(hip):
    xyz = np.concatenate([corners(0, 3), strip(2999, 0, 3, seed=2)])
    case = build(xyz, 4.0, 0.5, [(0, in_box(xyz, 1, 2), 5, 0.5)], groups=[[0]])
    assert case["plan"].T == 1
    want = _check(case)
    assert want[2].shape == (1, 3001) and want[5]["count"][0] == in_box(xyz, 1, 2).size


def test_one_counter_from_every_wave(hip):
    """30 000 of the scan's points lie in both tiles and in both masks: every wave of the overlap launch adds to
    inter[0, 1], inter[1, 0], shared[0, 1] and shared[1, 0], and every wave of the assemble launch to count[0]."""
    case = wall_case()
    want = _check(case)
    assert want[5]["inter"][0, 1] >= case["n_zone"] > 10000 and want[5]["count"][0] == case["plan"].N


def test_long_chain(hip):
    """300 rows in one chain: the union-find hooks 299 edges whose rows are far apart, and halves long paths."""
    want = _check(chain_case(links=150))
    assert want[4].shape == (300,) and want[0].shape == (1,) and want[1][0] == np.float32(0.9)


def test_caps_raise_before_any_launch(hip):
    from geoformer_amd import _lib, pointops, postprocess, scene

    assert pointops.tile_limits() == (4096, 256)
    rng = np.random.default_rng(0)
    xyz = np.concatenate([corners(0, 20, 0, 16), np.stack([rng.uniform(0, 20, 4000), rng.uniform(0, 16, 4000),
                                                           np.zeros(4000)], 1)])
    plan = scene.tile_plan(xyz, 4.0, 0.5)
    assert plan.T == 20

    def tiles(p_of):
        out = []
        for s in range(plan.T):
            n_s = int(plan.offsets[s + 1] - plan.offsets[s])
            out.append((torch.zeros(1, dtype=torch.int64, device="cuda"), torch.ones(1, device="cuda"),
                        torch.ones((1, n_s), dtype=torch.int32, device="cuda"),
                        torch.zeros(p_of(s), dtype=torch.int64, device="cuda")) if p_of(s) else
                       ([], [], [], torch.zeros(0, dtype=torch.int64, device="cuda")))
        return out

    with pytest.raises(RuntimeError, match="at most 256"):
        postprocess.merge_tiles(plan, tiles(lambda s: 257 if s == 3 else 1))
    with pytest.raises(RuntimeError, match="at most 4096"):
        postprocess.merge_tiles(plan, tiles(lambda s: 256 if s < 17 else 0))  # 4352 rows
    # 4096 rows exactly pass (every row is the same all-ones mask of its tile: neighbours merge)
    cls, scores, masks, pick, members = postprocess.merge_tiles(plan, tiles(lambda s: 256 if s < 16 else 0))
    assert members.shape == (4096,) and masks.shape[1] == plan.N and 1 <= masks.shape[0] <= 16
    # the library's own check of the host table
    table = np.zeros((1, pointops.TILE_SCENE_FIELDS), np.int64)
    table[0] = (0, 1, 0, 0, 257, 0, 0)
    dummy = torch.zeros(8, dtype=torch.int64, device="cuda")
    assert hip.gf_tile_pack_picks(dummy.data_ptr(), table.ctypes.data, 1, 257, dummy.data_ptr(), _lib.stream_ptr()) == -1
    table[0] = (0, 1, 0, 0, 2, 1, 0)  # first row does not follow
    assert hip.gf_tile_pack_picks(dummy.data_ptr(), table.ctypes.data, 1, 2, dummy.data_ptr(), _lib.stream_ptr()) == -1
    assert hip.gf_tile_merge(None, None, None, None, None, 4097, 1, 0.5, 20, None, None, dummy.data_ptr(), None, None,
                             _lib.stream_ptr()) == -1
    torch.cuda.synchronize()


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


def _scan(rooms=4, n=6000):
    """`rooms` small rooms side by side along x, 1.7 m apart: one raw [rooms * n, 8] scan of about 6.7 x 1.6 m."""
    from geoformer_amd import scene

    parts = []
    for i in range(rooms):
        r = scene.make_raw_scene(n + 500 * i, 60 + i, n_boxes=1, room=(1.6, 1.6, 0.6))
        r[:, 0] += 1.7 * i
        r[:, 7] = np.where(r[:, 7] >= 0, r[:, 7] + 100 * i, r[:, 7])
        parts.append(r)
    return np.concatenate(parts)


KW = dict(reserve=False, final_score_thresh=0.0)


def _predict(model, items, batch_size, **kw):
    from geoformer_amd import batch_eval

    np.random.seed(21)
    out = list(batch_eval.predict_batches(model, items, batch_size, **KW, **kw))
    torch.cuda.synchronize()
    return out


def _same(a, b):
    return all(torch.is_tensor(x) == torch.is_tensor(y) and (not torch.is_tensor(x) or torch.equal(x, y))
               for x, y in zip(a[1:], b[1:])) and a[0] == b[0]


def test_predict_batches_one_tile_equals_untiled(model):
    from geoformer_amd import batch_eval

    items = [("scan", _scan(2)), ("room", _scan(1))]
    plain, again = _predict(model, items, 2), _predict(model, items, 2)
    assert all(_same(a, b) for a, b in zip(plain, again))  # the untiled loop repeats exactly
    tiled = _predict(model, items, 2, tiles=batch_eval.Tiling(tile=100.0, max_points=10000))
    assert [r[0] for r in tiled] == ["scan", "room"] and _same(plain[1], tiled[1])  # the small scene passes through
    (_, c0, s0, m0, p0), (_, c1, s1, m1, p1) = plain[0], tiled[0]
    assert torch.is_tensor(c0) and p0.numel() > 0, "the untiled forward picked nothing: nothing is compared"
    print(f"T = 1: {p0.numel()} picks of {c0.shape[0]} proposals")
    assert torch.equal(c1, c0[p0]) and torch.equal(s1, s0[p0]) and torch.equal(m1, (m0[p0] != 0).int())
    assert m1.dtype == torch.int32 and torch.equal(p1, torch.sort(-s1, stable=True)[1])


def test_predict_batches_tiled_equals_host_merge_of_the_tiles(model):
    from geoformer_amd import batch_eval, postprocess

    items = [("room", _scan(1)), ("scan", _scan(4))]
    tiling = batch_eval.Tiling(tile=3.5, halo=0.3, max_points=10000, min_shared=10)
    expanded, plans = batch_eval.tile_items(items, tiling)
    plan = plans["scan"]
    assert plan.T == 2 and [n for n, _ in expanded] == ["room", ("scan", 0), ("scan", 1)]
    assert (plan.tile_of[:, 1] >= 0).sum() > 500
    per, again = _predict(model, expanded, 2), _predict(model, expanded, 2)
    assert all(_same(a, b) for a, b in zip(per, again))  # the untiled loop over the tiles repeats exactly
    tiled = _predict(model, items, 2, tiles=tiling)
    assert [r[0] for r in tiled] == ["room", "scan"] and _same(per[0], tiled[0])
    host = [tuple(x.cpu().numpy() if torch.is_tensor(x) else x for x in r[1:]) for r in per[1:]]
    assert sum(len(t[3]) for t in host) > 0, "no tile picked anything: nothing is merged"
    want = postprocess.merge_tiles_host(plan, host, iom=0.5, min_shared=10)
    _, cls, scores, masks, pick = tiled[1]
    print(f"T = 2: {[len(t[3]) for t in host]} picks -> {want[0].shape[0]} instances over {plan.N} points")
    for name, g, w in zip(("cls", "scores", "masks", "pick"), (cls, scores, masks, pick), want):
        assert torch.equal(g.cpu(), torch.from_numpy(w)), name
    assert masks.shape == (want[0].shape[0], plan.N)


def test_label_batches_and_evaluate_accept_tiles(model):
    from geoformer_amd import batch_eval

    items = [("scan", _scan(4))]
    tiling = batch_eval.Tiling(tile=3.5, halo=0.3, max_points=10000, min_shared=10)
    np.random.seed(21)
    ((name, lab),) = list(batch_eval.label_batches(model, items, 2, tiles=tiling, min_score=0.0, **KW))
    N = items[0][1].shape[0]
    assert name == "scan" and lab.ids.shape == lab.owner.shape == (N,) and (lab.owner >= 0).any()
    np.random.seed(21)
    ap, avgs = batch_eval.evaluate(model, items, 2, classes=0, tiles=tiling, **KW)
    assert "all_ap" in avgs
    with pytest.raises(ValueError, match="a Tiling"):
        list(batch_eval.predict_batches(model, items, 2, tiles="yes", **KW))


def test_semantic_with_tiles_raises(model):
    from geoformer_amd import batch_eval, evaluation

    items = [("scan", _scan(1))]
    tiling = batch_eval.Tiling(max_points=1000)
    ev = evaluation.SemanticEvaluator(train_fold=model.cfg.train_fold)
    with pytest.raises(ValueError, match="not supported with tiles yet"):
        list(batch_eval.predict_batches(model, items, 1, tiles=tiling, semantic=ev, **KW))
    with pytest.raises(ValueError, match="not supported with tiles yet"):
        list(batch_eval.panoptic_batches(model, items, 1, tiles=tiling, **KW))
