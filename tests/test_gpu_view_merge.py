"""GPU: the kernels that join the instances of a scan's views (csrc/view_merge.hip) bit for bit against the host statement
(postprocess.merge_views_host, mean_views_host) on every case of tests/view_merge_cases.py and at the shapes where the
launches can go wrong, their caps, and predict_batches(views=...) end to end."""
import numpy as np
import pytest
import torch

from tests.view_merge_cases import (F, all_views_case, case, chain_case, hand_cases, random_case, random_cases, view,
                                    wall_case)

pytestmark = pytest.mark.gpu

TILE, CHUNK_POINTS = 64, 32 * 32  # the overlap kernel's row block and the points of one LDS stage


def _dev(per_view):
    out = []
    for cls, scores, masks, pick in per_view:
        if isinstance(masks, list):
            out.append(([], [], [], torch.zeros(0, dtype=torch.int64, device="cuda")))
        else:
            out.append(tuple(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (cls, scores, masks, pick)))
    return out


NAMES = ("cls", "scores", "masks", "pick")
TABLES = ("inter", "cnt", "best", "comp", "members", "support", "count", "row_view")


def _check(c):
    """Every kernel output of the case against the host statement, twice."""
    from geoformer_amd import postprocess

    want = postprocess.merge_views_host(c["per_view"], c["N"], return_tables=True, **c["kw"])
    dev = _dev(c["per_view"])
    runs = [postprocess.merge_views(dev, c["N"], return_tables=True, **c["kw"]) for _ in range(2)]
    torch.cuda.synchronize()
    for got in runs:
        for name, g, w in zip(NAMES, got, want):
            w = torch.from_numpy(w)
            assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g.cpu(), w), name
        for name in TABLES:
            w = torch.from_numpy(want[4][name])
            assert got[4][name].dtype == torch.int32 and got[4][name].shape == w.shape, name
            assert torch.equal(got[4][name].cpu(), w), name
    for name, a, b in zip(NAMES, runs[0], runs[1]):
        assert torch.equal(a, b), name
    for name in TABLES:
        assert torch.equal(runs[0][4][name], runs[1][4][name]), name
    return want


@pytest.mark.parametrize("name", sorted(hand_cases()))
def test_hand_cases(hip, name):
    c = hand_cases()[name]
    want = _check(c)
    assert want[4]["members"].tolist() == c["expect"]["members"]


def test_random_cases(hip):
    for c in random_cases():
        _check(c)


@pytest.mark.parametrize("N", [1, 31, 32, 33, 63, 64, 65, CHUNK_POINTS - 1, CHUNK_POINTS, CHUNK_POINTS + 1,
                               2 * CHUNK_POINTS - 1, 2 * CHUNK_POINTS + 1])
def test_point_counts_at_the_word_and_chunk_boundaries(hip, N):
    want = _check(random_case(N, N=N, V=3, picks=[5, 4, 6], n_objects=4))
    assert want[4]["cnt"].shape == (15,)
    # the last point of the scan in a row of every view: the last word's last used bit
    c = case(N, [[({N - 1}, 1, 0.5)], [({N - 1, 0}, 1, 0.6)], [(set(range(N)), 1, 0.7)]], iou=0.0, min_views=1)
    want = _check(c)
    assert want[4]["inter"][0].tolist() == [1, 1, 1] and want[4]["cnt"].tolist() == [1, min(N, 2), N]


@pytest.mark.parametrize("P", [1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_row_counts_at_the_row_block_boundaries(hip, P):
    picks = [P - P // 2, P // 2]
    want = _check(random_case(50 + P, N=300, V=2, picks=picks, n_objects=12))
    assert want[4]["cnt"].shape == (P,)


def test_no_rows(hip):
    want = _check(case(40, [[], [], []]))
    assert want[0].shape == (0,) and want[2].shape == (0, 40) and want[4]["inter"].shape == (0, 0)
    want = _check(case(40, [[]]))
    assert want[4]["best"].shape == (0, 1)


@pytest.mark.parametrize("p_v", [31, 32, 33])
def test_picks_of_a_view_off_the_wave(hip, p_v):
    """gf_view_best deals the rows of a view over 64 lanes: p_v of 31 .. 33 and (twice that) 62 .. 66."""
    _check(random_case(p_v, N=257, V=3, picks=[p_v, 2 * p_v, 3], n_objects=20))


@pytest.mark.parametrize("V", [1, 2, 31, 32])
def test_view_counts(hip, V):
    want = _check(random_case(70 + V, N=150, V=V, picks=3, n_objects=3))
    assert want[4]["best"].shape == (3 * V, V)


def test_a_component_over_all_32_views(hip):
    want = _check(all_views_case())
    assert want[4]["support"].tolist() == [32] and want[4]["comp"].tolist() == [0] * 32
    assert want[2].sum() == 70 - 32  # vote = 1: the points that all the views hold


def test_long_chain(hip):
    """60 rows in one chain over three views: the union-find hooks 59 edges and halves long paths; the member list of the
    one instance is the sort's whole output."""
    want = _check(chain_case(60))
    assert want[4]["comp"].tolist() == [0] * 60 and want[4]["support"].tolist() == [3] and want[0].shape == (1,)


def test_one_counter_from_every_wave(hip):
    """Every wave of the pack launch adds to cnt[0] and cnt[1], every wave of the assemble launch to count[0]."""
    want = _check(wall_case())
    assert want[4]["cnt"].tolist() == [20000, 20000] and want[4]["count"].tolist() == [20000]


@pytest.mark.parametrize("N", [1000, 1500])
def test_every_cell_is_written(hip, N):
    """inter and masks filled with garbage before the calls: gf_view_overlaps and gf_view_assemble define every cell.
    P = 101 rows are two row blocks, so the mirror images of the off-diagonal block are stored too.  N = 1000 is one LDS
    stage of words: every cell is stored by the one workgroup that owns it, nothing is zeroed first; N = 1500 is two
    stages, split over two workgroups: a memset of the call and integer atomic adds."""
    from geoformer_amd import pointops, postprocess, view_merge

    c = random_case(7, N=N, V=3, picks=[40, 30, 31], n_objects=25)
    assert -(-N // CHUNK_POINTS) == (1 if N == 1000 else 2)  # LDS stages of words
    c["kw"]["min_views"] = 1
    want = postprocess.merge_views_host(c["per_view"], c["N"], return_tables=True, **c["kw"])
    N, kw = c["N"], c["kw"]
    rows = [(m, p, k, s) for k, s, m, p in _dev(c["per_view"])]
    table, sizes = postprocess.view_scene_table(rows, N)
    P = sizes["rows"]
    table_d = pointops._table_dev(table, "cuda")
    row_view, view_first = (torch.from_numpy(sizes[k]).cuda() for k in ("row_view", "view_first"))
    cls_all = torch.cat([k[p] for _, p, k, _ in rows]).contiguous()
    sc_all = torch.cat([s[p] for _, p, _, s in rows]).contiguous()
    bits, cnt = view_merge.view_pack(table_d, table, N)
    inter = torch.full((P, P), -12345, dtype=torch.int32, device="cuda")
    assert view_merge.view_overlaps(bits, N, out=inter) is inter
    assert torch.equal(inter.cpu(), torch.from_numpy(want[4]["inter"]))
    best = view_merge.view_best(inter, cnt, cls_all, row_view, view_first)
    merged = view_merge.view_merge(inter, cnt, best, cls_all, sc_all, row_view, kw["iou"], kw["min_views"])
    G = int(merged["G"].item())
    assert G == want[0].shape[0] > 3
    masks = torch.full((G, N), 77, dtype=torch.int32, device="cuda")
    got, count = view_merge.view_assemble(bits, merged, row_view, G, N, kw["vote"], out=masks)
    assert got is masks and torch.equal(masks.cpu(), torch.from_numpy(want[2]))
    assert torch.equal(count.cpu(), torch.from_numpy(want[4]["count"]))
    # the bitsets: the unused bits of the last word are zero
    b = bits.cpu().numpy().view(np.uint32)
    dense = np.unpackbits(b.view(np.uint8), axis=1, bitorder="little")
    assert dense.shape[1] == 32 * ((N + 31) // 32) and not dense[:, N:].any()
    assert (dense[:, :N].sum(1) == want[4]["cnt"]).all()


def _buf(shape, dtype, fill):
    return torch.full(shape, fill, dtype=dtype, device="cuda")


def test_caps_raise_before_any_launch(hip):
    from geoformer_amd import _lib, pointops, postprocess, view_merge

    assert view_merge.view_limits() == (4096, 32) and postprocess.VIEW_MAX_VIEWS == 32
    N = 8
    one = _dev([view(N, [({0, 1}, 1, 0.5)])])[0]

    def views(V, p):
        return [(one[0], one[1], one[2], torch.zeros(p, dtype=torch.int64, device="cuda")) for _ in range(V)]

    with pytest.raises(RuntimeError, match="at most 4096"):
        postprocess.merge_views(views(17, 241), N)  # 4097 rows
    with pytest.raises(ValueError, match="1 to 32"):
        postprocess.merge_views(views(33, 1), N)
    # 4096 rows exactly pass: every row is the same mask, so 128 rows per view tie and the first of each view joins
    cls, scores, masks, pick, tables = postprocess.merge_views(views(32, 128), N, min_views=32, return_tables=True)
    assert tables["members"].shape == (4096,) and masks.tolist() == [[1, 1, 0, 0, 0, 0, 0, 0]]
    assert tables["support"].tolist() == [32] and (tables["members"] == 0).sum() == 32
    # the wrappers: outputs given by the caller stay as they were
    bits = torch.zeros((4097, 1), dtype=torch.int32, device="cuda")
    inter = _buf((4097, 4097), torch.int32, 5)
    with pytest.raises(RuntimeError, match="at most 4096"):
        view_merge.view_overlaps(bits, N, out=inter)
    x = torch.zeros((4, 65), device="cuda")
    out = _buf((4, 65), torch.float32, 5.0)
    with pytest.raises(RuntimeError, match="1 to 64"):
        view_merge.view_mean_scores(pointops._table_dev(postprocess.tile_score_table([x]), "cuda"),
                                  postprocess.tile_score_table([x]), 4, 65, out=out)
    with pytest.raises(RuntimeError, match="1 to 64"):
        postprocess.mean_views([x, x])
    y = torch.zeros((4, 2), device="cuda")
    out2 = _buf((4, 2), torch.float32, 5.0)
    t33 = postprocess.tile_score_table([y] * 33)
    with pytest.raises(RuntimeError, match="1 to 32"):
        view_merge.view_mean_scores(pointops._table_dev(t33, "cuda"), t33, 4, 2, out=out2)
    with pytest.raises(ValueError, match="1 to 32"):
        postprocess.mean_views([y] * 33)
    # the library's own checks, on buffers that must stay as they were
    d, st = _buf((64,), torch.int64, 5), _lib.stream_ptr()
    p = d.data_ptr()
    table = np.zeros((33, pointops.TILE_SCENE_FIELDS), np.int64)
    table[:, 2] = N
    assert hip.gf_view_pack(p, table.ctypes.data, 33, 0, N, p, p, st) == -1  # V = 33
    table[0] = (p, 1, N, p, 4097, 0, 0)
    assert hip.gf_view_pack(p, table.ctypes.data, 1, 4097, N, p, p, st) == -1  # P = 4097
    table[0] = (p, 1, N, p, 2, 1, 0)
    assert hip.gf_view_pack(p, table.ctypes.data, 1, 2, N, p, p, st) == -1  # first row does not follow
    table[0] = (p, 1, N + 1, p, 2, 0, 0)
    assert hip.gf_view_pack(p, table.ctypes.data, 1, 2, N, p, p, st) == -1  # n_s is not N
    table[0] = (p, 1, N, p, 2, 0, 0)
    assert hip.gf_view_pack(p, table.ctypes.data, 1, 3, N, p, p, st) == -1  # the picks do not add up to P
    assert hip.gf_view_overlaps(p, 4097, N, p, st) == -1
    assert hip.gf_view_overlaps(p, 2, 1 << 31, p, st) == -1
    assert hip.gf_view_best(p, p, p, p, p, 2, 33, p, st) == -1
    assert hip.gf_view_merge(p, p, p, p, p, p, 4097, 2, 0.5, 1, p, p, p, p, p, p, p, p, st) == -1
    assert hip.gf_view_merge(p, p, p, p, p, p, 2, 33, 0.5, 1, p, p, p, p, p, p, p, p, st) == -1
    assert hip.gf_view_merge(p, p, p, p, p, p, 2, 2, 0.5, 3, p, p, p, p, p, p, p, p, st) == -1  # min_views > V
    assert hip.gf_view_assemble(p, p, p, p, p, 2, 3, N, 0.5, p, p, st) == -1  # G > P
    assert hip.gf_view_assemble(p, p, p, p, p, 2, 1, N, 0.0, p, p, st) == -1  # vote = 0
    score = np.zeros((33, pointops.TILE_SCORE_FIELDS), np.int64)
    score[:] = (p, 4)
    assert hip.gf_view_mean_scores(p, score.ctypes.data, 33, 4, 2, p, st) == -1
    assert hip.gf_view_mean_scores(p, score.ctypes.data, 2, 4, 65, p, st) == -1
    assert hip.gf_view_mean_scores(p, score.ctypes.data, 2, 5, 2, p, st) == -1  # n_s is not N
    torch.cuda.synchronize()
    assert (d == 5).all() and (inter == 5).all() and (out == 5).all() and (out2 == 5).all()


@pytest.mark.parametrize("V", [1, 2, 3, 8])
@pytest.mark.parametrize("C", [1, 20, 64])
def test_mean_views(hip, V, C):
    from geoformer_amd import postprocess

    rng = np.random.default_rng(V * 100 + C)
    for N in (1, 257, 1000):  # off the workgroup's 256 threads
        xs = [(rng.standard_normal((N, C)) * 10 ** rng.uniform(-3, 3)).astype(F) for _ in range(V)]
        want = torch.from_numpy(postprocess.mean_views_host(xs))
        dev = [torch.from_numpy(x).cuda() for x in xs]
        a, b = postprocess.mean_views(dev), postprocess.mean_views(dev)
        assert a.dtype == torch.float32 and torch.equal(a.cpu(), want) and torch.equal(a, b)
    with pytest.raises(ValueError, match="contiguous"):
        postprocess.mean_views([torch.zeros((4, 2 * C), device="cuda")[:, ::2]] * V)
    assert postprocess.mean_views([torch.zeros((0, C), device="cuda")] * V).shape == (0, C)


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


def _host(rec):
    return tuple(x.cpu().numpy() if torch.is_tensor(x) else x for x in rec[1:])


def _equals_host_join(per, joined, views, names, sizes):
    """`joined` (the records of predict_batches(views=...)) against merge_views_host of `per` (the records of the views
    run as plain scenes, V per scene); returns the number of joins."""
    from geoformer_amd import postprocess

    V, joins = views.V, 0
    assert [r[0] for r in joined] == names and len(per) == V * len(names)
    for i, (rec, N) in enumerate(zip(joined, sizes)):
        host = [_host(r) for r in per[V * i:V * i + V]]
        assert sum(len(h[3]) > 0 for h in host) >= 2, "fewer than two views picked something: nothing is merged"
        want = postprocess.merge_views_host(host, N, iou=views.params["iou"], min_views=views.min_views,
                                            vote=views.params["vote"], return_tables=True)
        assert want[0].shape[0] > 0
        for name, g, w in zip(NAMES, rec[1:], want):
            assert torch.equal(g.cpu(), torch.from_numpy(w)), name
        assert rec[3].shape == (want[0].shape[0], N) and rec[3].dtype == torch.int32
        P = want[4]["comp"].shape[0]
        joins += P - np.unique(want[4]["comp"]).size
    return joins


def test_predict_batches_views_equals_host_join_of_the_views(model):
    from geoformer_amd import batch_eval

    items = [("room", _scan(1)), ("scan", _scan(2))]
    views = batch_eval.Views(rotations=4, iou=0.25, min_views=1)
    expanded = batch_eval.view_items(items, views)
    per = _predict(model, expanded, 2)
    joined = _predict(model, items, 2, views=views)
    joins = _equals_host_join(per, joined, views, ["room", "scan"], [r.shape[0] for _, r in items])
    print(f"V = 4: {[len(r[4]) for r in per]} picks, {joins} joins -> {[r[1].shape[0] for r in joined]} instances")


def test_views_over_tiles_and_under_density(model):
    from geoformer_amd import batch_eval

    items = [("scan", _scan(4))]
    N = items[0][1].shape[0]
    views = batch_eval.Views(rotations=2, iou=0.25, min_views=1)
    tiling = batch_eval.Tiling(tile=3.5, halo=0.3, max_points=10000, min_shared=10)
    expanded = batch_eval.view_items(items, views)
    assert len(batch_eval.tile_items(expanded, tiling)[0]) == 4  # every view is cut into two tiles
    per = _predict(model, expanded, 2, tiles=tiling)
    assert all(r[3].shape[1] == N for r in per)
    joined = _predict(model, items, 2, views=views, tiles=tiling)
    joins = _equals_host_join(per, joined, views, ["scan"], [N])
    print(f"tiles under views: {[len(r[4]) for r in per]} merged rows, {joins} joins -> {joined[0][1].shape[0]}")
    # density= above: the views are views of the subsampled scene, and the masks come back on the scan's own points
    density = batch_eval.Density(cell=0.05)
    sub, maps = batch_eval.density_items(items, density, "cuda")
    assert "scan" in maps and sub[0][1].shape[0] < N
    per = _predict(model, batch_eval.view_items(sub, views), 2)
    inner = _predict(model, sub, 2, views=views)
    joins = _equals_host_join(per, inner, views, ["scan"], [sub[0][1].shape[0]])
    dense = _predict(model, items, 2, views=views, density=density)
    assert dense[0][0] == "scan" and dense[0][3].shape == (inner[0][3].shape[0], N)
    assert torch.equal(dense[0][3], inner[0][3][:, maps["scan"].cell_of.long()])
    assert all(torch.equal(a, b) for a, b in zip((dense[0][1], dense[0][2], dense[0][4]),
                                                 (inner[0][1], inner[0][2], inner[0][4])))
    print(f"views under density: {sub[0][1].shape[0]} of {N} points, {joins} joins")


class _Tap:
    """Stands where predict_batches takes a SemanticEvaluator: keeps every scene's scores and labels, hands them on."""

    def __init__(self, inner):
        self.inner, self.scores, self.labels = inner, {}, {}

    def add_batch(self, scores, labels, offsets, names, offsets_host=None):
        off = offsets_host.tolist()
        for i, n in enumerate(names):
            self.scores[n] = scores[off[i]:off[i + 1]].clone()
            self.labels[n] = labels[off[i]:off[i + 1]].clone()
        return self.inner.add_batch(scores, labels, offsets, names, offsets_host=offsets_host)


def test_semantic_under_views(model):
    from geoformer_amd import batch_eval, evaluation, postprocess

    items = [("room", _scan(1)), ("scan", _scan(2))]
    views = batch_eval.Views(rotations=3, flip=True, iou=0.25, min_views=1)
    mk = lambda: evaluation.SemanticEvaluator(n_classes=model.cfg.classes, train_fold=model.cfg.train_fold)  # noqa: E731
    tap = _Tap(mk())
    _predict(model, batch_eval.view_items(items, views), 2, semantic=tap)
    assert len(tap.scores) == 12
    want_ev = mk()
    for name, raw in items:
        mean = postprocess.mean_views_host([tap.scores[(name, k)].cpu().numpy() for k in range(6)])
        s = torch.from_numpy(mean).cuda()
        off = torch.tensor([0, s.shape[0]], dtype=torch.int32)
        want_ev.add_batch(s, tap.labels[(name, 0)], off.cuda(), [name], offsets_host=off)
    ev = mk()
    joined_tap = _Tap(ev)
    out = _predict(model, items, 2, views=views, semantic=joined_tap)
    assert [r[0] for r in out] == ["room", "scan"] and sorted(joined_tap.scores) == ["room", "scan"]
    torch.cuda.synchronize()
    a, b = ev.confusion(), want_ev.confusion()
    assert np.array_equal(a, b) and a.sum() > 0
    # the semantic-only loop gives the same counts
    ev2 = mk()
    names = [n for n, _ in batch_eval.semantic_batches(model, items, 2, reserve=False, evaluator=ev2, views=views)]
    assert names == ["room", "scan"]
    assert np.array_equal(ev2.confusion(), b)


def _confusion_of(model, scored):
    """The confusion matrix of an evaluator given (name, host scores [N, C], raw scene) one scene at a time."""
    from geoformer_amd import batch_eval, evaluation

    ev = evaluation.SemanticEvaluator(n_classes=model.cfg.classes, train_fold=model.cfg.train_fold)
    for name, scores, raw in scored:
        s = torch.from_numpy(np.ascontiguousarray(scores)).cuda()
        lab = torch.from_numpy(batch_eval.scene_dict(raw)["label"]).cuda()
        off = torch.tensor([0, s.shape[0]], dtype=torch.int32)
        ev.add_batch(s, lab, off.cuda(), [name], offsets_host=off)
    torch.cuda.synchronize()
    return ev.confusion()


def test_semantic_under_views_over_tiles(model):
    """_TileSemantics -> _ViewSemantics -> the evaluator: every view's tiles are stitched, the stitched views averaged."""
    from geoformer_amd import batch_eval, evaluation, postprocess

    items = [("room", _scan(1)), ("scan", _scan(4))]
    views = batch_eval.Views(rotations=2, iou=0.25, min_views=1)
    tiling = batch_eval.Tiling(tile=3.5, halo=0.3, max_points=10000, min_shared=10)
    mk = lambda: evaluation.SemanticEvaluator(n_classes=model.cfg.classes, train_fold=model.cfg.train_fold)  # noqa: E731
    viewed = batch_eval.view_items(items, views)
    tiles, plans = batch_eval.tile_items(viewed, tiling)
    assert sorted(plans) == [("scan", 0), ("scan", 1)] and all(p.T == 2 for p in plans.values())
    tap = _Tap(mk())
    _predict(model, tiles, 2, semantic=tap)  # every tile of every view as a plain scene
    scored = []
    for name, raw in items:
        per_view = []
        for k in range(views.V):
            vn = batch_eval.ViewName(name, k)
            if vn in plans:
                got = [tap.scores.get(batch_eval.TileName(vn, s)) for s in range(plans[vn].T)]
                per_view.append(postprocess.stitch_tiles_host(plans[vn], [None if x is None else x.cpu().numpy()
                                                                         for x in got], "mean"))
            else:
                per_view.append(tap.scores[vn].cpu().numpy())
        scored.append((name, postprocess.mean_views_host(per_view), raw))
    want = _confusion_of(model, scored)
    ev = mk()
    joined = _Tap(ev)
    out = _predict(model, items, 2, views=views, tiles=tiling, stitch="mean", semantic=joined)
    torch.cuda.synchronize()
    assert [r[0] for r in out] == ["room", "scan"] and sorted(joined.scores) == ["room", "scan"]
    assert joined.scores["scan"].shape[0] == items[1][1].shape[0]
    assert np.array_equal(ev.confusion(), want) and want.sum() > 0
    ev2 = mk()
    names = [n for n, _ in batch_eval.semantic_batches(model, items, 2, reserve=False, evaluator=ev2, views=views,
                                                       tiles=tiling, stitch="mean")]
    assert names == ["room", "scan"] and np.array_equal(ev2.confusion(), want)


def test_semantic_under_density_and_views(model):
    """_ViewSemantics -> _DensitySemantics -> the evaluator: the subsampled scene's views are averaged, the mean is put
    back on the scan's own points and counted against the scan's own labels."""
    from geoformer_amd import batch_eval, evaluation, postprocess

    items = [("scan", _scan(2))]
    N = items[0][1].shape[0]
    views = batch_eval.Views(rotations=2, iou=0.25, min_views=1)
    density = batch_eval.Density(cell=0.05)
    mk = lambda: evaluation.SemanticEvaluator(n_classes=model.cfg.classes, train_fold=model.cfg.train_fold)  # noqa: E731
    sub, maps = batch_eval.density_items(items, density, "cuda")
    assert "scan" in maps and sub[0][1].shape[0] < N
    tap = _Tap(mk())
    _predict(model, batch_eval.view_items(sub, views), 2, semantic=tap)
    mean = postprocess.mean_views_host([tap.scores[("scan", k)].cpu().numpy() for k in range(2)])
    want = _confusion_of(model, [("scan", mean[maps["scan"].cell_of.cpu().numpy()], items[0][1])])
    ev = mk()
    joined = _Tap(ev)
    out = _predict(model, items, 2, views=views, density=density, semantic=joined)
    torch.cuda.synchronize()
    assert [r[0] for r in out] == ["scan"] and joined.scores["scan"].shape[0] == N
    assert np.array_equal(ev.confusion(), want) and want.sum() > 0


@pytest.mark.parametrize("how", ["mapping", "geometric", "split"])
def test_views_with_segments_and_split(model, how):
    """segments= (a mapping under the scenes' names, or computed per view) and split= apply to every view: the joined
    result equals the host join of the views run as plain scenes with the same ids / the same split."""
    from geoformer_amd import batch_eval, scene

    items = [("room", _scan(1)), ("scan", _scan(2))]
    views = batch_eval.Views(rotations=2, iou=0.25, min_views=1)
    expanded = batch_eval.view_items(items, views)
    if how == "mapping":
        segs = {n: scene.grid_segments(r) for n, r in items}
        kw = dict(segments=segs)
        per_kw = dict(segments={batch_eval.ViewName(n, k): segs[n] for n, _ in items for k in range(2)})
    elif how == "geometric":
        kw = per_kw = dict(segments="geometric")
    else:
        kw = per_kw = dict(split="largest")
    per = _predict(model, expanded, 2, **per_kw)
    bare = _predict(model, expanded, 2)
    assert not all(_same(a, b) for a, b in zip(per, bare)), f"{how} changes nothing here: nothing is shown"
    joined = _predict(model, items, 2, views=views, **kw)
    joins = _equals_host_join(per, joined, views, ["room", "scan"], [r.shape[0] for _, r in items])
    print(f"{how}: {[len(r[4]) for r in per]} picks, {joins} joins -> {[r[1].shape[0] for r in joined]} instances")


def test_the_loops_accept_views_and_use_the_scan_s_own_coordinates(model):
    from geoformer_amd import batch_eval

    raw = _scan(2)
    raw[:, :3] += np.array([10.0, 20.0, 0.0], np.float32)  # far from the origin: a rotated view lies elsewhere
    items = [("scan", raw)]
    views = batch_eval.Views(rotations=4, iou=0.25, min_views=1)
    np.random.seed(21)
    ((name, lab),) = list(batch_eval.label_batches(model, items, 2, views=views, min_score=0.0, **KW))
    N = raw.shape[0]
    assert name == "scan" and lab.ids.shape == lab.owner.shape == (N,) and (lab.owner >= 0).any()
    full = np.asarray(lab.table.count) > 0
    assert full.any()
    lo, hi = raw[:, :3].min(0), raw[:, :3].max(0)
    c = np.asarray(lab.table.centroid)[full]
    assert (c >= lo - 1e-3).all() and (c <= hi + 1e-3).all()
    np.random.seed(21)
    ap, avgs = batch_eval.evaluate(model, items, 2, classes=0, views=views, **KW)
    assert "all_ap" in avgs
    np.random.seed(21)
    res = batch_eval.evaluate_panoptic(model, items, 2, views=views, **KW)
    assert isinstance(res, dict) and res
    np.random.seed(21)
    res = batch_eval.evaluate_boxes(model, items, 2, views=views, **KW)
    assert isinstance(res, dict) and res


def test_views_none_is_the_parent_s_loop(model):
    items = [("scan", _scan(2)), ("room", _scan(1))]
    plain, none = _predict(model, items, 2), _predict(model, items, 2, views=None)
    assert torch.is_tensor(plain[0][1]) and all(_same(a, b) for a, b in zip(plain, none))


def test_one_view_is_a_filter_and_a_reordering(model):
    from geoformer_amd import batch_eval

    items = [("room", _scan(1))]
    ((_, c0, s0, m0, p0),) = _predict(model, items, 1)
    ((_, c1, s1, m1, p1),) = _predict(model, items, 1, views=batch_eval.Views(rotations=1))
    assert p0.numel() > 0
    keep = p0[(m0[p0] != 0).any(1)]
    assert torch.equal(c1, c0[keep]) and torch.equal(s1, s0[keep]) and torch.equal(m1, (m0[keep] != 0).int())
    assert torch.equal(p1, torch.sort(-s1, stable=True)[1])
