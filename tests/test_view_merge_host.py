"""CPU: the statement of the join across views (postprocess.merge_views_host, mean_views_host) against an independent
brute force in Python sets and fractions and against hand cases written out; batch_eval.Views, view_items, ViewName and
the argument checks of predict_batches(views=...)."""
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests.view_merge_cases import F, hand_cases, mean32, random_cases, view


def brute(per_view, N, iou=0.5, min_views=None, vote=0.5):
    """The join, restated with sets and exact fractions; also what happened on the way (joins, ties, rejected pairs)."""
    V = len(per_view)
    min_views = (V + 1) // 2 if min_views is None else min_views
    rows = []  # (view, points, class, score)
    for v, (cls, scores, masks, pick) in enumerate(per_view):
        for r in [int(x) for x in pick]:
            if 0 <= r < len(masks):
                rows.append((v, {p for p in range(N) if masks[r][p] != 0}, int(cls[r]), F(scores[r])))
            else:
                rows.append((v, set(), int(cls[0]), F(scores[0])))
    P = len(rows)
    stats = dict(joins=0, ties=0, rejected=0)

    def frac(a, b):
        i = len(rows[a][1] & rows[b][1])
        return Fraction(i, len(rows[a][1] | rows[b][1])) if i else None

    best = [[-1] * V for _ in range(P)]
    for a in range(P):
        for v in range(V):
            if v == rows[a][0]:
                continue
            cands = [(frac(a, b), b) for b in range(P) if rows[b][0] == v and rows[b][2] == rows[a][2] and frac(a, b)]
            if cands:
                top = max(f for f, _ in cands)
                winners = [b for f, b in cands if f == top]
                stats["ties"] += len(winners) > 1
                best[a][v] = min(winners)
    adj = {a: set() for a in range(P)}
    for a in range(P):
        for b in range(a + 1, P):
            if rows[a][0] != rows[b][0] and best[a][rows[b][0]] == b and best[b][rows[a][0]] == a:
                i, u = len(rows[a][1] & rows[b][1]), len(rows[a][1] | rows[b][1])
                if float(i) >= iou * float(u):
                    adj[a].add(b), adj[b].add(a)
                    stats["joins"] += 1
                else:
                    stats["rejected"] += 1
    comp = [-1] * P
    for a in range(P):
        if comp[a] < 0:
            todo = [a]
            while todo:
                x = todo.pop()
                if comp[x] < 0:
                    comp[x] = a
                    todo += adj[x]
    inst = []
    for rep in sorted(set(comp)):
        mem = [r for r in range(P) if comp[r] == rep]
        support = len({rows[r][0] for r in mem})
        if support < min_views or not any(rows[r][1] for r in mem):
            continue
        acc = None
        votes = [0] * N
        for v in range(V):
            mv = [rows[r] for r in mem if rows[r][0] == v]
            m = max([r[3] for r in mv], default=F(0))
            acc = F(m) if acc is None else F(acc + m)
            for p in set().union(*[r[1] for r in mv]) if mv else ():
                votes[p] += 1
        mask = {p for p in range(N) if votes[p] > 0 and float(votes[p]) >= vote * float(support)}
        inst.append((rep, rows[rep][2], F(acc / F(V)), mask, support))
    gid = {rep: g for g, (rep, *_) in enumerate(inst)}
    return dict(members=[gid.get(c, -1) for c in comp], comp=comp, best=best, cls=[i[1] for i in inst],
                scores=[i[2] for i in inst], masks=[i[3] for i in inst], support=[i[4] for i in inst], stats=stats)


def check_against(want, got, N):
    cls, scores, masks, pick, tables = got
    G = len(want["cls"])
    assert cls.dtype == np.int64 and scores.dtype == np.float32 and masks.dtype == np.int32 and pick.dtype == np.int64
    assert cls.tolist() == list(want["cls"]) and masks.shape == (G, N) and scores.shape == (G,)
    assert scores.tobytes() == np.asarray(want["scores"], np.float32).tobytes()
    assert [set(np.nonzero(m)[0].tolist()) for m in masks] == [set(m) for m in want["masks"]]
    assert set(np.unique(masks).tolist()) <= {0, 1}
    assert pick.tolist() == sorted(range(G), key=lambda g: -scores[g])  # (sorted is stable)
    assert tables["members"].tolist() == list(want["members"]) and tables["support"].tolist() == list(want["support"])
    assert tables["count"].tolist() == [len(m) for m in want["masks"]]
    if "best" in want:
        assert tables["best"].tolist() == want["best"] and tables["comp"].tolist() == want["comp"]


@pytest.mark.parametrize("name", sorted(hand_cases()))
def test_hand_cases(name):
    from geoformer_amd import postprocess

    c = hand_cases()[name]
    got = postprocess.merge_views_host(c["per_view"], c["N"], return_tables=True, **c["kw"])
    check_against(c["expect"], got, c["N"])
    check_against(brute(c["per_view"], c["N"], **c["kw"]), got, c["N"])
    t = got[4]
    P = t["cnt"].shape[0]
    assert t["inter"].shape == (P, P) and (t["inter"] == t["inter"].T).all() and (np.diag(t["inter"]) == t["cnt"]).all()
    assert postprocess.merge_views_host(c["per_view"], c["N"], **c["kw"])[4] is None


def test_the_chain_is_one_component_of_four_rows():
    from geoformer_amd import postprocess

    c = hand_cases()["chain_through_one_view"]
    t = postprocess.merge_views_host(c["per_view"], c["N"], return_tables=True, **c["kw"])[4]
    assert t["comp"].tolist() == [0, 0, 0, 0] and t["support"].tolist() == [3] and t["count"].tolist() == [10]
    assert t["best"].tolist() == [[-1, 2, 3], [-1, -1, 3], [0, -1, 3], [1, 2, -1]]


def test_random_cases_against_the_brute_force():
    from geoformer_amd import postprocess

    cases = random_cases()
    assert len(cases) >= 40
    total = dict(joins=0, ties=0, rejected=0)
    for c in cases:
        want = brute(c["per_view"], c["N"], **c["kw"])
        check_against(want, postprocess.merge_views_host(c["per_view"], c["N"], return_tables=True, **c["kw"]), c["N"])
        for k in total:
            total[k] += want["stats"][k]
    print(total)
    assert all(v > 0 for v in total.values()), total
    assert {len(c["per_view"]) for c in cases} == set(range(1, 7))


def test_merge_views_host_rejects_bad_arguments():
    from geoformer_amd import postprocess

    one = [view(4, [({0}, 1, 0.5)])]
    for kw in (dict(vote=0.0), dict(vote=1.5), dict(min_views=0), dict(min_views=2), dict(iou=float("nan"))):
        with pytest.raises(ValueError):
            postprocess.merge_views_host(one, 4, **kw)
    with pytest.raises(ValueError, match="views"):
        postprocess.merge_views_host([], 4)
    with pytest.raises(ValueError, match="views"):
        postprocess.merge_views_host(one * 33, 4)
    with pytest.raises(ValueError, match="do not fit"):
        postprocess.merge_views_host(one, 5)
    assert postprocess.VIEW_DEFAULTS == dict(iou=0.5, min_views=None, vote=0.5)
    # CPU tensors run the statement and come back as tensors
    t = [tuple(torch.from_numpy(x) for x in one[0])]
    cls, scores, masks, pick, tables = postprocess.merge_views(t, 4)
    assert torch.is_tensor(masks) and masks.tolist() == [[1, 0, 0, 0]] and tables is None


def test_mean_views_host():
    from geoformer_amd import postprocess

    rng = np.random.default_rng(3)
    for V in (1, 2, 3, 5, 8):
        xs = [rng.standard_normal((7, 4)).astype(F) for _ in range(V)]
        want = np.zeros((7, 4), F)
        for i in range(7):
            for j in range(4):
                acc = xs[0][i, j]
                for x in xs[1:]:
                    acc = F(acc + x[i, j])
                want[i, j] = F(acc / F(V))
        got = postprocess.mean_views_host(xs)
        assert got.dtype == np.float32 and got.tobytes() == want.tobytes()
        assert torch.equal(postprocess.mean_views([torch.from_numpy(x) for x in xs]), torch.from_numpy(want))
    # 0.1 + 0.2 + 0.7 over 3: neither the sum nor the division is exact
    assert postprocess.mean_views_host([np.full((1, 1), v, F) for v in (0.1, 0.2, 0.7)])[0, 0] == mean32(0.1, 0.2, 0.7)
    with pytest.raises(ValueError, match="float32"):
        postprocess.mean_views_host([np.zeros((2, 2))])
    with pytest.raises(ValueError, match="expected scores"):
        postprocess.mean_views_host([np.zeros((2, 2), F), np.zeros((3, 2), F)])
    with pytest.raises(ValueError, match="views"):
        postprocess.mean_views_host([])


def test_views_validation_and_matrices():
    from geoformer_amd.batch_eval import Views

    v = Views()
    assert v.V == 4 and v.min_views == 2 and v.params["iou"] == 0.5 and v.params["vote"] == 0.5
    assert Views.DEFAULTS == dict(rotations=4, flip=False, matrices=None, iou=0.5, min_views=None, vote=0.5)
    assert "rotations=4" in repr(v) and repr(Views(iou=0.25)).startswith("Views(")
    want = [[[1, 0, 0], [0, 1, 0], [0, 0, 1]], [[0, 1, 0], [-1, 0, 0], [0, 0, 1]],
            [[-1, 0, 0], [0, -1, 0], [0, 0, 1]], [[0, -1, 0], [1, 0, 0], [0, 0, 1]]]
    assert v.matrices.dtype == np.float64 and v.matrices.tolist() == want  # exact 0 / +-1: no cos(pi / 2)
    e = Views(rotations=8)
    assert e.V == 8 and e.min_views == 4 and e.matrices[::2].tolist() == want
    h = np.sqrt(0.5)
    assert np.allclose(e.matrices[1], [[h, h, 0], [-h, h, 0], [0, 0, 1]], atol=1e-15)
    # view k turns the points by 360 k / rotations degrees about z
    assert np.allclose(np.array([1.0, 0, 5]) @ Views(rotations=3).matrices[1], [-0.5, np.sqrt(0.75), 5])
    f = Views(rotations=2, flip=True)
    assert f.V == 4 and f.min_views == 2
    assert f.matrices.tolist() == [want[0], [[-1, 0, 0], [0, 1, 0], [0, 0, 1]], want[2], [[1, 0, 0], [0, -1, 0], [0, 0, 1]]]
    for k in (0, 2):  # the twin is the rotation followed by x -> -x
        assert np.array_equal(f.matrices[k + 1], f.matrices[k] @ np.diag([-1.0, 1, 1]))
    assert Views(rotations=1).V == 1 and Views(rotations=1).min_views == 1
    assert Views(rotations=32).V == 32 and Views(rotations=16, flip=True).V == 32
    with pytest.raises(TypeError, match="unknown parameter"):
        Views(rotation=4)
    for kw in (dict(rotations=0), dict(rotations=33), dict(rotations=17, flip=True), dict(rotations=2.5),
               dict(iou=-0.1), dict(iou=1.5), dict(vote=0.0), dict(vote=1.1), dict(min_views=0), dict(min_views=5),
               dict(min_views=1.5)):
        with pytest.raises(ValueError):
            Views(**kw)
    m = Views(matrices=[np.eye(3), np.diag([1.0, -1, 1])])
    assert m.V == 2 and m.matrices.dtype == np.float64
    with pytest.raises(ValueError, match="identity"):
        Views(matrices=[np.diag([1.0, -1, 1])])
    with pytest.raises(ValueError, match="orthogonal"):
        Views(matrices=[np.eye(3), np.eye(3) * 1.001])
    with pytest.raises(ValueError, match="orthogonal"):
        Views(matrices=[np.eye(3), np.eye(3) + 1e-8])
    with pytest.raises(ValueError, match=r"\[V, 3, 3\]"):
        Views(matrices=np.eye(3))
    with pytest.raises(ValueError, match=r"\[V, 3, 3\]"):
        Views(matrices=[np.eye(3)] * 33)


def test_view_items_and_view_name():
    from geoformer_amd.batch_eval import TileName, ViewName, Views, view_items

    n = ViewName("s", 2)
    assert n == ("s", 2) and isinstance(n, tuple) and not isinstance(n, TileName) and hash(n) == hash(("s", 2))
    assert ViewName("s", np.int64(1))[1] == 1 and type(ViewName("s", np.int64(1))[1]) is int
    rng = np.random.default_rng(0)
    raw = rng.uniform(-2, 2, (50, 8)).astype(np.float32)
    other = torch.from_numpy(rng.uniform(-2, 2, (9, 8)).astype(np.float32))
    views = Views(rotations=4, flip=True)
    items = view_items([("a", raw), ("b", other)], views)
    assert [x[0] for x in items] == [("a", k) for k in range(8)] + [("b", k) for k in range(8)]
    assert all(isinstance(x[0], ViewName) for x in items) and items[0][1] is raw and items[8][1] is other
    for k in range(8):
        got = items[k][1]
        assert got.shape == raw.shape and got.dtype == raw.dtype and np.array_equal(got[:, 3:], raw[:, 3:])
        assert np.array_equal(got[:, :3], (raw[:, :3].astype(np.float64) @ views.matrices[k]).astype(np.float32))
    assert np.array_equal(items[2][1][:, :3], np.stack([-raw[:, 1], raw[:, 0], raw[:, 2]], 1))  # 90 degrees, exactly
    assert np.array_equal(items[11][1][:, 0], -(-other.numpy()[:, 1]))  # view 3 of b: 90 degrees, then mirrored
    assert np.array_equal(raw, items[0][1]) and view_items([], views) == []


class _Untouchable:
    """A model that raises when anything is asked of it."""

    def __getattr__(self, name):
        raise AssertionError(f"the model was touched ({name}) before the arguments were checked")


def test_predict_batches_checks_its_arguments_before_the_model():
    from geoformer_amd import batch_eval

    raw = np.zeros((10, 8), np.float32)
    items = [("a", raw), ("b", raw)]
    for bad in ("yes", 4, dict(rotations=4), batch_eval.Tiling()):
        with pytest.raises(ValueError, match="None or a Views"):
            list(batch_eval.predict_batches(_Untouchable(), items, 2, views=bad))
        with pytest.raises(ValueError, match="None or a Views"):
            list(batch_eval.predict_batches(_Untouchable(), items, 2, views=bad, density=batch_eval.Density()))
        with pytest.raises(ValueError, match="None or a Views"):
            list(batch_eval.semantic_batches(_Untouchable(), items, 2, views=bad))
    views = batch_eval.Views(rotations=2)
    twice = [("a", raw), ("b", raw), ("a", raw)]
    with pytest.raises(ValueError, match="share their name"):
        list(batch_eval.predict_batches(_Untouchable(), twice, 2, views=views, semantic=object()))
    with pytest.raises(ValueError, match="share their name"):
        list(batch_eval.predict_batches(_Untouchable(), twice, 2, views=views, semantic=object(),
                                        density=batch_eval.Density()))
    with pytest.raises(ValueError, match="share their name"):
        list(batch_eval.semantic_batches(_Untouchable(), twice, 2, views=views))
    with pytest.raises(ValueError, match="stitch= goes with tiles="):
        list(batch_eval.predict_batches(_Untouchable(), items, 2, views=views, stitch="mean"))
    # the keyword reaches the loops that pass **kw on
    for fn in (batch_eval.evaluate, batch_eval.evaluate_boxes, batch_eval.evaluate_semantic):
        with pytest.raises(ValueError, match="None or a Views"):
            fn(_UntouchableCfg(), items, 2, views="yes")
    for gen in (batch_eval.label_batches, batch_eval.panoptic_batches):
        with pytest.raises(ValueError, match="None or a Views"):
            list(gen(_UntouchableCfg(), items, 2, views="yes", device="cpu"))
    with pytest.raises(ValueError, match="None or a Views"):
        batch_eval.evaluate_panoptic(_UntouchableCfg(), items, 2, views="yes", device="cpu")


class _UntouchableCfg:
    """The loops around predict_batches read the model's cfg (and its parameters' device) for their own defaults first."""

    class cfg:
        cvfold, classes, train_fold = 0, 20, 0

    def parameters(self):
        return iter([torch.zeros(1)])

    def __getattr__(self, name):
        raise AssertionError(f"the model was touched ({name}) before the arguments were checked")


def test_view_semantics_averages_once_under_the_scene_name():
    """_ViewSemantics on the host: the views' scores are averaged when the last view is in and handed on once."""
    from geoformer_amd import batch_eval, postprocess

    class Inner:
        def __init__(self):
            self.got = []

        def add_batch(self, scores, labels, offsets, names, offsets_host=None):
            self.got.append((names, scores.clone(), labels.clone(), offsets_host.tolist()))

    rng = np.random.default_rng(5)
    s = [torch.from_numpy(rng.standard_normal((6, 3)).astype(F)) for _ in range(3)]
    lab = [torch.arange(6) + 10 * k for k in range(3)]
    inner = Inner()
    sem = batch_eval._ViewSemantics(inner, 3)
    V = batch_eval.ViewName
    off = torch.tensor([0, 6, 12], dtype=torch.int32)
    sem.add_batch(torch.cat([s[0], s[1]]), torch.cat([lab[0], lab[1]]), off, [V("x", 0), V("x", 1)], offsets_host=off)
    assert inner.got == []
    sem.add_batch(torch.cat([s[2], s[0]]), torch.cat([lab[2], lab[0]]), off, [V("x", 2), "plain"], offsets_host=off)
    assert [g[0] for g in inner.got] == [["x"], ["plain"]] and not sem.kept and not sem.labels
    assert torch.equal(inner.got[0][1], torch.from_numpy(postprocess.mean_views_host([x.numpy() for x in s])))
    assert torch.equal(inner.got[0][2], lab[0]) and inner.got[0][3] == [0, 6]  # view 0's labels
    assert torch.equal(inner.got[1][1], s[0])


def test_a_segments_mapping_serves_every_view_under_the_scene_name():
    from geoformer_amd import batch_eval
    from geoformer_amd.batch_eval import ViewName

    raw = np.zeros((5, 8), np.float32)
    items = [("a", raw), ("b", raw), ("c", raw)]
    ids = {"a": np.arange(5), "b": np.arange(5)[::-1].copy(), "elsewhere": np.zeros(3, np.int64)}
    out = batch_eval._view_segments(ids, items, 3)
    assert set(out) == {"a", "b", "elsewhere"} | {ViewName(n, k) for n in "ab" for k in range(3)}
    assert all(out[ViewName(n, k)] is ids[n] for n in "ab" for k in range(3)) and ViewName("c", 0) not in out
    assert set(ids) == {"a", "b", "elsewhere"}  # the caller's mapping is left as it was
    # collate_batches finds a view's ids under its ViewName, and gives -1 to the views of a scene without ids
    views = batch_eval.Views(rotations=3)
    chunks, batches = batch_eval.collate_batches(batch_eval.view_items(items, views), 3, segments=out)
    assert [b["segments"].tolist() for b in batches] == [[0, 1, 2, 3, 4] * 3, [4, 3, 2, 1, 0] * 3, [-1] * 15]
    geo = batch_eval.GeometricSegments()
    assert batch_eval._view_segments(geo, items, 3) is geo and batch_eval._view_segments("geometric", items, 3) == "geometric"
    assert batch_eval._view_segments(None, items, 3) is None


def test_the_caps_restated_in_python_are_the_library_s():
    from geoformer_amd import pointops, postprocess, view_merge

    assert view_merge.view_limits() == (view_merge.VIEW_MAX_ROWS, postprocess.VIEW_MAX_VIEWS) == (4096, 32)
    assert view_merge.VIEW_MAX_VIEWS is postprocess.VIEW_MAX_VIEWS
    assert view_merge.TILE_STITCH_MAX_CLASSES is pointops.TILE_STITCH_MAX_CLASSES
