"""GPU: picked masks split into connected clusters (csrc/mask_split.hip: pointops.mask_components, mask_keep_largest,
dbscan; postprocess.split_masks; split= in batch_eval) against the host statement postprocess.mask_components_host.
Every comparison is integer and exact."""
import numpy as np
import pytest
import torch

from tests.mask_split_cases import (GRAPHS, HAND_CASES, LATTICE_EPS, LATTICE_K, graph_inputs, lattice_cloud, ring_inputs,
                                    sklearn_ids)
from tests.test_gpu_label_map import calibrated_model  # noqa: F401  (the small calibrated model and its four scenes)

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _check(masks, pick, I, deg, min_samples, min_points, alone=True):
    """mask_components and mask_keep_largest against the statement; two calls bit-identical; each pick alone equals its
    row of the batched call.  Returns the statement's (comp, tab)."""
    from geoformer_amd import pointops, postprocess

    want_c, want_t = postprocess.mask_components_host(masks, pick, I, deg, min_samples, min_points)
    m, pk, Id, dd = _dev(masks), _dev(pick), _dev(I), _dev(deg)
    comp, tab = pointops.mask_components(m, pk, Id, dd, min_samples, min_points)
    comp2, tab2 = pointops.mask_components(m, pk, Id, dd, min_samples, min_points)
    out = pointops.mask_keep_largest(m, pk, comp, tab)
    singles = [pointops.mask_components(m, pk[r:r + 1].contiguous(), Id, dd, min_samples, min_points)
               for r in range(len(pick))] if alone else []
    torch.cuda.synchronize()
    assert comp.dtype == torch.int32 and comp.shape == want_c.shape and tab.dtype == torch.int32
    assert np.array_equal(tab.cpu().numpy(), want_t)
    assert np.array_equal(comp.cpu().numpy(), want_c)
    assert torch.equal(comp, comp2) and torch.equal(tab, tab2)
    for r, (c1, t1) in enumerate(singles):
        assert torch.equal(c1[0], comp[r]) and torch.equal(t1[0], tab[r])
    want_o = postprocess.mask_keep_largest_host(masks, pick, want_c, want_t)
    assert out.dtype == torch.int32 and np.array_equal(out.cpu().numpy(), want_o)
    unpicked = np.setdiff1d(np.arange(masks.shape[0]), pick)
    assert np.array_equal(want_o[unpicked], masks[unpicked])  # (the statement itself: rows nobody picked are the input's)
    return want_c, want_t


# ---- 1. synthetic rows under three masks at once ----------------------------------------------------------------------------
@pytest.mark.parametrize("min_samples", [1, 2])
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_components_from_synthetic_rows(hip, name, min_samples):
    masks, pick, I, deg = graph_inputs(name)
    want_c, want_t = _check(masks, pick, I, deg, min_samples, 1)
    if min_samples == 1:
        # what the statement gives for these graphs under mask 0 (all points) and mask 2 (all but the articulation
        # point), so that the host is not the only witness: the mask restriction decides the answer
        sizes = {"path_shuffled": ([5000], [2500, 2499]), "star": ([400], [1] * 399), "cliques_one_way": ([20], [9, 10]),
                 "padding_inside": ([40] + [1] * 20, [39] + [1] * 20), "self_loops": ([10] * 5, [4, 5] + [10] * 4),
                 "out_of_range": ([32] + [1] * 32, [31] + [1] * 32)}[name]
        for row, want in zip((0, 2), sizes):
            got = np.unique(want_c[row][want_c[row] >= 0], return_counts=True)[1]
            assert sorted(got.tolist()) == sorted(want)
        assert want_t[1, 0] == masks[1].sum() and 0 < want_t[1, 0] < masks.shape[1]


# ---- 2. shapes: points around the 64-point word, picks across a wave ----------------------------------------------------------
@pytest.mark.parametrize("density", [0.02, 0.6])
@pytest.mark.parametrize("p", [1, 3, 70])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4099])
def test_shapes(hip, n, p, density):
    """A ring under random masks, min_samples = 3 (a core point has both neighbours in the mask, a border point one)
    and min_points = 2."""
    masks, pick, I, deg = ring_inputs(n, p, density, seed=n * 100 + p)
    _check(masks, pick, I, deg, 3, 2, alone=p <= 3)
    if p == 70:  # picks in another order, one row twice, one out of range: rows follow their picks
        pick2 = np.r_[pick[::-1][:40], 5, 5, 70, -3].astype(np.int64)
        _check(masks, pick2, I, deg, 1, 1, alone=False)


# ---- 3. the hand cases ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(HAND_CASES))
def test_hand_cases(hip, name):
    from geoformer_amd import pointops

    c = HAND_CASES[name]()
    comp, tab = pointops.mask_components(_dev(c["masks"]), _dev(c["pick"]), _dev(c["I"]), _dev(c["deg"]),
                                         c["min_samples"], c["min_points"])
    torch.cuda.synchronize()
    assert comp.cpu().numpy().tolist() == c["comp"].tolist() and tab.cpu().numpy().tolist() == c["tab"].tolist()
    _check(c["masks"], c["pick"], c["I"], c["deg"], c["min_samples"], c["min_points"])


# ---- 4. end to end through knn_radius: sklearn's DBSCAN ----------------------------------------------------------------------
@pytest.mark.parametrize("min_samples", [1, 3, 5])
def test_dbscan_is_sklearn(hip, min_samples):
    from geoformer_amd import pointops

    xyz, member = lattice_cloud(3, keep=0.25)
    xd = _dev(xyz)
    _, I, deg = pointops.knn_radius(xd, LATTICE_K, LATTICE_EPS, sqrt_out=False, check_overflow=True)
    assert int(deg.max()) < LATTICE_K - 1  # every in-radius neighbour is in its row
    got, flag = pointops.dbscan(xd, LATTICE_EPS, min_samples=min_samples, k=LATTICE_K, return_flag=True)
    torch.cuda.synchronize()
    want = sklearn_ids(xyz, np.ones(len(xyz), bool), LATTICE_EPS, min_samples)
    assert got.dtype == torch.int32 and flag.tolist() == [0]
    assert got.cpu().numpy().tolist() == want.tolist()
    assert len(np.unique(want[want >= 0])) >= 2 and (min_samples == 1 or (want < 0).any())
    # one mask over the same rows: the member points alone
    comp, _ = pointops.mask_components(_dev(member.astype(np.int32)[None]), torch.zeros(1, dtype=torch.int64, device="cuda"),
                                       I, deg, min_samples, 1)
    assert comp[0].cpu().numpy().tolist() == sklearn_ids(xyz, member, LATTICE_EPS, min_samples).tolist()
    big = pointops.dbscan(xd, LATTICE_EPS, min_samples=min_samples, k=LATTICE_K, min_points=20).cpu().numpy()
    ids, size = np.unique(want[want >= 0], return_counts=True)
    assert big.tolist() == np.where(np.isin(want, ids[size >= 20]), want, -1).tolist()


# ---- 5. split_masks on a scene ------------------------------------------------------------------------------------------------
def test_split_masks_on_scene(hip):
    """A mask of two slabs of the room more than `radius` apart plus 20 stray points between them: "split" gives the two
    slabs, "largest" the bigger one, and with min_points = 50 the strays are gone in both modes."""
    from geoformer_amd import postprocess, scene

    sc = scene.make_small_scene(8192, seed=7)
    xyz = sc["xyz"].astype(np.float32)
    radius = 3 * float(sc["spacing"])
    x = xyz[:, 0]
    q = np.quantile(x, [0.2, 0.45, 0.55, 0.75])
    assert q[1] - q[0] > 2 * radius and q[3] - q[2] > 2 * radius
    a, b = x < q[0], x > q[3]
    stray = np.random.default_rng(3).choice(np.nonzero((x > q[1]) & (x < q[2]))[0], 20, replace=False)
    masks = np.zeros((3, len(xyz)), np.int32)
    masks[1, a | b] = 1
    masks[1, stray] = 1
    masks[2, ::3] = 1  # a proposal the NMS did not pick
    scores, cls = torch.tensor([0.3, 0.9, 0.5]).cuda(), torch.tensor([4, 7, 9]).cuda()
    pick = torch.tensor([1, 0]).cuda()
    kw = dict(radius=radius, k=16, min_samples=1, min_points=50)
    host = postprocess.split_masks(torch.from_numpy(masks), scores.cpu(), cls.cpu(), pick.cpu(), torch.from_numpy(xyz),
                                   mode="split", **kw)
    for mode in ("largest", "split"):
        c, s, m, p = postprocess.split_masks(_dev(masks), scores, cls, pick, _dev(xyz), mode=mode, **kw)
        torch.cuda.synchronize()
        m = m.cpu().numpy()
        if mode == "largest":
            assert c is cls and s is scores and torch.equal(p, pick) and m.shape == masks.shape
            assert np.array_equal(m[1], b.astype(np.int32)) and b.sum() > a.sum()
            assert np.array_equal(m[2], masks[2]) and not m[0].any()
        else:
            assert m.shape == (2, len(xyz)) and p.tolist() == [0, 1] and c.tolist() == [7, 7] and s.tolist() == [scores[1].item()] * 2
            lo, hi = sorted((int(np.argmax(a)), int(np.argmax(b))))  # by cluster id: the cluster's smallest point
            assert np.array_equal(m[0], (a if a[lo] else b).astype(np.int32))
            assert np.array_equal(m[1], (a if a[hi] else b).astype(np.int32))
            assert np.array_equal(m, host[2].numpy()) and host[0].tolist() == [7, 7]
        assert not m[:2][:, stray].any()  # (in both modes the first two rows are the picked mask's)
    # min_points = 1: the strays come back as clusters of their own
    _, _, m1, _ = postprocess.split_masks(_dev(masks), scores, cls, pick, _dev(xyz), mode="split", **dict(kw, min_points=1))
    assert m1.shape[0] > 2 and int(m1[:, stray].sum()) == 20


# ---- 6. arguments ---------------------------------------------------------------------------------------------------------------
def test_arguments(hip):
    from geoformer_amd import _lib, pointops

    masks, pick, I, deg = ring_inputs(100, 3, 0.6)
    m, pk, Id, dd = _dev(masks), _dev(pick), _dev(I), _dev(deg)
    comp, tab = pointops.mask_components(m, pk, Id, dd)
    for bad in ((m.long(), pk, Id, dd), (m, pk.int(), Id, dd), (m, pk, Id.long(), dd), (m, pk, Id, dd.long()),
                (m.cpu(), pk, Id, dd), (m, pk.cpu(), Id, dd), (m[:, ::2], pk, Id, dd), (m[0], pk, Id, dd),
                (m, pk, Id[:-1].contiguous(), dd), (m, pk, Id, dd[:-1].contiguous()),
                (m, torch.zeros(1025, dtype=torch.int64, device="cuda"), Id, dd)):
        with pytest.raises(RuntimeError):
            pointops.mask_components(*bad)
    for kw in (dict(min_samples=0), dict(min_points=0)):
        with pytest.raises(RuntimeError):
            pointops.mask_components(m, pk, Id, dd, **kw)
    for bad in ((m, pk, comp[:2].contiguous(), tab), (m, pk, comp, tab[:, :4].contiguous()), (m, pk, comp.long(), tab),
                (m, pk.int(), comp, tab), (m.cpu(), pk, comp, tab)):
        with pytest.raises(RuntimeError):
            pointops.mask_keep_largest(*bad)
    with pytest.raises(RuntimeError):
        pointops.dbscan(torch.zeros((10, 3), dtype=torch.float64, device="cuda"), 0.1)
    with pytest.raises(RuntimeError):
        pointops.dbscan(torch.zeros((10, 3), device="cuda"), 0.1, min_points=0)
    # the library's own checks, before any launch: the outputs keep their marker
    inval, st = -1, _lib.stream_ptr()  # GF_ERR_INVALID_ARG
    P = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    n, p, k = 100, 3, I.shape[1]
    ws = torch.empty(hip.gf_mask_components_scratch_bytes(n, p) // 8 + 1, dtype=torch.int64, device="cuda")
    assert hip.gf_mask_components_scratch_bytes(0, 3) == 0 and hip.gf_mask_components_scratch_bytes(100, 0) == 0
    assert hip.gf_mask_components_scratch_bytes(n, p) >= 2 * p * 2 * 8 + p * n * 4
    mark_c, mark_t = torch.full_like(comp, 77), torch.full_like(tab, 77)
    ptrs = dict(masks=m, pick=pk, I=Id, deg=dd, comp=mark_c, tab=mark_t, ws=ws)

    def mc(n=n, p=p, k=k, ms=1, mp=1, **null):
        a = {key: (None if key in null else t) for key, t in ptrs.items()}
        return hip.gf_mask_components(P(a["masks"]), 3, n, P(a["pick"]), p, P(a["I"]), P(a["deg"]), k, ms, mp,
                                      P(a["comp"]), P(a["tab"]), P(a["ws"]), st)

    assert mc(n=-1) == inval and mc(p=-1) == inval and mc(p=1025) == inval and mc(k=0) == inval
    assert mc(ms=0) == inval and mc(mp=0) == inval
    for key in ptrs:
        assert mc(**{key: True}) == inval
    torch.cuda.synchronize()
    assert bool((mark_c == 77).all()) and bool((mark_t == 77).all())
    assert mc(n=0) == 0 and mc(p=0) == 0
    assert hip.gf_mask_components(None, 0, 0, None, 0, None, None, 1, 1, 1, None, None, None, st) == 0
    torch.cuda.synchronize()
    assert bool((mark_c == 77).all()) and bool((mark_t == 77).all())  # nothing launched
    assert mc() == 0
    torch.cuda.synchronize()
    assert torch.equal(mark_c, comp) and torch.equal(mark_t, tab)
    out = torch.full_like(m, 77)

    def kl(n_rows=3, n=n, p=p, masks=m, pick=pk, comp=comp, tab=tab, out=out):
        return hip.gf_mask_keep_largest(P(masks), n_rows, n, P(pick), p, P(comp), P(tab), P(out), st)

    assert kl(n=-1) == inval and kl(p=-1) == inval and kl(p=1025) == inval and kl(n_rows=-1) == inval
    assert kl(masks=None) == inval and kl(pick=None) == inval and kl(comp=None) == inval and kl(tab=None) == inval
    assert kl(out=None) == inval
    assert kl(n=0) == 0 and kl(p=0) == 0
    torch.cuda.synchronize()
    assert bool((out == 77).all())
    assert kl() == 0
    torch.cuda.synchronize()
    assert torch.equal(out, pointops.mask_keep_largest(m, pk, comp, tab))
    # empty shapes through the wrappers
    c0, t0 = pointops.mask_components(m, pk[:0].contiguous(), Id, dd)
    assert c0.shape == (0, n) and t0.shape == (0, 5)
    assert torch.equal(pointops.mask_keep_largest(m, pk[:0].contiguous(), c0, t0), m)
    e = torch.zeros((3, 0), dtype=torch.int32, device="cuda")
    c0, t0 = pointops.mask_components(e, pk, Id[:0].contiguous(), dd[:0].contiguous())
    assert c0.shape == (3, 0) and t0.shape == (3, 5)
    assert pointops.dbscan(torch.zeros((0, 3), device="cuda"), 0.1).shape == (0,)
    torch.cuda.synchronize()


# ---- 7. wiring ------------------------------------------------------------------------------------------------------------------
def test_predict_batches_split(calibrated_model):  # noqa: F811
    from geoformer_amd import batch_eval, postprocess

    model, items = calibrated_model
    items = items[:2]
    shape = np.max([b["spatial_shape"] for b in batch_eval.collate_batches(items, 2)[1]], axis=0)
    kw = dict(spatial_shape=shape, reserve=False, final_score_thresh=0.0)
    locs = []

    def tap(_module, args, kwargs):
        b = args[0]
        off = b["offsets"].cpu().tolist()
        locs.extend(b["locs_float"][off[i]:off[i + 1]].contiguous() for i in range(len(off) - 1))

    def run(**more):
        locs.clear()
        np.random.seed(21)
        out = list(batch_eval.predict_batches(model, items, 2, **kw, **more))
        torch.cuda.synchronize()
        return out

    handle = model.register_forward_pre_hook(tap, with_kwargs=True)
    try:
        parent = run()  # the call as it was before the keyword
        none = run(split=None)
        largest = run(split="largest")
        tuned = run(split=batch_eval.MaskSplit(radius=0.15, min_points=20, mode="largest"))
        split = run(split="split")
    finally:
        handle.remove()
    changed = picked = rows = 0
    for b, ((n0, c0, s0, m0, p0), (n1, c1, s1, m1, p1), (n2, c2, s2, m2, p2), (_, _, _, m3, _), (n4, c4, s4, m4, p4)) in \
            enumerate(zip(parent, none, largest, tuned, split)):
        assert n0 == n1 == n2 == n4 == items[b][0]
        assert torch.is_tensor(c0) == torch.is_tensor(c1) == torch.is_tensor(c2) == torch.is_tensor(c4)
        if not torch.is_tensor(c0):
            continue
        assert torch.equal(c0, c1) and torch.equal(s0, s1) and torch.equal(m0, m1) and torch.equal(p0, p1)
        assert torch.equal(c0, c2) and torch.equal(s0, s2) and torch.equal(p0, p2) and m2.shape == m0.shape
        assert m2.dtype == torch.int32 and not bool(((m2 != 0) & (m0 == 0)).any())  # a subset of the original
        rest = torch.ones(m0.shape[0], dtype=torch.bool, device=m0.device)
        rest[p0] = False
        assert torch.equal(m2[rest], m0[rest].int())
        direct = postprocess.split_masks(m0, s0, c0, p0, locs[b], mode="largest")
        assert torch.equal(direct[2], m2)
        direct = postprocess.split_masks(m0, s0, c0, p0, locs[b], radius=0.15, min_points=20, mode="largest")
        assert torch.equal(direct[2], m3)
        picked += int(p0.numel())
        changed += int((m2[p0] != m0[p0]).any(dim=1).sum())
        assert torch.equal(p4, torch.arange(m4.shape[0], device=p4.device)) and p4.dtype == torch.int64
        assert c4.shape == s4.shape == (m4.shape[0],) and m4.shape[1] == m0.shape[1]
        direct = postprocess.split_masks(m0, s0, c0, p0, locs[b], mode="split")
        assert torch.equal(direct[2], m4) and torch.equal(direct[0], c4) and torch.equal(direct[1], s4)
        rows += m4.shape[0]
    print(f"split='largest' changed {changed} of {picked} picked masks; split='split' made {rows} rows of them")
    assert picked > 0
