"""GPU: geometric over-segmentation (csrc/oversegment.hip: pointops.point_normals, smooth_components, oversegment)
against the host statement postprocess.oversegment_host, and segments="geometric" in batch_eval.

The normals are compared with float64 to a derived bound; everything behind them is integer and compared exactly: the
components from synthetic rows, the rule from hand-made normals, and the rule on a scene from the kernel's OWN normals
once the host has shown that no decision lies within rounding of its threshold."""
import numpy as np
import pytest
import torch

from tests.oversegment_cases import RULE_CASES, UP, _rows
from tests.test_gpu_label_map import calibrated_model  # noqa: F401  (the small calibrated model and its four scenes)

pytestmark = pytest.mark.gpu

SCENE_SEED = 7  # the first seed of 7.. without an ambiguous decision under the kernel's normals (test 4's precondition)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def room(hip):
    """make_small_scene(8192, SCENE_SEED): xyz, spacing and the rule's keywords at that spacing."""
    from geoformer_amd import scene

    sc = scene.make_small_scene(8192, seed=SCENE_SEED)
    sp = float(sc["spacing"])
    return sc["xyz"].astype(np.float32), sp, dict(normal_deg=15.0, offset=0.5 * sp, flatness=0.01, min_points=8)


def _rows_gpu(xyz, k, radius):
    from geoformer_amd import pointops

    _, I, deg = pointops.knn_radius(_dev(xyz), k, radius, sqrt_out=False, check_overflow=True)
    return I, deg


# ---- 1. normals against float64 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,shift", [(16, 0.0), (3, 0.0), (64, 0.0), (16, 1000.0)])
def test_normals_against_float64(room, k, shift):
    """Valid points whose normal is determined ((l1 - l0) / l2 >= 0.1 in the arbiter): angle <= 1e-3 rad, |sigma -
    sigma_ref| <= 1e-4.  The fp32 sums of at most 64 difference products perturb C by about 2e-6 relative; over the gap
    of 0.1 that is 2e-5 rad and 4e-6 in sigma; the bounds leave a factor 25-50 for the Jacobi residual.  Invalid points
    agree exactly.  shift = 1000 m: the sums are formed from differences to the point, so nothing cancels."""
    from geoformer_amd import pointops, postprocess

    xyz0, sp, _ = room
    xyz = (xyz0 + np.float32(shift)).astype(np.float32)
    I, deg = _rows_gpu(xyz, k, 3 * sp)
    got = pointops.point_normals(_dev(xyz), I, deg)
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and got.shape == (xyz.shape[0], 4)
    got = got.cpu().numpy().astype(np.float64)
    ref, w = postprocess.point_normals_host(xyz, I.cpu().numpy(), deg.cpu().numpy(), return_eigenvalues=True)
    invalid = ref[:, 3] < 0
    assert np.array_equal(got[invalid], ref[invalid]) and not (got[~invalid, 3] < 0).any()
    sure = ~invalid & ((w[:, 1] - w[:, 0]) >= 0.1 * w[:, 2])
    assert sure.sum() > 0.5 * xyz.shape[0]  # (the comparison below is not an empty one)
    assert np.abs(np.linalg.norm(got[~invalid, :3], axis=1) - 1).max() <= 1e-6
    angle = np.arcsin(np.minimum(np.linalg.norm(np.cross(got[sure, :3], ref[sure, :3]), axis=1), 1.0))
    same_side = (got[sure, :3] * ref[sure, :3]).sum(axis=1) > 0
    # the sign rule may only decide differently where a component lies on different sides of its 1e-6 switch
    straddle = ((np.abs(got[sure, :3]) > 1e-6) != (np.abs(ref[sure, :3]) > 1e-6)).any(axis=1)
    d_sigma = np.abs(got[sure, 3] - ref[sure, 3])
    print(f"k={k} shift={shift}: {sure.sum()} of {xyz.shape[0]} points, invalid {invalid.sum()}, max angle "
          f"{angle.max():.3g} rad, max |d sigma| {d_sigma.max():.3g}, opposite sign {(~same_side).sum()}")
    assert angle.max() <= 1e-3 and d_sigma.max() <= 1e-4
    assert (same_side | straddle).all()


# ---- 2. components exactly, from synthetic rows ---------------------------------------------------------------------------
def _graphs():
    rng = np.random.default_rng(5)
    g = {}
    perm = rng.permutation(5000)
    rows = [None] * 5000
    for a, b in zip(perm[:-1], perm[1:]):
        rows[a] = [a, b]
    rows[perm[-1]] = [perm[-1]]
    g["path_shuffled"] = (rows, 8)
    g["star"] = ([[0] + list(range(1, 64))] + [[i, 0] for i in range(1, 400)], 8)
    clique = [list(range(10)) for _ in range(10)] + [list(range(10, 20)) for _ in range(10)]
    clique[3] = clique[3] + [14]  # 3 lists 14, 14 does not list 3
    g["cliques_one_way"] = (clique, 8)
    g["cliques_apart"] = ([list(r) for r in clique[:3]] + [list(range(10))] + [list(r) for r in clique[4:]], 8)
    g["padding_inside"] = ([[i, -1, (i + 1) % 40, -1, -1, (i + 7) % 40] for i in range(40)]
                           + [[i, -1, -1, -1, -1, -1] for i in range(40, 60)], 8)
    g["self_loops"] = ([[i, i, i, i + 1 if i % 10 != 9 else i] for i in range(50)], 8)
    n = 64
    g["out_of_range"] = ([[i, n + 5, (i + 1) % 32 if i < 32 else i, 2 ** 30, -7, n] for i in range(n)], 8)
    g["singletons_kept"] = ([[i] for i in range(3000)], 1)
    g["singletons_dissolved"] = ([[i] for i in range(3000)], 2)
    g["min_points_edge"] = ([[i, i + 1] for i in range(7)] + [[7]] + [[i, i + 1] for i in range(8, 14)] + [[14]], 8)
    return g


GRAPHS = _graphs()


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_components_from_synthetic_rows(hip, name):
    """All normals +z, sigma 0, every point on z = 0: every edge passes and the ids are the graph's components alone."""
    from geoformer_amd import pointops, postprocess

    lists, min_points = GRAPHS[name]
    n = len(lists)
    I, deg = _rows(lists)
    rng = np.random.default_rng(1)
    xyz = np.c_[rng.random((n, 2)), np.zeros(n)].astype(np.float32)
    n4 = np.tile(np.asarray(UP, np.float32), (n, 1))
    kw = dict(normal_deg=15.0, offset=0.012, flatness=0.01, min_points=min_points)
    want = postprocess.smooth_components_host(xyz, n4, I, deg, **kw)
    got = pointops.smooth_components(_dev(xyz), _dev(n4), _dev(I), _dev(deg), **kw)
    again = pointops.smooth_components(_dev(xyz), _dev(n4), _dev(I), _dev(deg), **kw)
    torch.cuda.synchronize()
    assert got.dtype == torch.int32 and got.cpu().numpy().tolist() == want.tolist()
    assert torch.equal(got, again)
    # what the statement gives for these graphs, so that the host is not the only witness
    sizes = {"path_shuffled": [5000], "star": [400], "cliques_one_way": [20], "cliques_apart": [10, 10],
             "padding_inside": [40], "self_loops": [10] * 5, "out_of_range": [32], "singletons_kept": [1] * 3000,
             "singletons_dissolved": [], "min_points_edge": [8]}[name]
    assert sorted(np.unique(want[want >= 0], return_counts=True)[1].tolist()) == sorted(sizes)


# ---- 3. the rule exactly, from hand-made normals --------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(RULE_CASES))
def test_rule_from_host_normals(hip, name):
    from geoformer_amd import pointops

    xyz, n4, I, deg, kw, want = RULE_CASES[name]()
    got = pointops.smooth_components(_dev(xyz), _dev(n4), _dev(I), _dev(deg), **kw)
    torch.cuda.synchronize()
    assert got.cpu().numpy().tolist() == want.tolist()


# ---- 4. the rule on a scene, from the kernel's own normals ------------------------------------------------------------------
def test_rule_on_scene_from_own_normals(room):
    """The kernel's normals4 go to both sides.  The host first shows that no edge or attach decision lies within 1e-5
    (dot product) or 1e-5 x radius (offsets) of its threshold -- the kernel's fp32 three-term products differ from
    float64 by about 2e-7 -- and then the ids are equal for every point."""
    from geoformer_amd import pointops, postprocess

    xyz, sp, kw = room
    I, deg = _rows_gpu(xyz, 16, 3 * sp)
    xd = _dev(xyz)
    n4 = pointops.point_normals(xd, I, deg)
    got = pointops.smooth_components(xd, n4, I, deg, **kw)
    torch.cuda.synchronize()
    want, ambiguous = postprocess.smooth_components_host(xyz, n4.cpu().numpy(), I.cpu().numpy(), deg.cpu().numpy(),
                                                         margins=(1e-5, 1e-5 * 3 * sp), **kw)
    print(f"seed {SCENE_SEED}: {ambiguous} ambiguous decisions, {len(np.unique(want[want >= 0]))} segments, "
          f"{(want < 0).mean():.3%} without one")
    assert ambiguous == 0
    assert 8 <= len(np.unique(want[want >= 0])) <= 16
    assert got.cpu().numpy().tolist() == want.tolist()


# ---- 5. end to end ----------------------------------------------------------------------------------------------------------
def _outside_majority(a, b):
    """Share of all points that lie in a segment of `a` but outside that segment's majority label of `b`."""
    in_a = a >= 0
    pairs, counts = np.unique(np.stack([a[in_a], b[in_a]]), axis=1, return_counts=True)
    best = {}
    for s, c in zip(pairs[0].tolist(), counts.tolist()):
        best[s] = max(best.get(s, 0), c)
    return (int(in_a.sum()) - sum(best.values())) / a.size


def test_end_to_end(room):
    """pointops.oversegment against the float64 statement on the same rows: at most 1 % of the points outside the
    majority match in either direction and at most 1 % difference in the share without a segment (the flatness decisions
    within 1e-4 of the threshold are the only ones fp32 normals can move); bit-identical from call to call."""
    from geoformer_amd import pointops, postprocess

    xyz, sp, kw = room
    xd = _dev(xyz)
    got, flag = pointops.oversegment(xd, k=16, radius=3 * sp, return_flag=True, **kw)
    again = pointops.oversegment(xd, k=16, radius=3 * sp, **kw)
    torch.cuda.synchronize()
    assert got.dtype == torch.int32 and got.shape == (xyz.shape[0],) and torch.equal(got, again)
    assert flag.dtype == torch.int32 and flag.tolist() == [0]
    I, deg = _rows_gpu(xyz, 16, 3 * sp)
    want = postprocess.oversegment_host(xyz, I.cpu().numpy(), deg.cpu().numpy(), radius=3 * sp, **kw)
    g = got.cpu().numpy()
    out_gw, out_wg = _outside_majority(g, want), _outside_majority(want, g)
    none = abs((g < 0).mean() - (want < 0).mean())
    print(f"outside the majority match: {out_gw:.4%} / {out_wg:.4%}; without a segment: {(g < 0).mean():.3%} vs "
          f"{(want < 0).mean():.3%}; {len(np.unique(g[g >= 0]))} vs {len(np.unique(want[want >= 0]))} segments")
    assert out_gw <= 0.01 and out_wg <= 0.01 and none <= 0.01


# ---- 6. arguments -------------------------------------------------------------------------------------------------------------
def test_arguments(hip):
    from geoformer_amd import _lib, pointops

    xyz, n4, I, deg, kw, _ = RULE_CASES["crease_14deg"]()
    x, nn, i, d = _dev(xyz), _dev(n4), _dev(I), _dev(deg)
    for bad in ((x.double(), i, d), (x, i.long(), d), (x, i, d.long()), (x.cpu(), i, d), (x[:, :2].contiguous(), i, d),
                (x, i, d[:-1].contiguous())):
        with pytest.raises(RuntimeError):
            pointops.point_normals(*bad)
    with pytest.raises(RuntimeError):
        pointops.smooth_components(x, nn.double(), i, d, **kw)
    with pytest.raises(RuntimeError):
        pointops.smooth_components(x, nn[:, :3].contiguous(), i, d, **kw)
    with pytest.raises(RuntimeError):
        pointops.smooth_components(x, nn, i, d, **dict(kw, min_points=0))
    with pytest.raises(RuntimeError):
        pointops.oversegment(x, min_points=0)
    with pytest.raises(RuntimeError):
        pointops.oversegment(x.double())
    # the library's own checks, before any launch
    inval, st = -1, _lib.stream_ptr()  # GF_ERR_INVALID_ARG
    ids = torch.empty(50, dtype=torch.int32, device="cuda")
    ws = torch.empty(hip.gf_smooth_components_scratch_bytes(50) // 4 + 1, dtype=torch.int32, device="cuda")
    P = lambda t: t.data_ptr()  # noqa: E731
    sc = lambda n, k, mp, xyz_p=P(x): hip.gf_smooth_components(xyz_p, P(nn), P(i), P(d), n, k, 0.9659, 0.012, 0.01, mp,  # noqa: E731
                                                              P(ids), P(ws), st)
    assert sc(50, I.shape[1], 0) == inval and sc(-1, I.shape[1], 8) == inval and sc(50, 0, 8) == inval
    assert sc(50, I.shape[1], 8, None) == inval
    assert sc(50, I.shape[1], 8) == 0
    assert hip.gf_smooth_components(None, None, None, None, 0, 4, 0.9, 0.01, 0.01, 8, None, None, st) == 0  # n = 0
    out = torch.empty((50, 4), dtype=torch.float32, device="cuda")
    assert hip.gf_point_normals(P(x), P(i), P(d), -1, 4, P(out), st) == inval
    assert hip.gf_point_normals(P(x), P(i), P(d), 50, 0, P(out), st) == inval
    assert hip.gf_point_normals(P(x), None, P(d), 50, 4, P(out), st) == inval
    assert hip.gf_point_normals(None, None, None, 0, 4, None, st) == 0
    assert hip.gf_point_normals_scratch_bytes(1000) == 0
    # n = 0 through the wrappers: empty results
    e = x[:0].contiguous()
    assert pointops.oversegment(e).shape == (0,) and pointops.oversegment(e).dtype == torch.int32
    assert pointops.point_normals(e, i[:0].contiguous(), d[:0].contiguous()).shape == (0, 4)
    assert pointops.smooth_components(e, nn[:0].contiguous(), i[:0].contiguous(), d[:0].contiguous()).shape == (0,)
    torch.cuda.synchronize()


# ---- 7. wiring ----------------------------------------------------------------------------------------------------------------
def test_predict_batches_geometric(calibrated_model):  # noqa: F811
    from geoformer_amd import batch_eval, pointops

    model, items = calibrated_model
    items = items[:2]
    shape = np.max([b["spatial_shape"] for b in batch_eval.collate_batches(items, 2)[1]], axis=0)
    kw = dict(spatial_shape=shape, reserve=False, final_score_thresh=0.0)
    seen = []

    def tap(_module, args, kwargs):
        b = args[0]
        seen.append((b.get("segments"), b["locs_float"], b["offsets"].cpu().tolist()))

    def run(**more):
        seen.clear()
        np.random.seed(21)
        out = list(batch_eval.predict_batches(model, items, 2, **kw, **more))
        torch.cuda.synchronize()
        return out

    handle = model.register_forward_pre_hook(tap, with_kwargs=True)
    try:
        tuned = batch_eval.GeometricSegments(radius=0.12, offset=0.02)
        for arg, params in (("geometric", {}), (tuned, dict(radius=0.12, offset=0.02))):
            geo = run(segments=arg)
            (seg, locs, off), = seen
            assert seg.dtype == torch.int32 and seg.is_cuda and seg.shape == (off[-1],)
            for b in range(2):  # scene-local ids: what the scene gets alone
                alone = pointops.oversegment(locs[off[b]:off[b + 1]].contiguous(), **params)
                assert torch.equal(seg[off[b]:off[b + 1]], alone)
        n_seg = len(torch.unique(seg[seg >= 0]))
        assert n_seg >= 4 and float((seg >= 0).float().mean()) > 0.5
        none = run(segments=None)
        assert seen[0][0] is None
        parent = run()  # the call as it was before the keyword could name a GeometricSegments
    finally:
        handle.remove()
    assert [n for n, *_ in geo] == [n for n, *_ in none] == [n for n, _ in items]
    differ = 0
    for (_, c0, s0, m0, p0), (_, c1, s1, m1, p1), (_, cg, sg, mg, pg) in zip(none, parent, geo):
        assert torch.is_tensor(c0) == torch.is_tensor(c1)
        if torch.is_tensor(c0):
            assert torch.equal(c0, c1) and torch.equal(s0, s1) and torch.equal(m0, m1) and torch.equal(p0, p1)
            differ += int(not (torch.is_tensor(mg) and mg.shape == m0.shape and torch.equal(mg, m0)))
    assert differ > 0  # the pooling changed at least one scene's masks
