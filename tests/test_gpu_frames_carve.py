"""csrc/frames_carve.hip on the GPU: frames.visibility and frames.Carver bit for bit against the host statement -- the
call's Visibility, codes, state() and keep() after EVERY observe -- each case from a fresh object once per launch shape;
Fuser.snapshot / kept with keep= against FuserHost.  The inputs and what each size straddles are named in
tests/frames_carve_cases.py."""
import numpy as np
import pytest
import torch

from geoformer_amd import frames
from tests import frames_cases as fc
from tests import frames_carve_cases as cc
from tests import frames_stream_cases as sc

pytestmark = pytest.mark.gpu

VARIANTS = (0, 1, None)


def _vis(xyz, fr, **kw):
    """frames.visibility with codes in every launch shape against the statement; returns the statement's codes."""
    want, want_codes = frames.visibility_host(xyz, fr, codes=True, **kw)
    x = torch.from_numpy(np.array(xyz)).cuda()
    for variant in VARIANTS:
        got, codes = frames.visibility(x, fr, codes=True, variant=variant, **kw)
        assert all(t.is_cuda for t in got) and codes.is_cuda
        assert cc.same(codes, want_codes), (variant, int((cc.h(codes) != want_codes).sum()))
        assert cc.same_vis(got, want), variant
        assert cc.same_vis(frames.visibility(x, fr, variant=variant, **kw), want)     # without codes
    return want_codes


def _carve(steps, fuser_kw=None, **kw):
    """A sequence of ("add", Frames) / ("observe", Frames) / ("points", xyz) steps on a FuserHost with a CarverHost and,
    per launch shape, on a fresh Fuser with a fresh Carver: Visibility, state() and keep() equal after every observe.
    Returns (the CarverHost, the Carvers)."""
    fuser_kw = fuser_kw or {}
    fh = frames.FuserHost(**fuser_kw)
    ch, want = frames.CarverHost(fh, **kw), []
    for what, arg in steps:
        if what == "add":
            fh.add(arg)
        elif what == "points":
            fh.add_points(arg)
        else:
            want.append((ch.observe(arg), ch.state(), ch.keep(), ch.keep(0), fh.cells))
    carvers = []
    for variant in VARIANTS:
        fu = frames.Fuser(**fuser_kw)
        ca, k = frames.Carver(fu, variant=variant, **kw), 0
        for what, arg in steps:
            if what == "add":
                fu.add(arg)
            elif what == "points":
                fu.add_points(arg)
            else:
                vis = ca.observe(arg)
                vis_w, state_w, keep_w, keep0_w, cells_w = want[k]
                assert all(t.is_cuda for t in vis) and cc.same_vis(vis, vis_w), (variant, k)
                assert all(cc.same(a, b) for a, b in zip(ca.state(), state_w)), (variant, k)
                assert ca.keep().is_cuda and cc.same(ca.keep(), keep_w) and cc.same(ca.keep(0), keep0_w)
                assert ca.cells == fu.cells == cells_w
                k += 1
        carvers.append(ca)
    return ch, carvers


def test_limits_are_the_modules(hip):
    assert frames.carve_limits() == (cc.STAGE, cc.THREADS, frames.MAX_POINTS, 2)
    assert frames.CARVE_VARIANT in (0, 1)
    with pytest.raises(ValueError, match="variant"):
        frames.visibility(torch.zeros((1, 3), device="cuda"), cc.boundary_frames(), variant=2)


@pytest.mark.parametrize("n", cc.SIZES)
def test_sizes_around_a_wave_and_a_workgroup(hip, n):
    codes = _vis(cc.narrow_points()[:n], fc.make(fc.narrow()), edge=cc.EDGE)
    assert codes.shape == (3, n) and (n < cc.WAVE - 1 or (codes == cc.SEEN).any())


@pytest.mark.parametrize("kind", ["u16", "f32"])
@pytest.mark.parametrize("edge", [None, cc.EDGE])
def test_narrow_and_dense_frames(hip, kind, edge):
    _vis(cc.narrow_points(), fc.make(fc.narrow(), kind), edge=edge)
    fr = sc.dense4(kind)
    codes = _vis(frames.fuse_host(fr, cell=cc.CELL).xyz.numpy(), fr, edge=edge, band=cc.BAND)
    assert codes.shape[1] > 5000 and {cc.OUTSIDE, cc.UNKNOWN, cc.OCCLUDED, cc.SEEN, cc.FREE} == set(np.unique(codes))


@pytest.mark.parametrize("F", [1, cc.STAGE, cc.STAGE + 1])
def test_frames_around_one_round_of_staged_records(hip, F):
    fr = cc.many_frames(max(F, 3))
    fr = sc.sub(fr, 0, F)
    codes = _vis(cc.narrow_points(), fr, edge=cc.EDGE)
    assert codes.shape[0] == F and (codes[F - 1] == cc.SEEN).any()


@pytest.mark.parametrize("edge", [None, cc.EDGE])
def test_nasty_depths_and_gaps(hip, edge):
    pts = frames.fuse_host(sc.dense4("f32"), cell=cc.CELL).xyz.numpy()
    codes = _vis(pts, sc.nasty3(), edge=edge)
    assert (codes == cc.UNKNOWN).sum() > 1000
    codes = _vis(pts, sc.gaps3(), edge=edge)
    assert not (codes[1] > cc.UNKNOWN).any() and (codes[2] == cc.FREE).any()      # frame 1 has no valid pixel


def test_every_boundary_of_the_rule(hip):
    codes = _vis(cc.boundary_points(), cc.boundary_frames(), near=cc.B_NEAR, far=cc.B_FAR, band=cc.B_BAND, rel=cc.B_REL)
    assert cc.same(codes, cc.boundary_codes())


def test_a_sheared_pose(hip):
    fr = cc.sheared(sc.dense4())
    pts = frames.fuse_host(fr, cell=cc.CELL).xyz.numpy()
    codes = _vis(pts, fr, edge=cc.EDGE, band=cc.BAND)
    assert (codes == cc.SEEN).sum() > pts.shape[0]


def test_random_points_diverge(hip):
    codes = _vis(cc.scene_random_points(), sc.dense4(), edge=cc.EDGE)
    share = np.bincount(codes.reshape(-1), minlength=5) / codes.size
    assert (share > 0.02).all() and share.max() < 0.5      # every class among the lanes of a wave, none the rule


def test_frames_on_another_device_than_the_points(hip):
    fr = sc.dense4()
    on = frames.Frames(fr.depth.cuda(), None, fr.table, fr.depth_shift)
    pts = cc.narrow_points()
    want = frames.visibility_host(pts, fr)
    assert cc.same_vis(frames.visibility(torch.from_numpy(np.array(pts)).cuda(), on), want)


# ---- Carver -------------------------------------------------------------------------------------------------------------
def test_the_map_grows_between_two_observes(hip):
    parts = sc.chunks(sc.dense4(), (1, 3))
    ch, carvers = _carve([("add", parts[0]), ("observe", parts[0]), ("add", parts[1]), ("observe", parts[1]),
                          ("observe", sc.dense4("f32"))], dict(cell=cc.CELL, edge=cc.EDGE))
    assert ch.cells > 4 * cc.FIRST_ROWS and all(c.row_growths >= 2 for c in carvers)


def test_the_box_leaves(hip):
    with_box, without, _ = cc.box_gone()
    ch, _ = _carve([("add", with_box), ("observe", with_box), ("observe", without), ("observe", without)],
                   dict(cell=cc.CELL, edge=cc.EDGE))
    assert 1000 < int((~ch.keep().numpy()).sum()) < ch.cells // 2


@pytest.mark.parametrize("kw", [dict(), dict(hit=2, miss=3, floor=-7, ceil=5), dict(hit=0, miss=5, floor=-3, ceil=0)])
def test_the_clamp_saturates(hip, kw):
    fuser_kw = dict(cell=1.0, near=cc.B_NEAR, origin=(-8, -8, -8))
    pts = np.array([[0, 0, 2], [0.5, 0.25, 1.5], [0, 0, 3.5]], np.float32)
    far_depth = frames.make(np.full((1, cc.B_H, cc.B_W), 4.0, np.float32), [4.0, 4.0, 4.0, 2.0], np.eye(4)[None], None, 1.0)
    fr = cc.boundary_frames()
    steps = [("points", pts)] + [("observe", fr)] * 10 + [("observe", frames.concat([fr, far_depth, far_depth]))] + \
            [("points", np.array([[-0.5, 0.25, 1.0], [3, 3, 3]], np.float32)), ("observe", fr)]
    ch, _ = _carve(steps, fuser_kw, band=cc.B_BAND, rel=cc.B_REL, **kw)
    hit, miss, floor, ceil = kw.get("hit", 1), kw.get("miss", 1), kw.get("floor", -8), kw.get("ceil", 8)
    assert ch.state()[2][1] == floor and ch.state()[0].tolist() == [12, 0, 0, 0, 0]
    score = 0
    for step in [hit] * 10 + [hit - 2 * miss, hit]:       # cell 0: seen ten times, then seen once and looked through twice
        score = min(ceil, max(floor, score + step))
    assert ch.state()[2][0] == score


def test_counts_saturate(hip):
    fu = frames.Fuser(cell=1.0, near=cc.B_NEAR, origin=(-8, -8, -8))
    fu.add_points(np.array([[0, 0, 2], [0.5, 0.25, 1.5], [0, 0, 3.5]], np.float32))
    fr = cc.boundary_frames()
    for variant in (0, 1):
        ca = frames.Carver(fu, band=cc.B_BAND, rel=cc.B_REL, variant=variant)
        ca.observe(fr)
        ca._seen[0] = ca._free[1] = 2 ** 31 - 2
        for _ in range(2):
            ca.observe(fr)
            assert ca.state()[0].tolist() == [2 ** 31 - 1, 0, 0] and ca.state()[1].tolist() == [0, 2 ** 31 - 1, 0]


def test_a_failed_observe_leaves_the_state(hip):
    fu = frames.Fuser(cell=cc.CELL)
    ca = frames.Carver(fu)
    with pytest.raises(ValueError, match="empty"):
        ca.observe(sc.narrow3())
    fu.add(sc.narrow3())
    ca.observe(sc.narrow3())
    before = ca.state()
    fr = sc.narrow3()
    flat = fr.table.copy()
    flat[:, 4:] = 0
    for bad in (fr.depth, None, frames.Frames(fr.depth, None, flat, fr.depth_shift)):
        with pytest.raises(ValueError):
            ca.observe(bad)
        assert all(cc.same(a, b) for a, b in zip(ca.state(), before))


# ---- keep= downstream ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_obs", [1, 3])
def test_snapshot_and_kept_with_keep(hip, min_obs):
    fh, fu, cells = frames.FuserHost(cell=sc.COARSE), frames.Fuser(cell=sc.COARSE), []
    for part in sc.chunks(sc.dense4(), (2, 2)):
        cells.append(fh.add(part))
        assert cc.same(fu.add(part), cells[-1])
    cells, M = torch.cat(cells), fh.cells
    base = fu.snapshot(min_obs, cells.cuda())
    for mask in (np.ones(M, bool), np.zeros(M, bool), np.random.default_rng(7).random(M) < 0.6):
        want = fh.snapshot(min_obs, cells, keep=mask)
        for keep in (mask, torch.from_numpy(mask).cuda(), mask.astype(np.uint8)):
            got = fu.snapshot(min_obs, cells.cuda(), keep=keep)
            assert all(t.is_cuda for t in got) and sc.same_fused(got, want)
            assert cc.same(fu.kept(min_obs, keep), fh.kept(min_obs, mask)) and fu.kept(min_obs, keep).is_cuda
        if mask.all():
            assert sc.same_fused(fu.snapshot(min_obs, cells.cuda(), keep=mask), base)
    assert sc.same_fused(fu.snapshot(min_obs, cells.cuda()), base) and sc.same_state(fu, fh)   # the map itself is untouched
    for bad in (np.ones(M - 1, bool), np.ones(M, np.int32)):
        with pytest.raises(ValueError, match="keep"):
            fu.snapshot(min_obs, keep=bad)
        with pytest.raises(ValueError, match="keep"):
            fu.kept(min_obs, bad)


def test_the_chain_through_the_model_equals_the_chain_on_the_host(hip):
    from geoformer_amd import batch_eval
    from geoformer_amd.model import GeoFormer, load_config
    from tests.util import synthetic_state_dict

    model = GeoFormer(load_config("test_geoformer_scannet.yaml"))
    model.load_state_dict(synthetic_state_dict(model.state_dict(), 0))
    model.cuda().eval()
    with_box, without, _ = cc.box_gone()
    kw = dict(cell=cc.CELL, edge=cc.EDGE)
    fu, fh = frames.Fuser(**kw), frames.FuserHost(**kw)
    ca, ch = frames.Carver(fu), frames.CarverHost(fh)
    tr, th = frames.Tracker(), frames.TrackerHost()
    cells, cells_h = fu.add(with_box), fh.add(with_box)
    for chunk in (with_box, without, without):
        assert cc.same_vis(ca.observe(chunk), ch.observe(chunk))
    keep, keep_h = ca.keep(), ch.keep()
    assert cc.same(keep, keep_h) and 1000 < int((~keep_h).sum())
    fused, fused_h = fu.snapshot(1, cells, keep=keep), fh.snapshot(1, cells_h, keep=keep_h)
    assert sc.same_fused(fused, fused_h) and fused.xyz.shape[0] == int(keep_h.sum())
    raw, shift = fused.raw_scene()
    raw_h, shift_h = fused_h.raw_scene()
    assert (raw == raw_h).all() and (shift == shift_h).all()
    np.random.seed(0)
    (name, labels), = batch_eval.label_batches(model, [("frames", raw)], 1)
    got = frames.track_scene(tr, fu, labels, keep=keep)
    host = labels.to_host()
    want = frames.track_scene(th, fh, host, keep=keep_h)
    assert all(cc.same(a, b) for a, b in zip(got, want)) and got.ids.shape[0] == fused.xyz.shape[0]
    assert cc.same(frames.gather(fused, got.ids), frames.gather(fused_h, want.ids))


# ---- the C entry point --------------------------------------------------------------------------------------------------
def test_bad_arguments_launch_nothing(hip):
    from geoformer_amd._lib import ptr, stream_ptr

    n, F, H, W = 5, 2, 4, 8
    xyz = torch.zeros((n, 3), device="cuda")
    depth = torch.ones((F, H, W), device="cuda")
    table, inv = torch.ones((F, 16), device="cuda"), torch.ones((F, 12), device="cuda")
    out = torch.full((3, n), -7, dtype=torch.int32, device="cuda")
    st = torch.full((3, n), 5, dtype=torch.int32, device="cuda")
    good = dict(xyz=ptr(xyz), n=n, depth=ptr(depth), dtype=1, F=F, H=H, W=W, shift=1.0, table=ptr(table), inv=ptr(inv), near=0.1,
                far=10.0, edge=0.0, band=0.06, rel=0.02, out=ptr(out), codes=None, seen=ptr(st[0]), free=ptr(st[1]),
                score=ptr(st[2]), hit=1, miss=1, floor=-8, ceil=8, variant=0)
    bads = [dict(n=-1), dict(n=(1 << 29) + 1), dict(dtype=2), dict(F=0), dict(F=(1 << 16) + 1), dict(H=0), dict(W=(1 << 13) + 1),
            dict(shift=0.0), dict(shift=float("inf")), dict(near=float("nan")), dict(far=float("nan")), dict(edge=-1.0),
            dict(band=float("nan")), dict(rel=float("inf")), dict(variant=2), dict(variant=-1), dict(seen=None),
            dict(free=None, score=None), dict(hit=-1), dict(miss=-1), dict(floor=9), dict(seen=ptr(st[1])), dict(xyz=None),
            dict(depth=None), dict(table=None), dict(inv=None), dict(out=None)]
    for bad in bads:
        args = {**good, **bad}
        assert hip.gf_frames_visibility(*args.values(), stream_ptr()) != 0, bad
        assert b"gf_frames_visibility" in hip.gf_last_error()
    torch.cuda.synchronize()
    assert (out == -7).all() and (st == 5).all()
    assert hip.gf_frames_visibility(*{**good, "n": 0, "xyz": None, "out": None}.values(), stream_ptr()) == 0   # nothing to do
