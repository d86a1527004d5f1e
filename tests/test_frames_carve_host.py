"""The host statement of csrc/frames_carve.hip: frames.visibility_host against the rule restated as a loop over probes,
inverse_records, every boundary of the rule on constructed probes, CarverHost's update, keep= downstream, and what the
feature is for.  The inputs and what each size straddles are named in tests/frames_carve_cases.py."""
import numpy as np
import pytest
import torch

from geoformer_amd import frames
from tests import frames_cases as fc
from tests import frames_carve_cases as cc
from tests import frames_stream_cases as sc


@pytest.mark.parametrize("kind,edge", [("u16", None), ("u16", cc.EDGE), ("f32", cc.EDGE)])
def test_the_vectorised_statement_equals_the_loop_over_probes(kind, edge):
    fr, xyz = fc.make(fc.narrow(), kind), cc.narrow_points()
    vis, codes = frames.visibility_host(xyz, fr, edge=edge, codes=True)
    want_codes, want = cc.loop_statement(xyz, fr, 0.1, 10.0, edge, 0.06, 0.02)
    assert cc.same(codes, want_codes) and cc.same_vis(vis, want)
    assert set(np.unique(codes)) >= {cc.OUTSIDE, cc.UNKNOWN, cc.SEEN}
    assert cc.same_vis(frames.visibility_host(xyz, fr, edge=edge), want)                      # without codes: the counts alone
    assert cc.same_vis(frames.visibility(torch.from_numpy(np.array(xyz)), fr, edge=edge), want)  # a CPU tensor: the statement


def test_the_fused_points_of_a_frame_are_seen_by_it():
    fr = fc.make(fc.dense(3))
    fused = frames.fuse_host(sc.sub(fr, 0, 1), cell=cc.CELL)
    vis, codes = frames.visibility_host(fused.xyz.numpy(), sc.sub(fr, 0, 1), band=cc.BAND, codes=True)
    assert (codes[0] == cc.SEEN).mean() > 0.95 and vis.free.sum() < 0.01 * codes.size


def test_inverse_records():
    fr = fc.make(fc.dense(3))
    inv = frames.inverse_records(fr)
    assert inv.dtype == np.float32 and inv.shape == (3, 12)
    A = fr.table[:, 4:].reshape(3, 3, 4)
    assert (inv[:, 9:] == A[:, :, 3]).all()
    prod = inv[:, :9].reshape(3, 3, 3).astype(np.float64) @ A[:, :, :3].astype(np.float64)
    assert np.abs(prod - np.eye(3)).max() < 4 * np.finfo(np.float32).eps      # a rigid pose: entries <= 1, float32 rounding
    assert np.abs(inv[:, :9].reshape(3, 3, 3) - A[:, :, :3].transpose(0, 2, 1)).max() < 4 * np.finfo(np.float32).eps
    sh = cc.sheared(fr)
    inv = frames.inverse_records(sh)
    prod = inv[:, :9].reshape(3, 3, 3).astype(np.float64) @ sh.table[:, 4:].reshape(3, 3, 4)[:, :, :3].astype(np.float64)
    assert np.abs(prod - np.eye(3)).max() < 1e-5
    pose = np.eye(4)[None].copy()
    pose[0, 2, :3] = pose[0, 1, :3]                                            # two equal rows
    with pytest.raises(ValueError, match="singular"):
        frames.inverse_records(frames.make(np.ones((1, 2, 2), np.float32), [1, 1, 1, 1], pose, None, 1.0))
    with pytest.raises(ValueError, match="Frames"):
        frames.inverse_records(fr.table)


def test_every_boundary_of_the_rule():
    fr, pts = cc.boundary_frames(), cc.boundary_points()
    vis, codes = frames.visibility_host(pts, fr, cc.B_NEAR, cc.B_FAR, None, cc.B_BAND, cc.B_REL, codes=True)
    want = cc.boundary_codes()
    assert cc.same(codes, want), [(why, int(g), w) for (_, w, why), g in zip(cc.BOUNDARY, codes[0]) if g != w]
    assert cc.same(vis.seen, (want[0] == cc.SEEN).astype(np.int32)) and cc.same(vis.free, (want[0] == cc.FREE).astype(np.int32))
    assert cc.same(vis.occluded, (want[0] == cc.OCCLUDED).astype(np.int32))
    assert cc.same(cc.loop_statement(pts, fr, cc.B_NEAR, cc.B_FAR, None, cc.B_BAND, cc.B_REL)[0], want)


@pytest.mark.parametrize("edge", [None, cc.EDGE])
def test_depths_that_are_no_numbers_are_unknown(edge):
    fr = sc.nasty3()
    d = fr.depth.numpy()
    z = np.where(np.isfinite(d) & (d > 0), d, np.float32(1.0))
    # the world point of every pixel of frame 0 by the frame's own record, at a stand-in depth where the pixel has none
    F, H, W = d.shape
    fx, fy, cx, cy = fr.table[0, :4].astype(np.float64)
    P = fr.table[0, 4:].astype(np.float64).reshape(3, 4)
    j, i = np.mgrid[0:H, 0:W]
    cam = np.stack([(i + 0.5 - cx) * z[0] / fx, (j + 0.5 - cy) * z[0] / fy, z[0]], -1).reshape(-1, 3)
    pts = (cam @ P[:, :3].T + P[:, 3]).astype(np.float32)
    _, codes = frames.visibility_host(pts, sc.sub(fr, 0, 1), edge=edge, codes=True)
    bad = ~(np.isfinite(d[0]) & (d[0] >= np.float32(0.1)) & (d[0] <= 10)).reshape(-1)
    assert bad.sum() > 500 and (codes[0][bad] == cc.UNKNOWN).all()
    assert (codes[0][~bad] == cc.SEEN).sum() > 0.5 * (~bad).sum()
    if edge is None:
        assert (codes[0][~bad] == cc.SEEN).all()
    else:  # the edge filter makes more pixels unknown, never fewer
        plain = frames.visibility_host(pts, sc.sub(fr, 0, 1), codes=True)[1]
        assert ((codes == cc.UNKNOWN) >= (plain == cc.UNKNOWN)).all() and (codes == cc.UNKNOWN).sum() > (plain == cc.UNKNOWN).sum()


def test_arguments():
    fr, pts = cc.boundary_frames(), cc.boundary_points()
    for bad in (dict(band=-1), dict(rel=np.inf), dict(edge=-0.1), dict(near=np.nan)):
        with pytest.raises(ValueError):
            frames.visibility_host(pts, fr, **bad)
    with pytest.raises(ValueError, match="float32"):
        frames.visibility_host(pts.astype(np.float64), fr)
    with pytest.raises(ValueError, match="float32"):
        frames.visibility_host(pts[:, :2], fr)
    with pytest.raises(ValueError, match="Frames"):
        frames.visibility_host(pts, pts)
    vis, codes = frames.visibility_host(pts[:0], fr, codes=True)
    assert codes.shape == (1, 0) and all(v.shape == (0,) and v.dtype == np.int32 for v in vis)
    with pytest.raises(ValueError, match="FuserHost"):
        frames.CarverHost(frames.TrackerHost())
    fu = frames.FuserHost()
    for bad in (dict(hit=-1), dict(miss=1.5), dict(floor=3, ceil=2), dict(drop=2 ** 31), dict(band=-1.0)):
        with pytest.raises(ValueError):
            frames.CarverHost(fu, **bad)
    with pytest.raises(ValueError, match="CPU"):
        frames.Carver(fu, device="cuda")
    assert isinstance(frames.Carver(fu)._host, frames.CarverHost) and isinstance(frames.Carver(fu, device="cpu")._host, frames.CarverHost)
    assert isinstance(frames.Carver(frames.Fuser(device="cpu"))._host, frames.CarverHost)


# ---- CarverHost ---------------------------------------------------------------------------------------------------------
def _boundary_map():
    """A FuserHost of 1 m cells holding three points of the boundary frame: one seen, one the frame looks through, one
    hidden; and the frame."""
    fu = frames.FuserHost(cell=1.0, near=cc.B_NEAR, origin=(-8, -8, -8))
    fu.add_points(np.array([[0, 0, 2], [0.5, 0.25, 1.5], [0, 0, 3.5]], np.float32))
    return fu, cc.boundary_frames()


def _carver(fu, **kw):
    return frames.CarverHost(fu, band=cc.B_BAND, rel=cc.B_REL, **kw)


def test_carver_defaults_come_from_the_fuser():
    fu = frames.FuserHost(cell=0.05, near=0.3, far=4.0, edge=0.1)
    ca = frames.CarverHost(fu)
    near, far, e, band, rel = ca._probe
    assert (near, far, e, rel) == (np.float32(0.3), np.float32(4.0), np.float32(0.1), np.float32(0.02))
    assert band == np.float32(3.0 * float(np.float32(0.05)))


def test_carver_counts_and_clamps():
    fu, fr = _boundary_map()
    ca = _carver(fu)
    for k in range(1, 12):
        vis = ca.observe(fr)
        assert [v.tolist() for v in vis] == [[1, 0, 0], [0, 1, 0], [0, 0, 1]] and all(v.dtype == torch.int32 for v in vis)
        seen, free, score = ca.state()
        assert seen.tolist() == [k, 0, 0] and free.tolist() == [0, k, 0]
        assert score.tolist() == [min(k, 8), max(-k, -8), 0] and score.dtype == np.int32
        assert ca.keep().tolist() == [True, k < 2, True] and ca.keep(-8).tolist() == [True, k < 8, True]
    ca = _carver(fu, hit=2, miss=3, floor=-7, ceil=5)
    want = [(2, -3), (4, -6), (5, -7), (5, -7)]
    for s, f in want:
        ca.observe(fr)
        assert ca.state()[2].tolist() == [s, f, 0]


def test_one_clamp_per_observe_not_per_frame():
    """Two frames in one call: a cell seen by one and looked through by the other moves by hit - miss, whatever the order;
    a cell at the ceiling that a chunk sees once and looks through twice ends at ceil - 1, not at ceil - 2."""
    fu, fr = _boundary_map()
    far_depth = frames.make(np.full((1, cc.B_H, cc.B_W), 4.0, np.float32), [4.0, 4.0, 4.0, 2.0], np.eye(4)[None], None, 1.0)
    ca = _carver(fu, ceil=2)
    ca.observe(fr), ca.observe(fr), ca.observe(fr)
    assert ca.state()[2].tolist() == [2, -3, 0]
    vis = ca.observe(frames.concat([fr, far_depth, far_depth]))   # cell 0: seen once, free twice
    assert [v.tolist()[0] for v in vis] == [1, 2, 0] and ca.state()[2][0] == 1


def test_counts_saturate():
    fu, fr = _boundary_map()
    ca = _carver(fu)
    ca.observe(fr)
    ca._state[0, 0] = ca._state[1, 1] = 2 ** 31 - 2
    ca.observe(fr)
    assert ca.state()[0][0] == 2 ** 31 - 1 == ca.state()[1][1]
    ca.observe(fr)
    assert ca.state()[0][0] == 2 ** 31 - 1 == ca.state()[1][1] and ca.state()[0].dtype == np.int32


def test_the_state_grows_with_the_map_and_new_cells_are_kept():
    fu, fr = _boundary_map()
    ca = _carver(fu, drop=-1)
    assert ca.cells == 0 and ca.keep().tolist() == [True] * 3
    ca.observe(fr), ca.observe(fr)
    assert ca.keep().tolist() == [True, False, True]
    fu.add_points(np.array([[-0.5, 0.25, 1.0], [3, 3, 3]], np.float32))
    assert ca.cells == 3 and ca.keep().tolist() == [True, False, True, True, True]
    vis = ca.observe(fr)
    assert ca.cells == 5 and vis.free.tolist() == [0, 1, 0, 1, 0]
    assert [s.tolist() for s in ca.state()] == [[3, 0, 0, 0, 0], [0, 3, 0, 1, 0], [3, -3, 0, -1, 0]]


def test_a_failed_observe_leaves_the_state():
    fu, fr = _boundary_map()
    ca = _carver(fu)
    ca.observe(fr)
    before = ca.state()
    pose = np.eye(4)[None].copy()
    pose[0, :3, :3] = 0
    for bad in (fr.depth, None, frames.make(fr.depth, [4, 4, 4, 2], pose, None, 1.0)):
        with pytest.raises(ValueError):
            ca.observe(bad)
        assert all(cc.same(a, b) for a, b in zip(ca.state(), before))
    with pytest.raises(ValueError, match="empty"):
        frames.CarverHost(frames.FuserHost()).observe(fr)


def test_a_chunk_of_another_shape_is_observed():
    fr = sc.dense4()
    fu = frames.FuserHost(cell=cc.CELL)
    fu.add(fr)
    ca = frames.CarverHost(fu)
    vis = ca.observe(fc.make(fc.narrow(), "f32"))   # another size, dtype and depth_shift than the stream's
    assert int(vis.seen.sum()) > 100
    assert cc.same_vis(vis, frames.visibility_host(fu.snapshot(1).xyz.numpy(), fc.make(fc.narrow(), "f32"), band=cc.BAND))


# ---- keep= downstream ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stream():
    """A FuserHost and two VoterHosts fed dense(4) in two chunks, and every chunk's cells."""
    fr = sc.dense4()
    fu, sem, ins = frames.FuserHost(cell=sc.COARSE), frames.VoterHost(ignore=0), frames.VoterHost(ignore=0)
    case = fc.dense(fc.DENSE_FRAMES_TOP)
    lab = (np.maximum(case.index, -1) % 7).astype(np.int32)
    cells = []
    for a, b in ((0, 2), (2, 4)):
        c = fu.add(sc.sub(fr, a, b))
        sem.add(c, lab[a:b]), ins.add(c, lab[a:b] % 3)
        cells.append(c)
    return fu, sem, ins, torch.cat(cells)


@pytest.mark.parametrize("min_obs", [1, 3])
def test_keep_downstream(stream, min_obs):
    fu, sem, ins, cells = stream
    M = fu.cells
    base, rows = fu.snapshot(min_obs, cells), fu.kept(min_obs)
    labels = frames.lift_scene_stream(fu, sem, ins, min_obs)
    for ones in (np.ones(M, bool), np.ones(M, np.uint8), torch.ones(M, dtype=torch.bool)):
        assert sc.same_fused(fu.snapshot(min_obs, cells, keep=ones), base) and cc.same(fu.kept(min_obs, ones), rows)
        assert all(cc.same(a, b) for a, b in zip(frames.lift_scene_stream(fu, sem, ins, min_obs, keep=ones), labels))
    mask = np.random.default_rng(5).random(M) < 0.6
    got, got_rows = fu.snapshot(min_obs, cells, keep=mask), fu.kept(min_obs, mask.astype(np.uint8))
    on = mask[rows.numpy()]                                             # of today's points, the ones that stay
    assert 0 < on.sum() < on.size
    assert cc.same(got_rows, rows[torch.from_numpy(on)])
    for a, b in zip(got[:3], base[:3]):
        assert cc.same(a, b[torch.from_numpy(on)])
    renum = np.where(on, np.cumsum(on) - 1, -1).astype(np.int32)
    assert cc.same(got.point_of, np.where(base.point_of.numpy() >= 0, renum[np.maximum(base.point_of.numpy(), 0)], -1).astype(np.int32))
    for a, b in zip(frames.lift_scene_stream(fu, sem, ins, min_obs, keep=mask), labels):
        assert cc.same(a, b[torch.from_numpy(on)])
    none = fu.snapshot(min_obs, cells, keep=np.zeros(M, bool))
    assert none.xyz.shape == (0, 3) and (none.point_of == -1).all() and fu.kept(min_obs, np.zeros(M, bool)).shape == (0,)
    for bad in (mask[:-1], np.ones(M + 1, bool), np.ones((M, 1), bool), np.ones(M, np.int32)):
        with pytest.raises(ValueError, match="keep"):
            fu.snapshot(min_obs, cells, keep=bad)
        with pytest.raises(ValueError, match="keep"):
            fu.kept(min_obs, bad)
        with pytest.raises(ValueError, match="keep"):
            frames.lift_scene_stream(fu, sem, ins, min_obs, keep=bad)


class _Labels:
    """What track_scene reads of a SceneLabels: owner and the table's label_id, score and kept."""

    def __init__(self, owner, p):
        self.owner = owner
        self.table = type("T", (), dict(label_id=np.arange(p, dtype=np.int32) % 5, score=np.linspace(0.5, 1, p).astype(np.float32),
                                        kept=np.ones(p, bool)))


def test_track_scene_with_keep(stream):
    fu = stream[0]
    M = fu.cells
    mask = np.random.default_rng(6).random(M) < 0.7
    rows, rows_m = fu.kept(1), fu.kept(1, mask)
    owner = (rows.numpy() % 4).astype(np.int32)
    a = frames.track_scene(frames.TrackerHost(), fu, _Labels(owner, 4))
    b = frames.track_scene(frames.TrackerHost(), fu, _Labels(owner, 4), keep=np.ones(M, bool))
    assert all(cc.same(x, y) for x, y in zip(a, b))
    owner_m = (rows_m.numpy() % 4).astype(np.int32)
    got = frames.track_scene(frames.TrackerHost(), fu, _Labels(owner_m, 4), keep=mask)
    want = frames.TrackerHost().update(rows_m, owner_m, np.arange(4, dtype=np.int32) % 5, np.linspace(0.5, 1, 4).astype(np.float32),
                                       np.ones(4, bool))
    assert all(cc.same(x, y) for x, y in zip(got, want)) and got.ids.shape[0] == int(mask.sum())
    with pytest.raises(ValueError, match="keep"):
        frames.track_scene(frames.TrackerHost(), fu, _Labels(owner, 4), keep=mask[:-1])


# ---- what the feature is for, on the statement alone ----------------------------------------------------------------------
def test_a_static_scene_keeps_its_cells():
    """dense(4) added and observed once at 2 cm, band = 3 cells, rel = 0.02, edge 0.05.  Measured with CarverHost: 0 of
    5877 cells at score <= -2 (80 free probes in all, none twice on one cell).  The cap is 0.1 %: the measured share is
    zero, so the factor of two is taken on the issue's own prototype figure for these frames (0.03 % of its cells), rounded
    up."""
    fr = sc.dense4()
    fu = frames.FuserHost(cell=cc.CELL, edge=cc.EDGE)
    ca = frames.CarverHost(fu)
    fu.add(fr)
    vis = ca.observe(fr)
    score = ca.state()[2]
    share = float((score <= -2).mean())
    print(f"static: {fu.cells} cells, {int(vis.free.sum())} free probes, share at score <= -2: {share:.5f}")
    assert fu.cells > 5000 and share <= 0.001
    assert cc.same(ca.keep(), score > -2)


BOX_FLOOR = 0.875    # measured 0.9751 of 1649 box cells carved; ten points below
REST_CAP = 0.115     # measured 0.0571 of 15028 other cells carved; a factor of two above.  857 of those 858 cells hold
#                      background pixels: the FAR_FILL plane of one camera, which the other cameras look through
REAL_CAP = 0.0006    # measured 1 of the 3807 other cells without a background pixel (0.00026); a factor of two above


def test_a_box_that_left_is_carved():
    """4 frames with the box (background at FAR_FILL) added and observed, then two rounds of the same cameras on the scene
    without the box, observed only.  A cell is a box cell when most of its pixels came from box points.  Measured with
    CarverHost: the figures beside the thresholds above."""
    with_box, without, is_box = cc.box_gone()
    fu = frames.FuserHost(cell=cc.CELL, edge=cc.EDGE)
    ca = frames.CarverHost(fu)
    cells = fu.add(with_box)
    ca.observe(with_box)
    box = cc.box_cells(cells, is_box, fu.cells)
    ca.observe(without), ca.observe(without)
    gone = ~ca.keep().numpy()
    c = cells.numpy().reshape(-1)
    filled = np.bincount(c[c >= 0], weights=(fc.dense(fc.DENSE_FRAMES_TOP).index.reshape(-1)[c >= 0] < 0), minlength=fu.cells) > 0
    real = ~box & ~filled
    carved_box, carved_rest, carved_real = float(gone[box].mean()), float(gone[~box].mean()), float(gone[real].mean())
    print(f"box gone: {int(box.sum())} box cells, {int((~box).sum())} others ({int(real.sum())} without a background pixel); "
          f"carved {carved_box:.4f} of the box, {carved_rest:.5f} of the rest, {carved_real:.5f} of the real rest")
    assert box.sum() > 1000 and real.sum() > 1000
    assert carved_box >= BOX_FLOOR and carved_rest <= REST_CAP and carved_real <= REAL_CAP
