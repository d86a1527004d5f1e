"""Furthest point sampling (k_fps, csrc/pointops.hip) bit for bit against the oracle's thread-by-thread restatement of the
reference kernel, in every launch regime: all eleven instantiations, every workgroup count, the tie-break blocks, the
"nothing left to pick" edges through the mailbox merge, batches over several launches, resume at the forward's geometry
and the launch queued by draw_sample.  Sizes and points: tests/fps_cases.py (tests/test_fps_plan_host.py proves that
the sizes reach the regimes).  Every case asserts the regime the planner puts it in before it runs, and every call
checks the kernel's error word."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import fps_cases as fc

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()  # (a copy: the shared cases are read-only)


def _assert_regime(hip, size):
    out = [ctypes.c_int(-1) for _ in range(5)]
    assert hip.gf_dev_fps_plan(size.n, *[ctypes.byref(o) for o in out]) == 0
    assert (out[0].value, out[2].value) == (size.G, size.inst), size
    return out[4].value  # point sets per launch


@functools.lru_cache(maxsize=4)
def _case(n, kind, m, origin0=False, b=1):
    """(points [b,n,3], the oracle's picks [b,m]): computed once per case, never written to."""
    from oracle import oracle as orc

    xyz = np.stack([fc.points(n, 17 + i, kind, origin0) for i in range(b)])
    ref = orc.fps(xyz, m)
    xyz.setflags(write=False)
    ref.setflags(write=False)
    return xyz, ref


def _fps(xyz, m, **kw):
    from geoformer_amd import pointops

    return pointops.furthest_point_sampling(_dev(xyz), m, check=True, **kw).cpu().numpy()


def _mismatch(got, ref):
    bad = np.argwhere(got != ref)
    return f"{len(bad)} picks differ, first at {bad[0].tolist()}: {got[tuple(bad[0])]} != {ref[tuple(bad[0])]}" if len(bad) else ""


@pytest.mark.parametrize("kind", fc.SIZE_KINDS)
@pytest.mark.parametrize("size", fc.SIZES, ids=lambda s: f"n{s.n}-G{s.G}-P{s.inst}")
def test_every_regime(hip, oracle, size, kind):
    _assert_regime(hip, size)
    m = fc.picks_for(size.n)
    xyz, ref = _case(size.n, kind, m)
    got = _fps(xyz, m)
    assert (got == ref).all(), _mismatch(got, ref)
    if size.n > m:
        assert len(np.unique(ref)) > m // 2  # a sequence, not a constant


def test_production_length(hip, oracle):
    size, m = fc.PRODUCTION
    _assert_regime(hip, size)
    xyz, ref = _case(size.n, "room", m)
    got = _fps(xyz, m)
    assert (got == ref).all(), _mismatch(got, ref)


@pytest.mark.parametrize("what", ["sparse", "origin", "point0"])
@pytest.mark.parametrize("size", fc.EDGE_SIZES, ids=lambda s: f"G{s.G}")
def test_nothing_left_to_pick_through_the_merge(hip, oracle, size, what):
    """More picks than points that can be picked: the sequence runs through the live candidates at distance 0 and then
    repeats the oracle's index; no point eligible at all: every pick is 0; point 0 itself not eligible."""
    _assert_regime(hip, size)
    m = fc.EDGE_PICKS
    xyz, ref = _case(size.n, "room" if what == "point0" else what, m, what == "point0")
    got = _fps(xyz, m)
    assert (got == ref).all(), _mismatch(got, ref)
    el = fc.eligible(xyz[0])
    if what == "sparse":
        assert el.sum() < m and ref[0, -1] == ref[0, -2] and len(np.unique(ref)) <= el.sum() + 1
        assert el[ref[0, 1:]].all()
    elif what == "origin":
        assert not el.any() and (got == 0).all()
    else:
        assert not el[0] and 0 not in got[0, 1:]


@pytest.mark.parametrize("m", fc.EDGE_M)
@pytest.mark.parametrize("size", fc.EDGE_SIZES, ids=lambda s: f"G{s.G}")
def test_few_picks(hip, oracle, size, m):
    """Fewer picks than, exactly as many as and just more than one exchange can deliver (FPS_K = 16, after the start)."""
    _assert_regime(hip, size)
    xyz, ref = _case(size.n, "room", m)
    got = _fps(xyz, m)
    assert got.shape == (1, m) and (got == ref).all(), _mismatch(got, ref)


def test_more_picks_than_points(hip, oracle):
    size, m = fc.OVERDRAW
    _assert_regime(hip, size)
    xyz, ref = _case(size.n, "room", m)
    got = _fps(xyz, m)
    assert (got == ref).all(), _mismatch(got, ref)
    assert (ref[0, size.n:] == ref[0, size.n]).all()  # the padding repeats one index


@pytest.mark.parametrize("bt", fc.BATCHES, ids=lambda bt: f"b{bt.b}-n{bt.size.n}")
def test_batch_over_several_launches(hip, oracle, bt):
    per_launch = _assert_regime(hip, bt.size)
    assert bt.b > per_launch == bt.launches[0]
    xyz, ref = _case(bt.size.n, "room", fc.BATCH_PICKS, False, bt.b)
    assert (xyz[0] != xyz[-1]).any() and (ref[0] != ref[-1]).any()
    got = _fps(xyz, fc.BATCH_PICKS)
    rows = [i for i in range(bt.b) if (got[i] != ref[i]).any()]
    assert not rows, f"point sets {rows} differ: {_mismatch(got, ref)}"
    if bt.b == 5:  # twice in a row on the same stream
        from geoformer_amd import pointops

        x = _dev(xyz)
        first = pointops.furthest_point_sampling(x, fc.BATCH_PICKS, check=True)
        second = pointops.furthest_point_sampling(x, fc.BATCH_PICKS, check=True)
        assert torch.equal(first, second) and (second.cpu().numpy() == ref).all()


@pytest.mark.parametrize("m0", fc.RESUME_M0)
@pytest.mark.parametrize("b,size", [(1, s) for s in fc.RESUME_SIZES] + [fc.RESUME_BATCH],
                         ids=lambda v: f"n{v.n}" if isinstance(v, fc.Size) else f"b{v}")
def test_resume_against_the_oracle(hip, oracle, b, size, m0):
    """Continuing from the ORACLE's first m0 picks gives the oracle's sequence."""
    _assert_regime(hip, size)
    m = fc.RESUME_M
    xyz, ref = _case(size.n, "room", m, False, b)
    known = _dev(ref[:, :m0])
    got = _fps(xyz, m, known=known)
    assert (got[:, :m0] == ref[:, :m0]).all()
    assert (got == ref).all(), _mismatch(got, ref)
    if m0 == m:  # nothing is launched: the output is the input, whatever it holds
        junk = _dev(np.arange(b * m, dtype=np.int32).reshape(b, m)[:, ::-1])
        assert (_fps(xyz, m, known=junk) == junk.cpu().numpy()).all()


@pytest.mark.parametrize("n,size", fc.DRAW, ids=lambda v: f"k{v.n}" if isinstance(v, fc.Size) else None)
def test_first_launch_queued_by_draw_sample(hip, oracle, n, size):
    """draw_sample with buffers made for a first sampling launch: its third result is the oracle's sequence over the
    points it gathered; twice on the same buffers."""
    from geoformer_amd import pointops

    _assert_regime(hip, size)
    k, m = size.n, fc.DRAW_FPS_M
    src = _dev(fc.points(n, 23, "room"))
    bufs = pointops.draw_sample_buffers(k, n, src.device, fps_m=m)
    flag_at = (hip.gf_fps_error_flag(bufs["fps_scratch"].data_ptr(), 1) - bufs["fps_scratch"].data_ptr()) // 4
    for rep in range(2):
        np.random.seed(31 + rep)
        got = pointops.draw_sample(n, k, src, bufs)
        assert got is not None and len(got) == 3
        idx, pts, picks = got
        assert picks.dtype == torch.int32 and tuple(picks.shape) == (1, m) and tuple(pts.shape) == (1, k, 3)
        assert torch.equal(pts[0], src[idx])
        ref = oracle.fps(pts.cpu().numpy(), m)
        assert int(bufs["fps_scratch"].view(torch.int32)[flag_at].item()) == 0
        assert (picks.cpu().numpy() == ref).all(), (rep, _mismatch(picks.cpu().numpy(), ref))


def test_draw_sample_shorter_than_the_first_launch(hip):
    from geoformer_amd import pointops

    n, k = fc.DRAW_SHORT
    assert k < fc.DRAW_FPS_M
    src = _dev(fc.points(n, 23, "room"))
    bufs = pointops.draw_sample_buffers(k, n, src.device, fps_m=fc.DRAW_FPS_M)
    np.random.seed(7)
    got = pointops.draw_sample(n, k, src, bufs)
    assert got is not None and len(got) == 2 and torch.equal(got[1][0], src[got[0]])


def test_refuses_more_points_than_the_largest_instantiation(hip):
    from geoformer_amd import _lib, pointops

    xyz = torch.zeros((1, fc.N_MAX + 1, 3), device="cuda")
    with pytest.raises(_lib.GeoFormerHipError, match="too large"):
        pointops.furthest_point_sampling(xyz, 8, check=True)
