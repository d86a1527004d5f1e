"""The sampler's launch planner (gf_dev_fps_plan, csrc/pointops.hip fps_plan) against the numpy restatement of
tests/fps_cases.py, the planner's invariants, and the coverage the GPU tests of tests/test_gpu_fps_regimes.py rest on:
a planner change that moves their sizes into other regimes fails here.  No GPU: the planner launches nothing."""
import ctypes

import numpy as np
import pytest

from tests import fps_cases as fc
from tests.test_host_logic import lib  # noqa: F401  (the library, built for gfx950 if missing)

OK, INVALID = 0, -1


def _lib_plan(lib, n):
    out = [ctypes.c_int(-7) for _ in range(5)]
    st = lib.gf_dev_fps_plan(int(n), *[ctypes.byref(o) for o in out])
    return st, tuple(o.value for o in out)  # G, P, inst, bs_log2, per_launch


def _sweeps():
    dense = np.arange(1, 8193)
    steps = np.arange(768, fc.N_MAX + 1, 768)
    coarse = np.unique(np.concatenate([steps - 1, steps, steps + 1]))
    return dense, coarse[coarse <= fc.N_MAX]


@pytest.mark.parametrize("sweep", [0, 1], ids=["1..8192", "multiples-of-768"])
def test_planner_equals_the_restatement(lib, sweep):
    ns = _sweeps()[sweep]
    ok, G, P, inst, bs_log2, per_launch = fc.plan_many(ns)
    assert ok.all() and ns[-1] == (8192, fc.N_MAX)[sweep]
    for i, n in enumerate(ns):
        st, got = _lib_plan(lib, n)
        assert st == OK, (n, lib.gf_last_error())
        assert got == (G[i], P[i], inst[i], bs_log2[i], per_launch[i]), n


def test_planner_invariants():
    for ns in _sweeps():
        ok, G, P, inst, bs_log2, per_launch = fc.plan_many(ns)
        assert ok.all()
        assert (fc.LANES * G * P >= ns).all() and (ns > fc.LANES * G * (P - 1)).all()
        ladder = np.asarray(fc.LADDER)
        assert np.isin(inst, ladder).all() and (inst >= P).all()
        below = np.where(ladder[None, :] < inst[:, None], ladder[None, :], 0).max(1)  # the next smaller entry (or 0)
        assert (below < P).all()
        assert (G >= 1).all() and (G * fc.FPS_KPUB <= 64).all()
        assert (per_launch >= 1).all() and (fc.FPS_WAVES * G * per_launch <= fc.RESIDENT_WAVES).all()
        assert [1 << int(v) for v in bs_log2] == [fc.oracle_block(int(n)) for n in ns]


def test_planner_refuses_what_the_kernel_cannot_hold(lib):
    assert fc.N_MAX == 270_336 and fc.plan(fc.N_MAX) == fc.Plan(16, 22, 22, 9, 4)
    st, got = _lib_plan(lib, fc.N_MAX + 1)
    assert st == INVALID and got == (-7,) * 5 and fc.plan(fc.N_MAX + 1) is None
    assert b"too large (max 270336)" in lib.gf_last_error()
    st, got = _lib_plan(lib, 1 << 22)
    assert st == INVALID and got == (-7,) * 5 and fc.plan(1 << 22) is None
    assert b"22-bit index" in lib.gf_last_error()
    assert _lib_plan(lib, (1 << 22) - 1)[0] == INVALID and b"too large" in lib.gf_last_error()
    assert _lib_plan(lib, 0)[0] == INVALID
    # the sampling call itself refuses the same sizes before it touches the device (null pointers are never read)
    for n, text in ((fc.N_MAX + 1, b"too large"), (1 << 22, b"22-bit index")):
        assert lib.gf_furthest_point_sampling(None, 1, n, 8, None, None, None) == INVALID
        assert text in lib.gf_last_error()


def test_error_flag_follows_the_mailboxes(lib):
    """gf_fps_error_flag: the word behind the b point sets' mailboxes, inside gf_fps_scratch_bytes(b)."""
    base = 1 << 20
    for b in (1, 2, 65):
        off = lib.gf_fps_error_flag(ctypes.c_void_p(base), b) - base
        assert off == b * 2 * fc.FPS_MAXG * fc.FPS_KPUB * 8
        assert off + 4 <= lib.gf_fps_scratch_bytes(b)


def test_gpu_table_is_what_the_planner_answers(lib):
    sizes = fc.all_sizes()
    assert len(fc.SIZES) == len(set(s.n for s in fc.SIZES)) == 49
    for s in sizes:
        pl = fc.plan(s.n)
        assert pl is not None and (pl.G, pl.inst) == (s.G, s.inst), s
        st, got = _lib_plan(lib, s.n)
        assert st == OK and got == tuple(pl), s
    assert [fc.plan(s.n).P for s in fc.LADDER16] == list(fc.LADDER16_P)
    assert [fc.plan(s.n).G for s in fc.G_SWEEP] == list(range(1, 16))


def test_gpu_table_covers_every_regime():
    plans = [fc.plan(s.n) for s in fc.SIZES]
    assert {p.inst for p in plans} == set(fc.LADDER) and len(fc.LADDER) == 11
    assert {p.G for p in plans} == set(range(1, fc.FPS_MAXG + 1))
    assert {p.bs_log2 for p in plans} >= {0, 1, 2, 6, 8, 9}
    # both ends of every instantiation at G = 16, and slots left empty on every lane (P below the instantiation)
    ends = {}
    for s in fc.LADDER16:
        ends.setdefault(s.inst, []).append(s.n)
    for inst, lo in zip(fc.LADDER[2:], (28801, 36865, 49153, 61441, 73729, 98305, 147457, 196609, 245761)):
        hi = fc.FPS_MAXG * fc.LANES * inst
        assert min(ends[inst]) == lo and max(ends[inst]) == hi, inst
        assert fc.plan(lo - 1).inst < inst or lo == 28801
        assert hi == fc.N_MAX or fc.plan(hi + 1).inst > inst
    assert fc.plan(28800).G == 15
    assert {p.P for p in plans if p.P < p.inst} == {7, 9, 13, 17, 21}
    # the batches take more than one launch, split as listed
    for bt in fc.BATCHES:
        per = fc.plan(bt.size.n).per_launch
        assert bt.b > per
        assert tuple(min(per, bt.b - b0) for b0 in range(0, bt.b, per)) == bt.launches, bt
    assert {len(bt.launches) for bt in fc.BATCHES} == {2, 3}
    # the edges run through the mailbox merge, resume at the forward's geometry
    assert [s.G for s in fc.EDGE_SIZES] == [2, 7, 16] and fc.OVERDRAW[1] > fc.OVERDRAW[0].n
    assert all(s.G == 16 for s in fc.RESUME_SIZES) and {s.inst for s in fc.RESUME_SIZES} == {3, 4}
    assert fc.RESUME_BATCH[1].G > 1
    # resume absorbs the known picks in groups of FPS_K: none, a partial group, exactly one, one and a bit, many
    assert {(m0 - 1) // fc.FPS_K for m0 in fc.RESUME_M0} >= {0, 1, 2, 7, 15, 31}
    assert {1, fc.FPS_K, fc.FPS_K + 1, fc.FPS_K + 2, fc.RESUME_M} <= set(fc.RESUME_M0)


@pytest.mark.parametrize("kind", fc.KINDS)
def test_point_generator(kind):
    for n in (1, 7, 41, 3000, 13440):
        p = fc.points(n, 3, kind)
        assert p.dtype == np.float32 and p.shape == (n, 3) and p.flags.c_contiguous
        assert (p == fc.points(n, 3, kind)).all() and (n < 3 or (p != fc.points(n, 4, kind)).any())
        el = fc.eligible(p)
        if kind == "origin":
            assert not el.any()
        elif kind == "sparse":
            assert 1 <= el.sum() <= 40 < fc.EDGE_PICKS
            if n > 40:
                idx = np.flatnonzero(el)
                assert el.sum() >= 36 and idx.min() < n // 8 and idx.max() > n - n // 8  # spread over the range
                assert len(np.unique(p[el], axis=0)) <= el.sum() - 11  # the duplicates
        elif n > 40:
            assert 4 <= (~el).sum() <= 8  # the origin's rim (lattice points may add the origin itself)
            _, counts = np.unique(p, axis=0, return_counts=True)
            assert counts.max() >= 30
            if kind == "lattice":
                assert (p * 4 == np.round(p * 4)).sum() >= 3 * (n - 5)
        assert not fc.eligible(fc.points(n, 3, kind, origin0=True))[0]
