"""Host side of the forward convolution's regime suite (no GPU): the case lists of tests/conv_fwd_cases.py reach every
regime label, the planner (asked with fake pointers, as test_conv_plan.py does) sends every case under its knobs to
exactly the family, template parameters and grid the case is meant for -- the cases that must LEAVE a family included --
the integer legs have headroom below 2^24, the numpy restatements of the step table and of k_group_chunks hold on cases
small enough to write down, and the kernels' reciprocal step division is exact for every (K, NCH) the argument checks
admit."""
import ctypes

import numpy as np
import pytest

from tests import conv_fwd_cases as F
from tests import conv_lw_cases as L
from tests.test_conv_plan import INVALID, OK, _call, _set_knobs, head_plan
from tests.test_host_logic import lib  # noqa: F401  (the library, built for gfx950 if missing)


def test_case_lists_reach_every_regime():
    ids = [c.id() for c in F.ALL_CASES]
    assert len(set(ids)) == len(ids)
    got = {}
    for c in F.ALL_CASES:
        got.setdefault(F.FAMILY[c.family], set()).update(F.labels(c))
    assert set(got) == set(F.REQUIRED)
    for fam, want in F.REQUIRED.items():
        assert got[fam] == want, (fam, sorted(want - got[fam]), sorted(got[fam] - want))
    # what the labels rest on, said once more in plain terms
    T = F.table("every")
    assert sorted(set(T.sizes.tolist())) == list(range(28)) and min(np.bincount(T.sizes)) >= 2 and T.M_out % 16 and T.ngroups == 85
    assert len({(c.want[0], c.form.aff, c.form.res != "none", c.want[1], c.want[2]) for c in F.CASES["g16p"]}) == 64
    assert {c.want[2] for c in F.CASES["g16p"]} == {4, 8, 12, 16}
    b = F.chunking("big", T.sizes)
    assert max(np.diff(b)) >= 70 and (np.diff(b) == 0).sum() == 3
    b = F.chunking("rule4096", T.sizes)
    assert len(b) == 4097 and (np.diff(b) == 0).sum() >= 4000
    big = [c for c in F.CASES["os"] if c.tname == "os2047"]
    assert len(big) == 1 and big[0].table.ngroups * 9 > 16384 == big[0].plan()[7] and big[0].form.aff and big[0].form.res == "sep"
    assert any(c.table.ngroups >= 2048 and c.want[:2] == [2, 4] for c in F.CASES["os"])
    assert max(c.table.M_out for c in F.ALL_CASES) <= 2048 * 16
    for c in F.ALL_CASES:  # prologue shifts of both signs: a shift kept for an absent row or step would show
        if c.form.aff:
            sh = L.operands(c.table, c.form, "int")[3]
            assert (sh != 0).any(), c.id()
    for name in ("every", "pair27", "pair8", "os37"):  # present offsets with absent rows
        t = F.table(name)
        rows = np.arange(t.M_out)
        bit = (t.gmask[rows // 16][None, :] >> np.arange(t.K, dtype=np.uint32)[:, None]) & 1
        assert ((t.nbr[:, : t.M_out] < 0) & (bit == 1)).any(), name
        assert t.nbr.max() < t.M_in and t.nbr.min() >= -1 and (t.nbr[:, t.M_out:] == -1).all()
    p = F.table("pair27")
    assert [bin(int(m)).count("1") for m in p.gmask[:4]] == [27, 0, 0, 5] and p.gmask[6] == p.gmask[7] != 0
    assert p.gmask[4] & p.gmask[5] == 0 and p.gmask[8] == p.gmask[9] == 0 and p.ngroups % 2 == 1


@pytest.mark.parametrize("fam", sorted(F.CASES))
def test_planner_sends_every_case_to_its_instance(lib, fam):  # noqa: F811
    desc = (ctypes.c_int * 10)()
    try:
        for c in F.CASES[fam]:
            _set_knobs(lib, c.knobs)
            q = c.query()
            assert _call(lib, q, desc) == OK, c.id()
            assert list(desc) == c.plan(), (c.id(), list(desc), c.plan())
            assert head_plan(q, c.knobs) == (OK, c.plan()), c.id()  # (the restated rules agree)
            assert desc[0] == c.family
    finally:
        _set_knobs(lib, {})
    if fam == "flat":  # 405 steps leave the flat kernel; one chunk fewer stays
        left = [c for c in F.CASES[fam] if c.family != F.FLAT]
        assert left and all(c.family == F.OS and c.table.K * (c.form.Cin // 16) == 405 for c in left)
        assert any(c.family == F.FLAT and c.table.K * (c.form.Cin // 16) == 378 and c.want == [6] for c in F.CASES[fam])


def test_integer_legs_stay_exact():
    for c in F.ALL_CASES:
        assert L.int_bound(c.form, c.table.K) < 2 ** 24, c.id()
    assert L.int_bound(L.Form(448, 224, 1, "sep", 1), 27) > 2 ** 17  # (the widest case is not a trivial one)
    for c in [F.CASES["pair"][3], F.CASES["os"][4], F.CASES["flat"][-3]]:
        ops = L.operands(c.table, c.form, "int")
        for v in L.expected(c.table, c.form, ops):
            assert v is None or (np.abs(v).max() <= L.int_bound(c.form, c.table.K) and (v == np.round(v)).all())
        assert ops[1].shape[0] == c.table.K


def test_reciprocal_step_division(lib):  # noqa: F811
    """k_conv_os and conv_flat_item compute s / NCH as (s * ceil(65536 / NCH)) >> 16.  Exact for every step of every
    (K <= 32, NCH <= 50); the first miss is NCH = 51, K = 27, s = 1325.  conv_fwd_impl admits K <= 32 and
    Cin <= CONV_MAX_CIN = 512 (NCH <= 32) -- for every call, not only with a prologue."""
    for K in range(1, 33):
        for nch in range(1, 51):
            assert F.reciprocal_exact(K, nch), (K, nch)
    assert not F.reciprocal_exact(27, 51)
    s = np.arange(27 * 51)
    bad = np.nonzero(((s * F._ceil(65536, 51)) >> 16) != s // 51)[0]
    assert bad[0] == 1325 and all(F.reciprocal_exact(K, 51) for K in range(1, 26))
    desc = (ctypes.c_int * 10)()
    base = dict(K=27, M_in=160, M_out=160, ld=160, Cout=32, nbr=True, gmask=True, steps=False, flat=False, sc=False,
                res=False, out2=False, osc=False, aligned={k: True for k in ("in", "sc", "out", "res", "out2", "osc")})
    for K in (1, 8, 27, 32):
        for Cin, sc, rc in [(F.MAX_CIN, False, OK), (F.MAX_CIN + 1, False, INVALID), (51 * 16, False, INVALID),
                            (F.MAX_CIN - 16, True, OK), (F.MAX_CIN - 15, True, INVALID), (4096, False, INVALID)]:
            assert _call(lib, dict(base, K=K, Cin=Cin, sc=sc), desc) == rc, (K, Cin, sc)
    assert _call(lib, dict(base, K=33, Cin=16), desc) == INVALID
    assert F._ceil(F.MAX_CIN, 16) <= 50


def test_step_table_restated():
    """Two groups small enough to write down: offsets 3 and 20 in the first, thirteen offsets in the second."""
    ld, M_out, M_in = 32, 29, 50
    nbr = np.full((27, ld), -1, np.int32)
    nbr[3, 0], nbr[3, 5], nbr[20, 15] = 7, 8, 9
    for k in range(13):
        nbr[2 * k, 16 + k] = 30 + k
    nbr[26, 30] = 49  # (a row from M_out on: absent)
    T = L.Table("two", 0, M_in, M_out, nbr, [2, 13])
    buf = F.step_table(T, [0, 1, 1, 2])
    assert buf.size == F.steps_words(ld) == 2 * 7 * 64 + 4096 + 16
    blocks = buf[: 2 * 7 * 64].reshape(2, 7, 16, 4)
    poison = F.poison_buffer(ld, M_in)
    pblocks = poison[: 2 * 7 * 64].reshape(2, 7, 16, 4)
    assert blocks[0, 0, 0].tolist() == [7, -1, -1, -1] and blocks[0, 0, 5, 0] == 8 and blocks[0, 0, 15].tolist() == [-1, 9, -1, -1]
    assert (blocks[0, :3, :, :].reshape(-1, 4)[:, 2:] == -1).all() and (blocks[0, 1:3] == -1).all()
    assert (blocks[0, 3:] == pblocks[0, 3:]).all() and F.written_blocks(2) == 3  # unwritten: what the buffer held
    for s in range(13):
        col = blocks[1, s // 4, :, s % 4]
        assert col[s] == 30 + s and (np.delete(col, s) == -1).all()
    assert (blocks[1, 3, :, 1:] == -1).all() and (blocks[1, 4:] == pblocks[1, 4:]).all() and F.written_blocks(13) == 4
    assert (pblocks >= 0).all() and (pblocks < M_in).all() and len(set(pblocks.ravel().tolist())) == M_in
    tail = buf[2 * 7 * 64:]
    assert tail[:5].tolist() == [3, 0, 1, 1, 2] and (tail[5:] == poison[2 * 7 * 64 + 5:]).all() and (tail[5:] >= F.BOUND_POISON).all()
    # the spot check of test_gpu_fullsize.py on the same builder
    for n in range(28):
        assert F.written_blocks(n) * 4 == max(12, (n + 3) // 4 * 4)


def test_group_chunks_restated():
    """The floor rule on four groups of costs 4, 13, 24, 3 (sizes 1, 10, 13, 0): C = 44."""
    assert [F.chunk_cost(n) for n in (0, 1, 12, 13, 27)] == [3, 4, 15, 24, 38]
    sizes = [1, 10, 13, 0]
    # preceding costs 0, 4, 17, 41: chunk c starts at the first group with floor(before * n / 44) >= c
    assert F.group_chunks(sizes, 4) == [0, 2, 3, 3, 4]       # floors 0 0 1 3
    assert F.group_chunks(sizes, 2) == [0, 3, 4]             # floors 0 0 0 1
    assert F.group_chunks(sizes, 11) == [0, 1, 2, 2, 2, 3, 3, 3, 3, 3, 3, 4]  # floors 0 1 4 10
    assert F.group_chunks([], 4) == [0, 0, 0, 0, 0] and F.group_chunks([5], 3) == [0, 1, 1, 1]
    rng = np.random.default_rng(5)
    for ng, n in [(1, 4096), (85, 12), (85, 4096), (1200, 3072), (5000, 4)]:
        sizes = rng.integers(0, 28, ng)
        b = F.group_chunks(sizes, n)
        assert len(b) == n + 1 and b[0] == 0 and b[-1] == ng and (np.diff(b) >= 0).all()
        cost = np.array([F.chunk_cost(int(s)) for s in sizes])
        cs = np.concatenate([[0], np.cumsum(cost)])
        per = cs[np.array(b[1:])] - cs[np.array(b[:-1])]
        assert per.sum() == cost.sum() and per.max() <= cost.sum() / n + 2 * cost.max()  # (equal cost: no chunk far above its share)
