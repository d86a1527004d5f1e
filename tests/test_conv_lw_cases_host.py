"""Host side of the LDS-weight convolution's regime suite (no GPU): the float64 reference of tests/conv_lw_cases.py is
the oracle's convolution, the flat table's buffer holds a table of every bin count, the integer leg has headroom below
2^24, and the case lists of test_gpu_conv_lw_regimes.py reach every regime of k_conv_lw's per-wave step stream -- shown
from the restated dealing alone (conv_lw_cases.wave_streams), the launches by asking the planner itself."""
import ctypes

import numpy as np
import pytest

from tests import conv_lw_cases as C
from tests.test_conv_plan import ALIGN_KEYS, LW, OK, _call, _set_knobs
from tests.test_host_logic import lib  # noqa: F401  (the library, built for gfx950 if missing)


def test_reference_is_the_oracles_convolution(oracle):
    """On integer operands the oracle's scalar fp32 loop is exact, so it must EQUAL the float64 restatement: the plain
    sum, and prologue / residual / epilogue written around it.  The tables have absent rows inside present offsets,
    where the prologue's shift must be dropped with the row."""
    for name, form in [("r8", C.Form(48, 32, 1, "sep", 1, out2=True)), ("s4b", C.Form(32, 16, 1, "inplace", 1)),
                       ("one", C.Form(16, 16, 0, "none", 0)), ("e4", C.Form(16, 32, 1, "sep", 1))]:
        T = C.table(name)
        x, W, sc, sh, res, osc, osh = ops = C.operands(T, form, "int")
        assert (sh > 0).any() and (sh < 0).any()  # (a kept shift of an absent row would show)
        plain, _ = C.forward_ref(x, W, T.nbr, T.M_out)
        assert (oracle.conv_fwd(x, W, T.nbr, T.M_out).astype(np.float64) == plain).all()
        a = np.maximum(x * sc + sh, 0).astype(np.float32) if form.aff else x
        raw = oracle.conv_fwd(a, W, T.nbr, T.M_out).astype(np.float64) + (res if form.res != "none" else 0)
        act = np.maximum(raw * osc + osh, 0)
        want, want2 = C.expected(T, form, ops)
        if form.out2:
            assert (want == raw).all() and (want2 == act).all()
        else:
            assert (want == (act if form.act else raw)).all()
        if name not in ("e4",):
            assert np.abs(plain).max() > 20  # (not a comparison of zeros)


def test_integer_legs_stay_exact():
    """Every partial sum, sum + residual and epilogue value of the integer leg stays below 2^24 in magnitude: a
    condition on the operands' ranges (conv_lw_cases.int_bound), and what the references actually reach."""
    for name, form in C.CASES + [(C.EDGE_TABLE, f) for f in C.EDGE_FORMS]:
        assert C.int_bound(form) < 2 ** 24, (name, str(form))
    for name, form in [("r8", C.WIDE_FORMS[13]), ("s4a", C.WIDE_FORMS[11])]:
        T = C.table(name)
        ops = C.operands(T, form, "int")
        for v in C.expected(T, form, ops):
            assert v is None or (np.abs(v).max() <= C.int_bound(form) and (v == np.round(v)).all())
        assert np.abs(ops[0]).max() == C.X_LIM and np.abs(ops[1]).max() == C.W_LIM


def test_flat_buffer_holds_every_bin_count(lib):  # noqa: F811
    """gf_rules_flat_words sizes the table's buffer without knowing the bin count: it must hold the layout of every
    count the setter accepts (the descriptor rows grow with ceil(groups / bins) * bins)."""
    for ngroups in [1, 2, 3, 5, 63, 64, 65, 511, 513, 768, 1019, 1021, 1023, 1024, 1025, 2047, 2049, 9375]:
        words = lib.gf_rules_flat_words(27, 16 * ngroups)
        for nbins in range(4, C.BINS_DEFAULT + 1, 4):
            need = C.flat_layout(ngroups, nbins, 27 * ngroups)[2]
            assert need <= words, (ngroups, nbins, need, words)


def test_dealing_restated():
    """The dealing on a case small enough to write down: 10 groups over 4 bins, three rounds in snake order."""
    s = C.wave_streams([1, 9, 3, 7, 5, 5, 2, 8, 0, 4], 4)
    # sorted 9 8 7 5 | 5 4 3 2 (backwards) | 1 0
    assert [s[(b, 0)] for b in range(4)] == [[9], [8], [7], [5]]
    assert [s[(b, 1)] for b in range(4)] == [[2], [3], [4], [5]]
    assert [s[(b, 2)] for b in range(4)] == [[1], [0], [], []]
    s = C.wave_streams(list(range(1, 15)), 4)  # round 3 goes to wave 0 again
    assert s[(0, 0)] == [14] and s[(3, 0)] == [11, 2] and s[(2, 0)] == [12, 1] and s[(3, 1)] == [10] and s[(0, 2)] == [6]
    assert len(s) == 12 and sum(len(v) for v in s.values()) == 14
    assert C.passes(16) == [1] and C.passes(32) == [2] and C.passes(48) == [2, 1] and C.passes(64) == [2, 2]
    assert C.passes(112) == [2, 2, 2, 1]


def _ends_with_empties(st, n_exact=None, at_least=None):
    """A stream with a non-empty group followed by empty ones up to its end."""
    k = 0
    while k < len(st) and st[-1 - k] == 0:
        k += 1
    if k == len(st):
        return False
    return k == n_exact if n_exact is not None else k >= at_least


def test_case_lists_reach_every_regime(lib):  # noqa: F811
    cases = C.CASES
    assert len({(t, f.key()) for t, f in cases}) == len(cases)
    tables = {name: C.table(name) for name in C.TABLES}
    streams = {name: T.streams() for name, T in tables.items()}
    forms_of = {name: [f for t, f in cases if t == name] for name in C.TABLES}
    # every stream regime gets at least the three residual forms, under both ring depths
    for name in C.TABLES:
        got = {(D, f.res) for f in forms_of[name] for (_, _, D, _) in C.instantiations(f)}
        assert got >= {(D, r) for D in (6, 8) for r in ("none", "sep", "inplace")}, (name, got)

    # ---- operand forms: every instantiation, width, pass structure ----
    allf = [f for _, f in cases]
    inst = set().union(*(C.instantiations(f) for f in allf))
    assert inst == {(n, b, C.ring_depth(n, b), a) for n in (1, 2) for b in (1, 2) for a in (0, 1)} and len(inst) == 8
    assert {f.Cin for f in allf} == {16, 32, 48, 64, 112} and {f.Cout for f in allf} == {16, 32}
    assert {tuple(C.passes(f.Cin)) for f in allf} == {(1,), (2,), (2, 1), (2, 2), (2, 2, 2, 1)}
    for ncb in (1, 2):  # the second output with one and two column blocks; with and without a residual, in place too
        assert {f.res for f in allf if f.out2 and f.Cout == 16 * ncb} >= {"sep"}
    assert {f.res for f in allf if f.out2} == {"none", "sep", "inplace"}
    assert {(f.aff, f.act) for f in allf} == {(a, b) for a in (False, True) for b in (False, True)}
    assert any(len(C.passes(f.Cin)) > 1 and f.res == r and f.aff for f in allf for r in ("inplace",))
    assert any(len(C.passes(f.Cin)) > 1 and f.res == "none" for f in allf)  # later passes: residual = out all the same

    # ---- groups per wave ----
    per_wave = {name: {k: len(v) for k, v in st.items()} for name, st in streams.items()}
    counts = set().union(*(set(v.values()) for v in per_wave.values()))
    assert {0, 1, 2} <= counts and any(4 <= c < 64 for c in counts)
    T = tables["full4"]
    assert T.ngroups == C.LANES * C.WPS * T.nbins and T.M_out == 12_288
    assert set(per_wave["full4"].values()) == {64} and len(per_wave["full4"]) == 12  # a descriptor in every lane
    assert max(t.M_out for t in tables.values()) <= 12_288
    # an idle wave beside busy ones in its workgroup; a whole idle workgroup beside busy ones
    def workgroups(name):
        nb = tables[name].nbins
        return [[per_wave[name][(b, t)] for b in range(4 * w, 4 * w + 4) for t in range(C.WPS)] for w in range(nb // 4)]
    assert any(0 in wg and max(wg) > 0 for name in C.TABLES for wg in workgroups(name))
    assert any(max(wg) == 0 for wg in workgroups("few64")) and any(max(wg) > 0 for wg in workgroups("few64"))

    # ---- steps per wave and the residual wait's boundaries, for both ring depths ----
    for D in (6, 8):
        with_res = [name for name in C.TABLES
                    if any(f.res != "none" and D in {i[2] for i in C.instantiations(f)} for f in forms_of[name])]
        sts = [st for name in with_res for st in streams[name].values() if st]
        totals = {sum(st) for st in sts}
        assert {1, D - 1, D, D + 1, 2 * D - 1, 2 * D, 2 * D + 1, 27} <= totals, (D, sorted(totals))
        single = {st[0] for st in sts if len(st) == 1}
        assert {1, D - 1, D, D + 1, 2 * D - 1, 2 * D, 2 * D + 1, 27} <= single, (D, sorted(single))
        multi = [st for st in sts if len(st) >= 2]
        # the first group's request goes out behind the prologue's D gathers (since = -1): D steps wait, D + 1 do not
        assert {D, D + 1} <= {st[0] for st in multi}, (D, multi)
        # a later group's request is D consumed steps old after D steps: D - 1 steps wait, D do not
        assert {D - 1, D} <= {n for st in multi for n in st[1:]}, (D, multi)
        # ... and a later group behind a SHORT one (its own request went out less than D steps before)
        assert any(st[i] < D and st[i + 1] > 0 for st in multi for i in range(len(st) - 1))

    # ---- empty groups: the sort files them behind every other group, so at the end of a stream ----
    every = [(name, st) for name in C.TABLES for st in streams[name].values() if st]
    assert all(sorted(st, reverse=True) == st for _, st in every)
    assert any(_ends_with_empties(st, n_exact=1) for _, st in every)
    assert any(_ends_with_empties(st, at_least=2) for _, st in every)
    assert any(max(st) == 0 and tables[name].sizes.max() > 0 and len(st) >= 2 for name, st in every)  # an all-empty wave
    assert tables["e4"].sizes.max() == 0 and any(len(st) >= 2 for st in streams["e4"].values())  # an all-empty table
    assert any(0 < min(st) for _, st in every)

    # ---- ragged and absent rows ----
    assert any(t.M_out % 16 != 0 and t.sizes[-1] > 0 for t in tables.values())
    assert any(t.M_out % 16 != 0 and t.sizes[-1] == 0 for t in tables.values())
    assert tables["one"].M_out == 1 and tables["sixteen"].M_out == 16
    assert any(t.M_in < t.M_out for t in tables.values()) and any(t.M_in > t.M_out for t in tables.values())
    for t in tables.values():
        if t.sizes.max() > 0 and t.name != "one":
            rows = np.arange(t.M_out)
            bit = (t.gmask[rows // 16][None, :] >> np.arange(27, dtype=np.uint32)[:, None]) & 1
            assert ((t.nbr[:, : t.M_out] < 0) & (bit == 1)).any(), t.name  # a present offset with absent rows
        assert t.nbr.max() < t.M_in and t.nbr.min() >= -1 and (t.nbr[:, t.M_out:] == -1).all()

    # ---- bin counts ----
    assert {t.nbins for t in tables.values()} == {4, 8, 28, 64, 1024}
    for nb in (4, 8, 64):  # at least two rounds: the odd one runs over the bins backwards
        assert any(t.nbins == nb and t.ngroups > nb and len(set(t.sizes.tolist())) > 1 for t in tables.values()), nb
    assert all(any(t.nbins == nb and t.ngroups < nb for t in tables.values()) for nb in (28, 64, 1024))
    assert any(t.ngroups % t.nbins != 0 and t.ngroups > t.nbins for t in tables.values())  # a last round that is not full

    # ---- the launches: the planner's own answer for every case, under the case's bin count ----
    desc = (ctypes.c_int * 10)()
    al = {k: True for k in ALIGN_KEYS}

    def query(T, f):
        return dict(K=27, M_in=T.M_in, M_out=T.M_out, ld=T.ld, Cin=f.Cin, Cout=f.Cout, nbr=True, gmask=True, steps=False,
                    flat=True, sc=f.aff, res=f.res != "none", out2=f.out2, osc=f.act, aligned=al)

    seen = set()
    try:
        for name, f in cases:
            T = tables[name]
            _set_knobs(lib, dict(lw=1, bins=T.nbins))
            assert _call(lib, query(T, f), desc) == OK
            ps = C.passes(f.Cin)
            assert list(desc)[:8] == [LW, len(ps), ps[0], ps[-1], f.Cout // 16, 12, int(f.aff), T.nbins // 4], (name, str(f))
            assert desc[9] == 27 * ps[0] * (f.Cout // 16) * 1024
            seen |= C.instantiations(f)
        assert len(seen) == 8
        # one group beyond the lanes of 4 bins' waves: another kernel; under the default bin count the same table fits
        T = C.table(C.EDGE_TABLE)
        assert T.nbins == 4 and T.ngroups == 769
        for f in C.EDGE_FORMS:
            _set_knobs(lib, dict(lw=1, bins=4))
            assert _call(lib, query(T, f), desc) == OK and desc[0] != LW, str(f)
            _set_knobs(lib, dict(lw=1))
            assert _call(lib, query(T, f), desc) == OK and desc[0] == LW and desc[7] == 256
    finally:
        _set_knobs(lib, {})


def test_bin_count_setter(lib):  # noqa: F811
    """0 = the default; otherwise a multiple of 4 of at most 1024; a rejected value leaves the setting as it was."""
    desc = (ctypes.c_int * 10)()
    T = C.table("s4a")
    q = dict(K=27, M_in=T.M_in, M_out=T.M_out, ld=T.ld, Cin=32, Cout=32, nbr=True, gmask=True, steps=False, flat=True, sc=False,
             res=False, out2=False, osc=False, aligned={k: True for k in ALIGN_KEYS})
    try:
        _set_knobs(lib, dict(lw=1, bins=28))
        for bad in (-4, -1, 1, 2, 6, 1022, 1028, 4096):
            assert lib.gf_dev_conv_flat_bins(bad) != 0, bad
            assert b"gf_dev_conv_flat_bins" in lib.gf_last_error()
            assert _call(lib, q, desc) == OK and desc[7] == 7
        for good in (4, 8, 64, 1020, 1024):
            assert lib.gf_dev_conv_flat_bins(good) == 0
            assert _call(lib, q, desc) == OK and desc[7] == good // 4
        assert lib.gf_dev_conv_flat_bins(0) == 0
        assert _call(lib, q, desc) == OK and desc[7] == 256
    finally:
        _set_knobs(lib, {})
