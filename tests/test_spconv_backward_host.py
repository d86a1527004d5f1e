"""Host side of the sparse convolution's backward suite (no GPU): the float64 references of
tests/spconv_backward_ref.py are the oracle's operations, and the case lists of test_gpu_spconv_backward.py reach
every regime the gradient kernels have -- the weight gradient's by a restatement of conv_wgrad_masked_impl's choice,
the input gradient's by asking the launch planner itself."""
import ctypes

import numpy as np
import pytest

from tests import spconv_backward_ref as R
from tests.test_conv_plan import ALIGN_KEYS, FAMILY, FORCED, FLAT, G16, G16P, LW, OK, OS, PAIR, _call, _set_knobs
from tests.test_gpu_spconv_backward import DGRAD_CASES, FORCED_KNOBS, FORCED_WIDTHS, WGRAD_CASES, case_id
from tests.test_host_logic import lib  # noqa: F401  (the library, built for gfx950 if missing)
from tests.util import random_voxels


@pytest.fixture(scope="module")
def sizes(oracle):
    """voxel set -> (rows, rows of its down-sampled level)"""
    out = {}
    for name in sorted({c[0] for c in WGRAD_CASES}):
        coords, shape, _ = R.voxels(name)
        out[name] = (coords.shape[0], oracle.rules_down2(coords, shape)[0].shape[0])
    return out


@pytest.mark.parametrize("Cin,Cout", [(19, 21), (112, 112)])
def test_references_are_the_oracles_operations(oracle, Cin, Cout):
    """On integer operands the oracle's scalar fp32 loops are exact, so they must EQUAL the float64 restatements:
    submanifold, child (M_out = the coarse count, far below ld) and up (one offset per row) tables."""
    rng = np.random.default_rng(Cin * 3 + Cout)
    shape = (20, 18, 16)
    coords = random_voxels(rng, 700, shape, 2, surface=True)
    M = coords.shape[0]
    nbr = oracle.rules_subm3(coords, shape)
    oc, child, parent, koff = oracle.rules_down2(coords, shape)
    up = oracle.up_table(parent, koff)
    Mc = oc.shape[0]
    assert M % 16 != 0 and 0 < Mc < M - 16
    for tbl, K, M_in, M_out in [(nbr, 27, M, M), (child, 8, M, Mc), (up, 8, Mc, M)]:
        X = R.rows_operand(rng, (M_in, Cin), "int")
        G = R.rows_operand(rng, (M_out, Cout), "int")
        W = R.weight_operand(rng, K, Cin, Cout, "int")
        ref_w, ref_d = R.wgrad_ref(X, G, tbl, K, M_out), R.dgrad_ref(G, W, tbl, M_in, M_out)
        assert np.abs(ref_w).max() > 20 and np.abs(ref_d).max() > 20  # (not a comparison of zeros)
        assert (oracle.conv_wgrad(X, G, tbl, K).astype(np.float64) == ref_w).all()
        assert (oracle.conv_dgrad(G, W, tbl, M_in).astype(np.float64) == ref_d).all()
    # no table (K = 1): the rows themselves
    X, G = R.rows_operand(rng, (M, Cin), "int"), R.rows_operand(rng, (M, Cout), "int")
    W = R.weight_operand(rng, 1, Cin, Cout, "int")
    ident = np.arange(M, dtype=np.int32)[None]
    assert (R.wgrad_ref(X, G, None, 1, M) == R.wgrad_ref(X, G, ident, 1, M)).all()
    assert (R.dgrad_ref(G, W, None, M, M) == R.dgrad_ref(G, W, ident, M, M)).all()


def wgrad_kernel(has_tbl, has_mask, K, Cin, Cout, M_out):
    """conv_wgrad_masked_impl's choice (csrc/spconv_conv.hip): (kernel, slices, items per slice)."""
    if ((not has_mask or not has_tbl) and not (K == 1 and not has_tbl)) or Cin % 16 or Cout % 16:
        return "plain", (M_out + 2047) // 2048, K * ((Cin + 15) // 16) * ((Cout + 15) // 16)
    nslices = (M_out + 1023) // 1024
    return ("tiled-xcd" if nslices >= 128 else "tiled"), nslices, K * (Cin // 16) * (Cout // 16)


def _wgrad_routes(case, sizes):
    """The launches test_wgrad makes for a case: (kernel, slices, items, K, Cin, Cout, M_out, table)."""
    name, kind, Cin, Cout = case
    g = R.geometry(kind, *sizes[name])
    has_tbl = g["tbl"] is not None
    out = []
    for has_mask in (False, True, True):  # sparse.conv_wgrad without / with gmask, gf_conv_wgrad_masked_acc
        if not has_tbl and has_mask:  # the 1x1x1: gf_conv_wgrad_masked(_acc) without table and masks
            has_mask = False
            kern = wgrad_kernel(False, False, 1, Cin, Cout, g["rows_out"])
        elif not has_tbl:  # sparse.conv_wgrad -> gf_conv_wgrad
            kern = ("plain", (g["rows_out"] + 2047) // 2048, ((Cin + 15) // 16) * ((Cout + 15) // 16))
        else:
            kern = wgrad_kernel(True, has_mask, g["K"], Cin, Cout, g["rows_out"])
        out.append(kern + (g["K"], Cin, Cout, g["rows_out"], g["tbl"], g["ld"]))
    return out


def dgrad_query(case, sizes, flat_route, residual, forced_tables=False):
    """The planner's view of a case's input-gradient launch: the forward kernel with rows and widths swapped, over the
    backward table; step / flat tables where sparse.subm_rules builds them (or where the test builds them itself)."""
    from geoformer_amd import sparse

    name, kind, Cin, Cout = case
    g = R.geometry(kind, *sizes[name])
    has_tbl = g["btbl"] is not None
    subm = kind == "subm"
    return dict(K=g["K"], M_in=g["rows_out"], M_out=g["rows_in"], ld=g["bld"], Cin=Cout, Cout=Cin, nbr=has_tbl,
                gmask=has_tbl, steps=subm and (forced_tables or g["bld"] >= sparse.STEPS_MIN_ROWS),
                flat=subm and flat_route and (forced_tables or g["bld"] >= sparse.FLAT_MIN_ROWS), sc=False, res=residual,
                out2=False, osc=False, aligned={k: True for k in ALIGN_KEYS})


def test_case_lists_reach_every_regime(lib, sizes):  # noqa: F811
    assert len(set(WGRAD_CASES)) == len(WGRAD_CASES) and set(DGRAD_CASES) <= set(WGRAD_CASES)
    # ---- weight gradient ----
    routes = [r for c in WGRAD_CASES for r in _wgrad_routes(c, sizes)]
    kernels = {r[0] for r in routes}
    assert kernels == {"plain", "tiled", "tiled-xcd"}, kernels
    xcd = [r for r in routes if r[0] == "tiled-xcd"]
    # the XCD order's two early exits: a last round of 8 slices that is not full, a last workgroup of a slice that is not
    assert any(r[1] % 8 != 0 and r[2] % 4 != 0 for r in xcd), xcd
    assert any(r[3] == 8 for r in xcd) and any(r[3] == 1 for r in xcd) and any(r[3] == 27 for r in xcd)
    tiled = [r for r in routes if r[0] != "plain" and r[7] is not None]
    assert any(r[4] // 16 == 14 and r[5] // 16 == 7 for r in tiled), "no table case at NCI = 14, NCO = 7"
    assert any(r[4] // 16 > 2 and r[3] == 8 for r in tiled), "no K = 8 table beyond two channel blocks"
    assert any(r[6] % 16 != 0 for r in tiled) and any(r[6] == 1 for r in tiled) and any(r[6] == 17 for r in tiled)
    assert any(r[7] == "child" and r[6] < r[8] - 1024 for r in tiled), "no child table with M_out far below ld"
    plain = [r for r in routes if r[0] == "plain"]
    assert any(r[4] % 16 and r[5] % 16 and r[5] % 4 for r in plain), "plain kernel: no case ragged on both sides"
    assert any(r[4] % 16 == 0 and r[5] % 16 for r in plain) and any(r[4] % 16 and r[5] % 16 == 0 for r in plain)
    assert any(r[1] > 1 and r[6] % 2048 for r in plain)
    # ---- input gradient: the families the size-based choice takes ----
    desc = (ctypes.c_int * 10)()
    seen = set()
    _set_knobs(lib, {})
    for case in DGRAD_CASES:
        for flat_route, residual in [(False, False), (True, False), (True, True)]:  # conv_dgrad, with flat=, executor call
            q = dgrad_query(case, sizes, flat_route, residual)
            assert _call(lib, q, desc) == OK, (case, q)
            seen.add((desc[0], desc[2] if desc[0] == OS else -1, desc[3] if desc[0] == OS else -1))
    fam = {s[0] for s in seen}
    assert {LW, FLAT, G16P, PAIR, OS} <= fam, [FAMILY[f] for f in fam]
    assert {(OS, 0, 1), (OS, 4, 1), (OS, 0, 0), (OS, 4, 0)} <= seen, seen  # waves per item, 16-byte gathers or not
    # ---- the in-place call under the forced knob sets ----
    assert FORCED_KNOBS == [dict(k, flat=0) for k in FORCED] + [dict(flat=1), dict(lw=1)]
    seen = set()
    try:
        for kn in FORCED_KNOBS:
            _set_knobs(lib, kn)
            for Cin, Cout in FORCED_WIDTHS:
                q = dgrad_query(("mid", "subm", Cin, Cout), sizes, True, True, forced_tables=True)
                assert _call(lib, q, desc) == OK, (kn, q)
                seen.add((desc[0], desc[2] if desc[0] == OS else (desc[1] if desc[0] in (G16, G16P) else -1)))
    finally:
        _set_knobs(lib, {})
    fam = {s[0] for s in seen}
    assert {LW, FLAT, G16P, G16, PAIR, OS} <= fam, [FAMILY[f] for f in fam]
    assert {(OS, 0), (OS, 4), (OS, 16), (G16, 1), (G16, 2), (G16P, 1), (G16P, 2)} <= seen, seen


def test_integer_legs_stay_exact(sizes):
    """Every partial sum of the integer leg stays below 2^24 in magnitude: a condition on the operands."""
    for case in WGRAD_CASES:
        name, kind, Cin, Cout = case
        g = R.geometry(kind, *sizes[name])
        # dW: one product of two values in [-3, 3] per output row; _acc twice on top of an initial value in [-3, 3]
        assert g["rows_out"] * R.FEAT_LIM * R.FEAT_LIM < 2 ** 24, case_id(case)
        assert 2 * g["rows_out"] * R.FEAT_LIM * R.FEAT_LIM + R.FEAT_LIM < 2 ** 24, case_id(case)
        # dX: K offsets x Cout channels of (gradient in [-3, 3]) x (weight in [-2, 2]), plus the residual
        assert g["K"] * Cout * R.FEAT_LIM * R.W_LIM + R.FEAT_LIM < 2 ** 24, case_id(case)
