"""The sparse convolution's two gradients, operator by operator, against float64 numpy restatements
(tests/spconv_backward_ref.py, pinned to the oracle by test_spconv_backward_host.py), at every regime the kernels
have: both weight-gradient kernels, the tiled one in both item orders; the input gradient (= the forward kernel over
the transposed relation with gf_conv_pack_weights_t) through sparse.conv_dgrad and through the call
gf_unet_train_bwd makes, which accumulates in place by passing one buffer as `residual` and `out`.

Two legs per case.  Integer operands: the result must EQUAL the reference (sums of small integers are exact in fp32
in any order; test_spconv_backward_host.py asserts the headroom below 2^24), so one dropped, doubled or misplaced
row fails.  Gaussian operands: the bounds test_gpu_fullsize.py holds for these operators, 1e-4 (input gradient) and
2e-4 (weight gradient) of max(1, max|ref|); the largest error of every route is printed (-s).

What each case list reaches (kernels, item orders, launch families) is proven without a GPU by
test_spconv_backward_host.py::test_case_lists_reach_every_regime."""
import types

import numpy as np
import pytest
import torch

from tests import spconv_backward_ref as R
from tests.test_gpu_fullsize import KNOBS

pytestmark = pytest.mark.gpu

DGRAD_TOL, WGRAD_TOL = 1e-4, 2e-4  # of max(1, max|ref|): test_gpu_fullsize.py::test_conv_dgrad_wgrad_full_size
LEGS = ["int", "gauss"]

# (voxel set, kind, Cin, Cout) of the FORWARD convolution; kinds as spconv_backward_ref.geometry names them.
_C = [16 * i for i in range(1, 8)]  # the m = 16 network's widths, level by level
_MID = ([("mid", "subm", c, c) for c in _C] + [("mid", "subm", 2 * c, c) for c in _C]
        + [("mid", "down", c, c + 16) for c in _C[:-1]] + [("mid", "inv", c + 16, c) for c in _C[:-1]]
        + [("mid", "1x1", 2 * c, c) for c in _C]
        # ragged widths (the m = 8 / m = 12 networks of test_gpu_widths.py, and one pair ragged on both sides)
        + [("mid", "subm", 8, 8), ("mid", "subm", 16, 8), ("mid", "subm", 24, 12), ("mid", "subm", 12, 24), ("mid", "subm", 19, 21),
           ("mid", "down", 12, 24), ("mid", "inv", 24, 12), ("mid", "1x1", 24, 12)])
_BIG = ([("big", "subm", a, b) for a, b in [(16, 16), (32, 16), (16, 32), (32, 32), (64, 32), (112, 112), (19, 21)]]
        + [("big", "down", 16, 32), ("big", "inv", 32, 16), ("big", "1x1", 32, 16)])
_DENSE = [("dense", "subm", 16, 16), ("dense", "subm", 32, 16), ("dense", "subm", 64, 32), ("dense", "subm", 19, 21),
          ("dense", "down", 16, 32), ("dense", "inv", 32, 16)]
_TINY = [(t, k, a, b) for t in ("tiny1", "tiny17", "tiny40")
         for k, a, b in [("subm", 16, 16), ("subm", 32, 16), ("subm", 19, 21), ("subm", 224, 112), ("down", 16, 32),
                         ("inv", 32, 16), ("1x1", 32, 16)]]
DGRAD_CASES = _BIG + _MID + _DENSE + _TINY
# the input convolution 6 -> 16 has no input gradient
WGRAD_CASES = DGRAD_CASES + [("big", "subm", 6, 16), ("mid", "subm", 6, 16), ("tiny40", "subm", 6, 16)]
# the in-place call under every forced launch family, on `mid` with step and flat tables built for it
FORCED_WIDTHS = [(16, 16), (32, 16), (16, 32), (32, 32), (64, 32)]
FORCED_KNOBS = KNOBS + [dict(lw=1)]


def case_id(case):
    return "%s-%s-%dx%d" % case


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def tables(hip, oracle):
    """name -> the voxel set's tables: built by the HIP rulebooks, asserted equal to the oracle's; the references
    are computed from the oracle's copies."""
    from geoformer_amd import sparse

    cache = {}

    def get(name):
        if name in cache:
            return cache[name]
        coords, shape, B = R.voxels(name)
        M = coords.shape[0]
        nbr = oracle.rules_subm3(coords, shape)
        oc, child, parent, koff = oracle.rules_down2(coords, shape)
        up = oracle.up_table(parent, koff)
        c = _dev(coords)
        rules = sparse.subm_rules(c, sparse.build_index(c, B, shape))
        r = sparse.down_rules(c, B, shape)
        assert rules.M == M and rules.ld == nbr.shape[1] and (rules.nbr.cpu().numpy() == nbr).all()
        assert r.M_out == oc.shape[0] and r.ld == child.shape[1] and r.ld_up == up.shape[1]
        assert (r.child.cpu().numpy() == child).all() and (r.up.cpu().numpy() == up).all()
        if name == "tiny17":
            assert (nbr[np.arange(27) != 13] < 0).all()  # isolated voxels: the centre offset only
        T = types.SimpleNamespace(name=name, M=M, Mc=oc.shape[0], host=dict(nbr=nbr, child=child, up=up),
                                  dev=dict(nbr=(rules.nbr, rules.gmask), child=(r.child, r.gmask_down),
                                           up=(r.up, r.gmask_up)),
                                  steps=rules.steps, flat=rules.flat, rules=rules, coords=c, shape=shape, batch=B)
        cache[name] = T
        return T

    return get


def _report(what, leg, err, tol):
    print("[spconv-bwd] %-58s %-5s max|err| = %.3e  bound = %.3e" % (what, leg, err, tol))


def _check_dw(got, want, ref, leg, what, htbl, M_out, base=None):
    """got (device) against want = the float64 expectation; `ref` scales the Gaussian bound.  Offsets that no output row
    has keep exactly what dW held (zero, or `base`)."""
    got = got.cpu().numpy().astype(np.float64)
    err = np.abs(got - want)
    if htbl is not None:
        for k in range(want.shape[0]):
            if not (htbl[k, :M_out] >= 0).any():
                assert (got[k] == (0.0 if base is None else base[k])).all(), (what, leg, "offset without a neighbour", k)
    if leg == "int":
        bad = np.argwhere(err != 0)
        ks = sorted(set(bad[:, 0].tolist()))
        assert bad.shape[0] == 0, ("%s: %d of %d entries differ, in offsets k = %s; first (k, ci, co) %s: got %s, want %s"
                                   % (what, bad.shape[0], err.size, ks[:27], bad[:4].tolist(),
                                      [got[tuple(b)] for b in bad[:4]], [want[tuple(b)] for b in bad[:4]]))
    else:
        tol = WGRAD_TOL * max(1.0, float(np.abs(ref).max()))
        _report(what, leg, float(err.max()), tol)
        assert float(err.max()) < tol, (what, float(err.max()), tol, np.unravel_index(err.argmax(), err.shape))


def _check_dx(got, want, ref, leg, what):
    got = got.cpu().numpy().astype(np.float64)
    err = np.abs(got - want)
    if leg == "int":
        rows = np.unique(np.argwhere(err != 0)[:, 0])
        assert rows.size == 0, ("%s: %d of %d rows differ; first rows %s (16-row groups %s), columns of the first %s"
                                % (what, rows.size, err.shape[0], rows[:8].tolist(), sorted(set((rows[:8] // 16).tolist())),
                                   np.nonzero(err[rows[0]])[0][:8].tolist() if rows.size else []))
    else:
        tol = DGRAD_TOL * max(1.0, float(np.abs(ref).max()))
        _report(what, leg, float(err.max()), tol)
        assert float(err.max()) < tol, (what, float(err.max()), tol, np.unravel_index(err.argmax(), err.shape))


@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("case", WGRAD_CASES, ids=case_id)
def test_wgrad(tables, case, leg):
    """sparse.conv_wgrad without the group masks (k_conv_wgrad) and with them (k_conv_wgrad_t where both widths are
    multiples of 16), and gf_conv_wgrad_masked_acc -- the only form the training executor calls -- twice into a dW
    that holds something."""
    from geoformer_amd import _lib, sparse
    from geoformer_amd._lib import check, ptr, stream_ptr

    name, kind, Cin, Cout = case
    T = tables(name)
    g = R.geometry(kind, T.M, T.Mc)
    K, M_out, ld = g["K"], g["rows_out"], g["ld"]
    rng = np.random.default_rng(R.seed_of("wgrad", case, leg))
    X = R.rows_operand(rng, (g["rows_in"], Cin), leg)
    G = R.rows_operand(rng, (M_out, Cout), leg)
    dW0 = R.rows_operand(rng, (K, Cin, Cout), leg)
    htbl = T.host[g["tbl"]] if g["tbl"] else None
    tbl, gm = T.dev[g["tbl"]] if g["tbl"] else (None, None)
    ref = R.wgrad_ref(X, G, htbl, K, M_out)
    x, gy = _dev(X), _dev(G)
    what = "wgrad " + case_id(case)
    lib = _lib.load()
    _check_dw(sparse.conv_wgrad(x, gy, tbl, K, M_out, ld), ref, ref, leg, what + " no mask", htbl, M_out)
    if tbl is not None:
        got = sparse.conv_wgrad(x, gy, tbl, K, M_out, ld, gmask=gm)
    else:  # a 1x1x1 convolution: no table, no masks, and still the tiled kernel
        got = torch.full((K, Cin, Cout), 7.0, device="cuda")
        check(lib.gf_conv_wgrad_masked(ptr(x), ptr(gy), None, None, K, M_out, ld, Cin, Cout, ptr(got), stream_ptr()),
              "gf_conv_wgrad_masked")
    _check_dw(got, ref, ref, leg, what + " masked", htbl, M_out)
    dW = _dev(dW0)
    for _ in range(2):
        check(lib.gf_conv_wgrad_masked_acc(ptr(x), ptr(gy), ptr(tbl), ptr(gm), K, M_out, ld, Cin, Cout, ptr(dW),
                                           stream_ptr()), "gf_conv_wgrad_masked_acc")
    _check_dw(dW, dW0.astype(np.float64) + 2 * ref, ref, leg, what + " acc x2", htbl, M_out, base=dW0)


def _exec_dgrad(T, g, gy, w, Cin, Cout, residual, out, steps, flat):
    """The input-gradient launch of gf_unet_train_bwd (csrc/unet_train.hip): transposed pack, then the forward kernel
    over the backward table with the forward's output rows as input rows."""
    from geoformer_amd import _lib
    from geoformer_amd._lib import check, ptr, stream_ptr

    lib = _lib.load()
    K = g["K"]
    wp = torch.empty(lib.gf_conv_packed_floats(K, Cout, Cin), dtype=torch.float32, device="cuda")
    check(lib.gf_conv_pack_weights_t(ptr(w), K, Cin, Cout, g["flip"], ptr(wp), stream_ptr()), "gf_conv_pack_weights_t")
    btbl, bgm = T.dev[g["btbl"]] if g["btbl"] else (None, None)
    check(lib.gf_conv_fwd_flat(ptr(gy), ptr(wp), ptr(btbl), ptr(bgm), ptr(steps), ptr(flat), K, g["rows_out"], g["rows_in"],
                               g["bld"], Cout, Cin, None, None, ptr(residual), None, None, ptr(out), None, stream_ptr()),
          "gf_conv_fwd_flat")
    return out


def _dgrad_operands(T, case, leg, tag="dgrad"):
    _, kind, Cin, Cout = case
    g = R.geometry(kind, T.M, T.Mc)
    rng = np.random.default_rng(R.seed_of(tag, case, leg))
    G = R.rows_operand(rng, (g["rows_out"], Cout), leg)
    W = R.weight_operand(rng, g["K"], Cin, Cout, leg)
    res = R.rows_operand(rng, (g["rows_in"], Cin), leg)
    ref = R.dgrad_ref(G, W, T.host[g["tbl"]] if g["tbl"] else None, g["rows_in"], g["rows_out"])
    return g, G, W, res, ref


@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("case", DGRAD_CASES, ids=case_id)
def test_dgrad(tables, case, leg):
    """sparse.conv_dgrad ("subm" with the step table where the rules have one, "table" for the strided pair and the
    1x1x1), the same with the level's flat step table, and the executor's call: with a separate residual and with
    `residual` and `out` one buffer."""
    from geoformer_amd import sparse

    name, kind, Cin, Cout = case
    T = tables(name)
    g, G, W, res, ref = _dgrad_operands(T, case, leg)
    gy, w = _dev(G), _dev(W)
    what = "dgrad " + case_id(case)
    steps = flat = None
    if kind == "subm":
        steps, flat = T.steps, T.flat
        bwd = ("subm", T.dev["nbr"] + (27, T.M, g["bld"], steps))
    else:
        bwd = ("table", (T.dev[g["btbl"]] if g["btbl"] else (None, None)) + (g["K"], g["rows_in"], g["bld"]))
    _check_dx(sparse.conv_dgrad(gy, w, bwd, g["rows_in"]), ref, ref, leg, what + " conv_dgrad")
    if flat is not None:
        _check_dx(sparse.conv_dgrad(gy, w, bwd, g["rows_in"], flat=flat), ref, ref, leg, what + " conv_dgrad flat")
    want = res.astype(np.float64) + ref
    out = torch.full((g["rows_in"], Cin), 7.0, device="cuda")
    _check_dx(_exec_dgrad(T, g, gy, w, Cin, Cout, _dev(res), out, steps, flat), want, ref, leg, what + " exec residual")
    buf = _dev(res)
    _check_dx(_exec_dgrad(T, g, gy, w, Cin, Cout, buf, buf, steps, flat), want, ref, leg, what + " exec residual == out")


@pytest.fixture(scope="module")
def mid_forced(tables):
    """`mid` with the tables the counted-loop and the LDS-weight kernels need, which its size alone does not get."""
    from geoformer_amd import sparse

    T = tables("mid")
    old_min = sparse.STEPS_MIN_ROWS
    sparse.STEPS_MIN_ROWS = 0
    try:
        rules = sparse.subm_rules(T.coords, sparse.build_index(T.coords, T.batch, T.shape))
    finally:
        sparse.STEPS_MIN_ROWS = old_min
    assert rules.steps is not None and (rules.nbr == T.rules.nbr).all()
    return rules.steps, sparse.flat_steps(T.rules.nbr, T.rules.gmask, 27, T.M, T.rules.ld)


@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("Cin,Cout", FORCED_WIDTHS)
def test_dgrad_in_place_every_family(tables, mid_forced, Cin, Cout, leg):
    """`residual` == `out` (include/geoformer_hip.h: gf_conv_fwd) under every forced launch family; a knob set whose
    family does not take the shape leaves the size-based choice, which must be right as well."""
    from geoformer_amd import sparse

    T = tables("mid")
    steps, flat = mid_forced
    case = ("mid", "subm", Cin, Cout)
    g, G, W, res, ref = _dgrad_operands(T, case, leg, tag="forced")
    gy, w = _dev(G), _dev(W)
    want = res.astype(np.float64) + ref
    try:
        for knobs in FORCED_KNOBS:
            sparse.dev_conv_knobs(**knobs)
            buf = _dev(res)
            _check_dx(_exec_dgrad(T, g, gy, w, Cin, Cout, buf, buf, steps, flat), want, ref, leg,
                      "dgrad %s in place %s" % (case_id(case), knobs))
    finally:
        sparse.dev_conv_knobs()  # back to the size-based choice
