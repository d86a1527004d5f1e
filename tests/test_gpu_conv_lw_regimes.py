"""The LDS-weight sparse convolution (csrc/spconv_lw.hip k_conv_lw) at every regime of its per-wave step stream, against
the float64 reference of tests/conv_lw_cases.py.  Every case is a hand-built neighbour table run through
gf_conv_fwd_flat with the kernel forced (lw = 1) under the case's bin count (gf_dev_conv_flat_bins): with 4 bins a few
hundred groups give every wave a stream of many groups, so group changes in mid-stream, the residual request one group
ahead, the hand-counted residual wait at both sides of its boundary, empty groups, the walk over the lanes'
descriptors and a descriptor in every lane all run in milliseconds.  What the case lists reach is proven without a GPU
by test_conv_lw_cases_host.py::test_case_lists_reach_every_regime.

Two legs per case.  Integer operands: `out` (and `out2`) must EQUAL the reference; both are pre-filled with a sentinel
and carry 16 guard rows behind M_out, so a skipped group, a stale residual register or a misplaced row fails on the
exact row.  The residual wait is a claim about latency -- a request that is D consumed steps old has landed -- so the
residual rows are made as late as a test can make them: a buffer larger than the caches is overwritten after the
residual is in place, then a launch with other output and residual buffers brings the table, the input rows and the
weights back, and the launch under test finds everything close but its residual.  Gaussian operands: 1e-4 of
max(1, max|ref|) (the bound of test_gpu_spconv_backward.py's DGRAD_TOL and of BASELINE.json's north_star), the largest
error printed (-s), and two runs that must agree bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

from tests import conv_lw_cases as C

pytestmark = pytest.mark.gpu

TOL = 1e-4  # of max(1, max|ref|)
LEGS = ["int", "gauss"]
LW = 1  # gf_dev_conv_plan's family number of k_conv_lw
GUARD = 16  # rows behind M_out that no launch may touch
SCRUB_BYTES = 1 << 30  # more than the 8 x 4 MiB of L2 and the 256 MiB behind them


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def device_tables(hip):
    """name -> (nbr, gmask, flat) on the device; the flat table is built under the table's own bin count."""
    from geoformer_amd import sparse

    cache = {}

    def get(name):
        if name not in cache:
            T = C.table(name)
            nbr, gmask = _dev(T.nbr), _dev(T.gmask.view(np.int32))
            try:
                sparse.dev_conv_flat_bins(T.nbins)
                flat = sparse.flat_steps(nbr, gmask, 27, T.M_out, T.ld)
            finally:
                sparse.dev_conv_flat_bins(0)
            # the header carries the setting the table was built under; the kernel is handed the same one below
            assert int(flat[1]) == T.nbins and int(flat[2]) == T.ngroups, (name, flat[:5].tolist())
            cache[name] = (nbr, gmask, flat)
        return cache[name]

    return get


@pytest.fixture(scope="module")
def scrub(hip):
    return torch.empty(SCRUB_BYTES // 4, dtype=torch.float32, device="cuda")


def _plan(lib, T, form, dev, x, wp, vec, res, out, out2):
    from geoformer_amd._lib import ptr

    nbr, gmask, flat = dev
    desc = (ctypes.c_int * 10)()
    rc = lib.gf_dev_conv_plan(ptr(x), ptr(wp), ptr(nbr), ptr(gmask), None, ptr(flat), 27, T.M_in, T.M_out, T.ld, form.Cin,
                              form.Cout, ptr(vec["sc"]), ptr(vec["sh"]), ptr(res), ptr(vec["osc"]), ptr(vec["osh"]),
                              ptr(out), ptr(out2), desc)
    assert rc == 0
    return list(desc)


def _run(lib, T, form, ops, dev, scrub, want_lw=True):
    """One call of gf_conv_fwd_flat for the form; returns (out, out2 or None) as numpy, guard rows checked."""
    from geoformer_amd import sparse
    from geoformer_amd._lib import check, ptr, stream_ptr

    x, W, sc, sh, res, osc, osh = ops
    nbr, gmask, flat = dev
    xd = _dev(x)
    wp = sparse.pack_weights(_dev(W))
    vec = dict(sc=_dev(sc) if form.aff else None, sh=_dev(sh) if form.aff else None,
               osc=_dev(osc) if form.act else None, osh=_dev(osh) if form.act else None)
    rows = T.M_out + GUARD
    full = torch.full((rows, form.Cout), C.SENTINEL, device="cuda")
    out = full[: T.M_out]
    full2 = torch.full((rows, form.Cout), C.SENTINEL, device="cuda") if form.out2 else None
    out2 = full2[: T.M_out] if form.out2 else None
    resd = None
    if form.res == "sep":
        resd = _dev(res)
    elif form.res == "inplace":
        out.copy_(_dev(res))
        resd = out
    plan = _plan(lib, T, form, dev, xd, wp, vec, resd, out, out2)
    if want_lw:
        ps = C.passes(form.Cin)
        assert plan[:7] == [LW, len(ps), ps[0], ps[-1], form.Cout // 16, 12, int(form.aff)] and plan[7] == T.nbins // 4, plan
    else:
        assert plan[0] != LW, plan

    def launch(resd, out, out2):
        check(lib.gf_conv_fwd_flat(ptr(xd), ptr(wp), ptr(nbr), ptr(gmask), None, ptr(flat), 27, T.M_in, T.M_out, T.ld, form.Cin,
                                   form.Cout, ptr(vec["sc"]), ptr(vec["sh"]), ptr(resd), ptr(vec["osc"]), ptr(vec["osh"]),
                                   ptr(out), ptr(out2), stream_ptr()), "gf_conv_fwd_flat")

    if resd is not None:  # the residual rows far away, everything else close (module docstring)
        other = torch.zeros((3, T.M_out, form.Cout), device="cuda")
        scrub.fill_(0.0)
        launch(other[0], other[1], other[2] if form.out2 else None)
    launch(resd, out, out2)
    torch.cuda.synchronize()
    for buf in (full, full2):
        if buf is not None:
            assert bool((buf[T.M_out:] == C.SENTINEL).all()), "rows behind M_out were written"
    return out.cpu().numpy(), (out2.cpu().numpy() if form.out2 else None)


def _compare(what, leg, got, want, ref_scale, worst):
    got = got.astype(np.float64)
    err = np.abs(got - want)
    if leg == "int":
        rows = np.unique(np.argwhere(err != 0)[:, 0])
        assert rows.size == 0, ("%s: %d of %d rows differ; first rows %s (16-row groups %s); row %d got %s, want %s"
                                % (what, rows.size, err.shape[0], rows[:8].tolist(), sorted(set((rows[:8] // 16).tolist())),
                                   rows[0], got[rows[0]][:8].tolist(), want[rows[0]][:8].tolist()))
    else:
        tol = TOL * max(1.0, ref_scale)
        worst.append(float(err.max()) if err.size else 0.0)
        assert worst[-1] < tol, (what, worst[-1], tol, np.unravel_index(err.argmax(), err.shape))


def _check_case(lib, T, form, leg, dev, scrub, want_lw=True):
    from geoformer_amd import sparse

    ops = C.operands(T, form, leg)
    want, want2 = C.expected(T, form, ops)
    scale = float(max(np.abs(want).max(), np.abs(want2).max() if want2 is not None else 0.0))
    what = "conv_lw %s %s" % (T.name, form)
    worst = []
    try:
        sparse.dev_conv_knobs(lw=1)
        sparse.dev_conv_flat_bins(T.nbins)
        got, got2 = _run(lib, T, form, ops, dev, scrub, want_lw)
        _compare(what + " out", leg, got, want, scale, worst)
        if form.out2:
            _compare(what + " out2", leg, got2, want2, scale, worst)
        if leg == "gauss":  # the hand-counted waits are where a race would show: a second run must give the same bits
            again, again2 = _run(lib, T, form, ops, dev, scrub, want_lw)
            assert (again.view(np.uint32) == got.view(np.uint32)).all(), what + ": two runs differ"
            if form.out2:
                assert (again2.view(np.uint32) == got2.view(np.uint32)).all(), what + ": two runs differ (out2)"
            print("[conv-lw] %-44s %s max|err| = %.3e  bound = %.3e"
                  % (what, sorted(C.instantiations(form)) if want_lw else "(another kernel)", max(worst), TOL * max(1.0, scale)))
    finally:
        sparse.dev_conv_knobs()
        sparse.dev_conv_flat_bins(0)


@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_conv_lw_regime(hip, device_tables, scrub, case, leg):
    T = C.table(case[0])
    _check_case(hip, T, case[1], leg, device_tables(T.name), scrub)


@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("form", C.EDGE_FORMS, ids=str)
def test_planner_leaves_the_kernel_past_64_groups_per_wave(hip, device_tables, scrub, form, leg):
    """4 bins hold 64 * 3 * 4 = 768 groups, one per lane of every wave (table full4, among the cases above).  One group
    more and the planner must pick another kernel -- checked with gf_dev_conv_plan inside _run -- whose result is the
    same reference."""
    T = C.table(C.EDGE_TABLE)
    assert T.ngroups == C.LANES * C.WPS * T.nbins + 1
    _check_case(hip, T, form, leg, device_tables(T.name), scrub, want_lw=False)


def test_mismatching_bin_count_is_rejected(hip, device_tables):
    """gf_rules_flat_steps builds tables of the current bin count only (0 or that count); the setter takes 0 or a
    multiple of 4 of at most 1024."""
    from geoformer_amd import _lib, sparse

    T = C.table("sixteen")
    nbr, gmask, _ = device_tables(T.name)
    try:
        for bad in (-4, 2, 6, 1028, 2048):
            with pytest.raises(_lib.GeoFormerHipError):
                sparse.dev_conv_flat_bins(bad)
        sparse.dev_conv_flat_bins(8)
        assert int(sparse.flat_steps(nbr, gmask, 27, T.M_out, T.ld, 8)[1]) == 8
        assert int(sparse.flat_steps(nbr, gmask, 27, T.M_out, T.ld, 0)[1]) == 8
        for other in (4, 1024):
            with pytest.raises(_lib.GeoFormerHipError):
                sparse.flat_steps(nbr, gmask, 27, T.M_out, T.ld, other)
    finally:
        sparse.dev_conv_flat_bins(0)
    assert int(sparse.flat_steps(nbr, gmask, 27, T.M_out, T.ld, 1024)[1]) == 1024
    with pytest.raises(_lib.GeoFormerHipError):
        sparse.flat_steps(nbr, gmask, 27, T.M_out, T.ld, 8)
