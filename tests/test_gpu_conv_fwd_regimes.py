"""The five forward families of csrc/spconv_conv.hip that the LDS-weight suite does not cover -- k_conv_g16p, k_conv_g16,
k_conv_pair, k_conv_os and k_conv_flat -- at every template instance and regime, against the float64 reference of
tests/conv_lw_cases.py.  Every case (tests/conv_fwd_cases.py) is a hand-built neighbour table of at most a few thousand
rows run through gf_conv_fwd_flat under the dev knobs that force its family; the step tables of k_conv_g16 / k_conv_g16p
are built in numpy with chunk boundaries set by hand and POISON wherever the device builder writes nothing.  What the
case lists reach, and that the planner sends each case to the instance it is meant for, is proven without a GPU by
test_conv_fwd_cases_host.py; every case asserts its plan here once more through gf_dev_conv_plan with the real pointers.

Two legs per case.  Integer operands: `out` (and `out2`) must EQUAL the reference; both are pre-filled with a sentinel
and carry 16 guard rows behind M_out.  Gaussian operands: 1e-4 of max(1, max|ref|) (TOL of the LDS-weight suite,
BASELINE.json's north_star), two runs that must agree bit for bit, the largest error per instance printed (-s).

test_device_built_tables has gf_rules_subm3 build step tables into pre-poisoned buffers under several chunk counts: the
step blocks and all count + 1 boundaries must equal the numpy restatement word for word (k_subm3, k_group_chunks), and
k_conv_g16p then runs its integer leg on them.

Not reachable at these sizes: grids past the 256 * 64 cap of k_conv_pair and of k_conv_os' one-wave-per-item shape (over
2 M rows), and inputs beyond the 32-bit byte offsets (4 GiB of features)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import conv_fwd_cases as F
from tests import conv_lw_cases as L
from tests.test_gpu_conv_lw_regimes import GUARD, TOL, _compare, _dev

pytestmark = pytest.mark.gpu

LEGS = ["int", "gauss"]
WORST = {}  # (family, instance) -> largest Gaussian-leg error / its bound


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for key in sorted(WORST):
        print("[conv-fwd] %-5s %-28s largest max|err| / bound = %.3e / %.3e" % (key + WORST[key]))


def _set_knobs(kn):
    from geoformer_amd import sparse

    kn = dict(kn)
    wpb, chunks = kn.pop("wpb", 0), kn.pop("chunks", 0)
    sparse.dev_conv_knobs(**kn)
    sparse.dev_conv_g16p_wpb(wpb)
    sparse.dev_conv_chunks(chunks)


@pytest.fixture(scope="module")
def device_tables(hip):
    """(table name, chunking) -> dict(nbr, gmask, steps) on the device."""
    cache = {}

    def get(c):
        key = (c.tname, c.chunks if c.family == F.G16P else ("g16" if c.steps else None))
        if key not in cache:
            T = c.table
            steps = None
            if c.steps:  # (k_conv_g16 reads the blocks only; the boundaries are there all the same)
                steps = _dev(F.step_table(T, c.bounds() if c.chunks else F.chunking("rule12", T.sizes)))
            cache[key] = dict(nbr=_dev(T.nbr), gmask=_dev(T.gmask.view(np.int32)), steps=steps)
        d = cache[key]
        return dict(nbr=d["nbr"] if c.nbr else None, gmask=d["gmask"] if c.gmask else None, steps=d["steps"])

    return get


def _run(lib, T, form, ops, dev, want_plan, misaligned=False):
    """One call of gf_conv_fwd_flat; returns (out, out2 or None) as numpy, plan and guard rows checked."""
    from geoformer_amd import sparse
    from geoformer_amd._lib import check, ptr, stream_ptr

    x, W, sc, sh, res, osc, osh = ops
    if misaligned:  # a view 4 bytes behind a 16-byte boundary
        flat = torch.zeros(x.size + 1, device="cuda")
        flat[1:].copy_(_dev(x).view(-1))
        xd = flat[1:].view(x.shape)
        assert xd.data_ptr() % 16 == 4
    else:
        xd = _dev(x)
    wp = sparse.pack_weights(_dev(W))
    v = dict(sc=_dev(sc) if form.aff else None, sh=_dev(sh) if form.aff else None,
             osc=_dev(osc) if form.act else None, osh=_dev(osh) if form.act else None)
    rows = T.M_out + GUARD
    full = torch.full((rows, form.Cout), L.SENTINEL, device="cuda")
    out = full[: T.M_out]
    full2 = torch.full((rows, form.Cout), L.SENTINEL, device="cuda") if form.out2 else None
    out2 = full2[: T.M_out] if form.out2 else None
    resd = None
    if form.res == "sep":
        resd = _dev(res)
    elif form.res == "inplace":
        out.copy_(_dev(res))
        resd = out
    args = (ptr(xd), ptr(wp), ptr(dev["nbr"]), ptr(dev["gmask"]), ptr(dev["steps"]), None, T.K, T.M_in, T.M_out, T.ld,
            form.Cin, form.Cout, ptr(v["sc"]), ptr(v["sh"]), ptr(resd), ptr(v["osc"]), ptr(v["osh"]), ptr(out), ptr(out2))
    desc = (ctypes.c_int * 10)()
    assert lib.gf_dev_conv_plan(*args, desc) == 0
    assert list(desc) == want_plan, (list(desc), want_plan)
    check(lib.gf_conv_fwd_flat(*args, stream_ptr()), "gf_conv_fwd_flat")
    torch.cuda.synchronize()
    for buf in (full, full2):
        if buf is not None:
            assert bool((buf[T.M_out:] == L.SENTINEL).all()), "rows behind M_out were written"
    return out.cpu().numpy(), (out2.cpu().numpy() if form.out2 else None)


def _check(lib, what, T, form, leg, dev, knobs, want_plan, misaligned=False):
    ops = L.operands(T, form, leg)
    want, want2 = L.expected(T, form, ops)
    scale = float(max(np.abs(want).max(), np.abs(want2).max() if want2 is not None else 0.0))
    worst = []
    try:
        _set_knobs(knobs)
        got, got2 = _run(lib, T, form, ops, dev, want_plan, misaligned)
        _compare(what + " out", leg, got, want, scale, worst)
        if form.out2:
            _compare(what + " out2", leg, got2, want2, scale, worst)
        if leg == "gauss":
            again, again2 = _run(lib, T, form, ops, dev, want_plan, misaligned)
            assert (again.view(np.uint32) == got.view(np.uint32)).all(), what + ": two runs differ"
            if form.out2:
                assert (again2.view(np.uint32) == got2.view(np.uint32)).all(), what + ": two runs differ (out2)"
            bound = TOL * max(1.0, scale)
            key = (F.FAMILY[want_plan[0]], str(want_plan[1:7]))
            if key not in WORST or max(worst) / bound > WORST[key][0] / WORST[key][1]:
                WORST[key] = (max(worst), bound)
            print("[conv-fwd] %-70s max|err| = %.3e  bound = %.3e" % (what, max(worst), bound))
    finally:
        _set_knobs({})


def _case(hip, device_tables, c, leg):
    _check(hip, c.id(), c.table, c.form, leg, device_tables(c), c.knobs, c.plan(), c.misaligned)


@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("case", F.CASES["g16p"], ids=F.case_id)
def test_g16p_regime(hip, device_tables, case, leg):
    _case(hip, device_tables, case, leg)


@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("case", F.CASES["g16"], ids=F.case_id)
def test_g16_regime(hip, device_tables, case, leg):
    _case(hip, device_tables, case, leg)


@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("case", F.CASES["pair"], ids=F.case_id)
def test_pair_regime(hip, device_tables, case, leg):
    _case(hip, device_tables, case, leg)


@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("case", F.CASES["os"], ids=F.case_id)
def test_os_regime(hip, device_tables, case, leg):
    _case(hip, device_tables, case, leg)


@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("case", F.CASES["flat"], ids=F.case_id)
def test_flat_regime(hip, device_tables, case, leg):
    """(the cases of 405 steps per item must leave the family: their plan is k_conv_os' sixteen-wave shape)"""
    _case(hip, device_tables, case, leg)


@pytest.mark.parametrize("chunks", [4, 12, 3072, 4096])
@pytest.mark.parametrize("vox", ["five", "mid", "big"])
def test_device_built_tables(hip, oracle, vox, chunks):
    from geoformer_amd import sparse
    from geoformer_amd._lib import check, ptr, stream_ptr

    coords = F.voxel_set(vox)
    M = coords.shape[0]
    ld = max(L._round16(M), 16)
    c = _dev(coords)
    index = sparse.build_index(c, 1, F.VOXEL_SHAPE)
    nbr = torch.empty((27, ld), dtype=torch.int32, device="cuda")
    gmask = torch.empty(ld // 16, dtype=torch.int32, device="cuda")
    before = F.poison_buffer(ld, M)
    assert before.size == hip.gf_rules_steps_words(ld)
    steps = _dev(before)
    X, Y, Z = F.VOXEL_SHAPE
    try:
        sparse.dev_conv_chunks(chunks)
        check(hip.gf_rules_subm3(ptr(c), M, None, X, Y, Z, ptr(index.bitmap), ptr(index.prefix), ptr(index.perm), ptr(nbr), ld,
                                 ptr(gmask), ptr(steps), stream_ptr()), "gf_rules_subm3")
    finally:
        sparse.dev_conv_chunks(0)
    nbr_h = nbr.cpu().numpy()
    assert (nbr_h == oracle.rules_subm3(coords, F.VOXEL_SHAPE)).all()
    masks = L.group_masks(nbr_h, M)
    sizes = np.array([bin(int(m)).count("1") for m in masks])
    T = L.Table("built-%s-%d" % (vox, chunks), 0, M, M, nbr_h, sizes)
    assert (gmask.cpu().numpy().view(np.uint32) == T.gmask).all()
    if vox == "big":
        assert M > 16384 and T.ngroups > 1024 and {1, 3, 9, 27} <= set(sizes.tolist())
    bounds = F.group_chunks(sizes, chunks)
    want = F.step_table(T, bounds)
    got = steps.cpu().numpy()
    nblk = (ld // 16) * F.STEP_BLKS * 64
    bad = np.nonzero(got[:nblk] != want[:nblk])[0]
    assert bad.size == 0, ("step blocks differ at (group, block) %s" % sorted({(int(w) // 448, int(w) % 448 // 64) for w in bad[:8]}))
    bad = np.nonzero(got[nblk:] != want[nblk:])[0]
    assert bad.size == 0, ("tail words differ at %s: got %s, want %s (count %d: words 1 .. %d are boundaries, the rest "
                           "must keep what the buffer held)" % (bad[:8].tolist(), got[nblk:][bad[:8]].tolist(),
                                                                want[nblk:][bad[:8]].tolist(), chunks, chunks + 1))
    dev = dict(nbr=nbr, gmask=gmask, steps=steps)
    for nch, wpb, ldsw, form in [(1, 12 if chunks % 12 == 0 else 8, 1, L.Form(16, 16, 1, "sep", 1, out2=True)),
                                 (2, 4 if chunks % 12 == 0 else 16, chunks != 12, L.Form(32, 16, 1, "inplace", 0))]:
        plan = [F.G16P, nch, int(ldsw), wpb, 1, 1, 0, F._ceil(F.CHUNKS_MAX, wpb), 64 * wpb, 27 * nch * 1024 * int(ldsw)]
        _check(hip, "%s %s wpb %d" % (T.name, form, wpb), T, form, "int", dev,
               dict(F.G16P_KNOBS, g16_ldsw=int(ldsw), wpb=wpb), plan)
