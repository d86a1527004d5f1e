"""The sparse convolution's launch planner (gf_dev_conv_plan, spconv_conv.hip conv_plan) against a Python restatement of
the selection rules it replaced: conv_fwd_impl, gf_conv_lw_supported, launch_g16p and gf_conv_dual_supported as they
stood before the planner.  No GPU: the planner never dereferences the (fake) pointers it is given."""
import ctypes
import itertools

import numpy as np
import pytest

from tests.test_host_logic import lib  # noqa: F401  (the library, built for gfx950 if missing)

OK, INVALID = 0, -1
NONE, LW, FLAT, G16P, G16, PAIR, OS = range(7)
FAMILY = ["none", "lw", "flat", "g16p", "g16", "pair", "os"]
DEFAULT_KNOBS = dict(split=-1, wide=-1, pair=-1, block=0, g16=-1, g16_ldsw=-1, g16_gpw=0, g16_pipe=-1, flat=-1,
                     flat_items=0, lw=-1, lw_items=0, wpb=0, chunks=0, bins=0)


def _tri(v):
    return -1 if v < 0 else int(v != 0)


def _norm(kn):
    """The knob setters' normalisation (gf_dev_conv_knobs*, gf_dev_conv_knob_flat / _lw, _g16p_wpb, _chunks, _flat_bins)."""
    k = dict(DEFAULT_KNOBS, **kn)
    for n in ("split", "wide", "pair", "g16", "g16_ldsw", "g16_pipe", "flat", "lw"):
        k[n] = _tri(k[n])
    k["block"] = 0 if k["block"] <= 0 else min(k["block"], 256)
    for n in ("g16_gpw", "flat_items", "lw_items"):
        k[n] = max(k[n], 0)
    k["chunks"] = k["chunks"] if k["chunks"] > 0 else 3072
    k["bins"] = k["bins"] or 1024  # bins of the flat step table: a wave of k_conv_lw keeps at most 64 groups of its bin
    return k


def head_plan(q, kn):
    """(status, [family, p0..p5, grid, block, lds]) of one gf_conv_fwd_flat call as the dispatch chose it before the
    planner.  q: sizes, which tables / operands are present and which pointers are 16-byte aligned."""
    kn = _norm(kn)
    K, M_in, M_out, ld, Cin, Cout = q["K"], q["M_in"], q["M_out"], q["ld"], q["Cin"], q["Cout"]
    sc, res, out2, osc = q["sc"], q["res"], q["out2"], q["osc"]
    al = q["aligned"]  # in, sc (scale | shift), out, res, out2, osc (scale | shift)
    # gf_conv_fwd_flat, then conv_fwd_impl's argument checks
    if out2 and not (osc and al["out2"]):
        return INVALID, None
    if not (1 <= K <= 32) or Cin < 1 or Cout < 1 or (sc and Cin > 512 - 16):
        return INVALID, None
    if Cin > 512:  # CONV_MAX_CIN, with or without a prologue: what keeps the kernels' reciprocal step division exact
        return INVALID, None
    if not (q["nbr"] or q["steps"] or K == 1):
        return INVALID, None
    if osc and not al["osc"]:
        return INVALID, None
    if M_out <= 0:
        return OK, [NONE] + [0] * 9
    ngroups = (M_out + 15) // 16
    ncb, nch = (Cout + 15) // 16, (Cin + 15) // 16
    in_bytes64 = M_in * Cin * 4
    vec = Cin % 16 == 0 and al["in"] and in_bytes64 < 0xFFFFFFF0 and (not sc or al["sc"])
    split = ngroups < 6000 if kn["split"] < 0 else kn["split"] != 0
    wide = split and (ngroups * ncb <= 256 if kn["wide"] < 0 else kn["wide"] != 0)
    flat_ok = vec and nch <= 16 and K * nch <= 16 * 4 * 6 and in_bytes64 < 0xFFFFFFF0
    if kn["flat"] < 0:
        flat = flat_ok and split and ngroups * ncb <= (kn["flat_items"] or 256)
    else:
        flat = flat_ok and kn["flat"] != 0
    ncbw = (2 if not wide and ncb >= 2 and ngroups >= 2048 else 1) if split else min(ncb, 8)
    nitems = ngroups * ((ncb + ncbw - 1) // ncbw)
    block = kn["block"] or 256
    blocks = min(nitems if split else (nitems + block // 64 - 1) // (block // 64), 256 * 64)
    wbytes = K * nch * ncb * 1024
    g16 = (q["steps"] and q["gmask"] and vec and Cout == 16 and nch <= 2 and al["out"] and (not res or al["res"])
           and in_bytes64 <= 0xFFFFFF00)
    g16 = g16 and (kn["g16"] != 0 if kn["g16"] >= 0 else not split)
    # gf_conv_lw_supported, given a flat table
    if q["flat"] and q["gmask"]:
        aligned = vec and al["out"] and (not res or al["res"]) and (not out2 or al["out2"]) and (not osc or al["osc"])
        forced = kn["lw"] == 1
        lw = kn["lw"] != 0 and aligned and K == 27 and Cin % 16 == 0 and Cout % 16 == 0
        if lw:
            npass = (nch + 1) // 2
            shape = lambda n: n in (1, 2) and ncb in (1, 2)  # noqa: E731
            lw = shape((nch + npass - 1) // npass) and shape(nch // npass)
            lw = lw and M_in < (1 << 24) and M_in * Cin * 4 <= (1 << 30) - 4096 and ngroups <= 64 * 3 * kn["bins"]
            lw = lw and (forced or (npass == 1 and nch == 2 and ngroups >= (kn["lw_items"] or 1500)))
        if lw and (forced or not (g16 and nch == 1)):
            rest, ns = nch, []  # input chunks per pass: ceil(rest / passes left)
            for p in range(npass):
                ns.append((rest + (npass - p) - 1) // (npass - p))
                rest -= ns[-1]
            return OK, [LW, npass, ns[0], ns[-1], ncb, 12, int(sc), kn["bins"] // 4, 64 * 12, 27 * ns[0] * ncb * 1024]
    if flat and (q["nbr"] or K == 1) and not out2:
        maxb = 4 if K * nch <= 16 * 4 * 4 else 6
        return OK, [FLAT, maxb, 0, 0, 0, 0, 0, ngroups * ncb, 1024, 0]
    if g16:
        gl = wbytes <= 64 * 1024 and (kn["g16_ldsw"] < 0 or kn["g16_ldsw"] != 0)
        pipe = (ld // 16) * 7 * 256 < 0xFFFFF000 and ld >= M_out and (kn["g16_pipe"] < 0 or kn["g16_pipe"] != 0)
        lds = wbytes if gl else 0
        if pipe:
            wpb = kn["wpb"] or (12 if nch == 1 and kn["chunks"] % 12 == 0 else 4)
            return OK, [G16P, nch, int(gl), wpb, int(sc), int(res), 0, (4096 + wpb - 1) // wpb, 64 * wpb, lds]
        if out2:
            return INVALID, None
        gpw = kn["g16_gpw"] or (2 if gl else 1)
        return OK, [G16, nch, int(gl), gpw, int(sc), int(res), 0, (ngroups + 4 * gpw - 1) // (4 * gpw), 256, lds]
    if out2 or not (q["nbr"] or K == 1):
        return INVALID, None
    pair = not split and vec and ncb == 1 and q["nbr"] and K <= 32 and nch <= 8 and in_bytes64 <= 0xFFFFF000 - 4096
    pair = pair and (kn["pair"] < 0 or kn["pair"] != 0)
    if pair:
        return OK, [PAIR, int(sc), 0, 0, 0, 0, 0, min(((ngroups + 1) // 2 + 3) // 4, 256 * 64), 256, 0]
    if split and wide:
        return OK, [OS, 1, 16, int(vec), 0, 0, 0, blocks, 1024, 0]
    if split:
        return OK, [OS, ncbw, 4, int(vec), 0, 0, 0, blocks, 256, 0]
    return OK, [OS, ncbw, 0, int(vec), 0, 0, 0, blocks, block, 0]


def head_dual_supported(M_out, ld, Cin, Cout, has_steps, kn):
    """gf_conv_dual_supported before the planner (its own copy of the rules: no alignment, in_bytes or step-table limits)."""
    kn = _norm(kn)
    split = (M_out + 15) // 16 < 6000 if kn["split"] < 0 else kn["split"] != 0
    g16 = has_steps and Cout == 16 and Cin in (16, 32) and (kn["g16"] != 0 if kn["g16"] >= 0 else not split)
    return int(g16 and M_out > 0 and ld >= M_out and (kn["g16_pipe"] < 0 or kn["g16_pipe"] != 0))


def _set_knobs(lib, kn):
    k = dict(DEFAULT_KNOBS, **kn)
    assert lib.gf_dev_conv_knobs(k["split"], k["wide"], k["pair"], 0, k["block"]) == 0
    assert lib.gf_dev_conv_knobs_g16(k["g16"], k["g16_ldsw"], k["g16_gpw"], k["g16_pipe"]) == 0
    assert lib.gf_dev_conv_knob_flat(k["flat"], k["flat_items"]) == 0
    assert lib.gf_dev_conv_knob_lw(k["lw"], k["lw_items"]) == 0
    assert lib.gf_dev_conv_g16p_wpb(k["wpb"]) == 0
    assert lib.gf_dev_conv_chunks(k["chunks"]) == 0
    assert lib.gf_dev_conv_flat_bins(k["bins"]) == 0


# the shapes test_gpu_fullsize.py::test_every_launch_shape_forced forces, the LDS-weight kernel's knob and the rest
FORCED = [dict(split=0, pair=1, g16=0), dict(split=0, pair=0, g16=0), dict(split=1, wide=0, g16=0),
          dict(split=1, wide=1, g16=0), dict(split=0, pair=0, block=64, g16=0), dict(split=0, pair=0, block=128, g16=0),
          dict(g16=1, g16_ldsw=0, g16_pipe=0), dict(g16=1, g16_ldsw=1, g16_pipe=0, g16_gpw=3),
          dict(g16=1, g16_ldsw=0, g16_pipe=1), dict(g16=1, g16_ldsw=1, g16_pipe=1)]
KNOB_SETS = ([{}] + [dict(k, flat=0) for k in FORCED] + [dict(flat=1), dict(flat=-1, flat_items=1000)]
             + [dict(lw=1), dict(lw=0), dict(lw_items=100), dict(lw_items=3000), dict(wpb=8), dict(wpb=16),
                dict(chunks=2048), dict(chunks=4096), dict(block=300), dict(block=100, split=0, g16=0, pair=0),
                dict(bins=4), dict(bins=4, lw=1), dict(bins=64), dict(bins=64, lw=1), dict(bins=64, lw_items=100)])
CHANNELS = [6, 16, 19, 21, 32, 48, 64, 96, 112, 224]
# 16-row groups on both sides of every size threshold: 6000 (split), 256 items (wide / flat), 2048 (two column blocks
# per wave), 1500 (LDS-weight kernel), 128 / 129 (256 items at two column blocks), one group, none; the LDS-weight
# kernel's capacity of 64 groups per wave at 4, 64 and 1024 bins
GROUPS = [0, 1, 100, 128, 129, 256, 257, 1499, 1500, 2047, 2048, 5999, 6000, 12_000, 64 * 3 * 1024, 64 * 3 * 1024 + 1,
          64 * 3 * 4, 64 * 3 * 4 + 1, 64 * 3 * 64, 64 * 3 * 64 + 1]
BASE = 1 << 20  # fake device addresses: 16-byte aligned, +4 = misaligned
ALIGN_KEYS = ["in", "sc", "out", "res", "out2", "osc"]


def _case(rng):
    ng = int(rng.choice(GROUPS))
    M_out = max(ng * 16 - int(rng.integers(0, 16)), 0) if ng else int(rng.choice([0, -1]))
    big = rng.random() < 0.08  # inputs beyond the 32-bit byte offsets / the LDS-weight kernel's 2^30 / the step table
    M_in = int(rng.choice([M_out, 3 * M_out + 5, 1 << 24, 70_000_000])) if big else max(M_out, 1)
    ld = (M_out + 15) // 16 * 16
    if big and rng.random() < 0.5:
        ld = int(rng.choice([40_000_000, 0x0FFFFFF0 // 7 * 16]))  # the step table's 4 GiB limit sits at ld ~ 38.3 M
    elif rng.random() < 0.05:
        ld = max(ld - 16, 0)  # ld < M_out: no pipelined kernel
    q = dict(K=int(rng.choice([1, 8, 27, 27, 27, 33])), M_in=M_in, M_out=M_out, ld=ld,
             Cin=int(rng.choice(CHANNELS + [16, 32] * 3 + [500])), Cout=int(rng.choice(CHANNELS + [16, 32] * 4)))
    for t in ("nbr", "gmask", "steps", "flat"):
        q[t] = bool(rng.random() < 0.75)
    for t in ("sc", "res", "osc"):
        q[t] = bool(rng.random() < 0.5)
    q["out2"] = bool(rng.random() < 0.2)
    q["osc"] = q["osc"] or (q["out2"] and rng.random() < 0.9)
    q["aligned"] = {k: True for k in ALIGN_KEYS}
    if rng.random() < 0.2:
        q["aligned"][str(rng.choice(ALIGN_KEYS))] = False
    return q


def _call(lib, q, desc):
    def p(name, present=True):
        if not present:
            return None
        return BASE * (1 + ALIGN_KEYS.index(name) if name in ALIGN_KEYS else 9) + (0 if q["aligned"].get(name, True) else 4)

    return lib.gf_dev_conv_plan(p("in"), BASE * 10, p("nbr", q["nbr"]), p("gmask", q["gmask"]), p("steps", q["steps"]),
                                p("flat", q["flat"]), q["K"], q["M_in"], q["M_out"], q["ld"], q["Cin"], q["Cout"],
                                p("sc", q["sc"]), p("sc", q["sc"]), p("res", q["res"]), p("osc", q["osc"]),
                                p("osc", q["osc"]), p("out"), p("out2", q["out2"]), desc)


@pytest.mark.parametrize("ki", range(len(KNOB_SETS)), ids=[str(k or "size-based") for k in KNOB_SETS])
def test_plan_matches_head_rules(lib, ki):  # noqa: F811
    kn = KNOB_SETS[ki]
    rng = np.random.default_rng(1000 + ki)
    desc = (ctypes.c_int * 10)()
    seen = set()
    try:
        _set_knobs(lib, kn)
        for i in range(8000):
            q = _case(rng)
            want_rc, want = head_plan(q, kn)
            got_rc = _call(lib, q, desc)
            assert got_rc == want_rc, (i, q, want)
            if want_rc == OK:
                assert list(desc) == want, (i, q, FAMILY[want[0]])
                seen.add(want[0])
            else:
                seen.add("error")
    finally:
        _set_knobs(lib, {})
    assert len(seen) >= 3, seen  # (every knob set reaches several launch shapes)


def test_plan_reaches_every_shape(lib):  # noqa: F811
    """The sweep above is random; every launch shape, every instance and the errors are also hit on purpose."""
    al = {k: True for k in ALIGN_KEYS}
    tabs = dict(nbr=True, gmask=True, steps=True, flat=True)
    off = dict(sc=False, res=False, out2=False, osc=False)

    def q(ng, Cin, Cout, K=27, **kw):
        return dict(dict(dict(K=K, M_in=ng * 16, M_out=ng * 16, ld=ng * 16, Cin=Cin, Cout=Cout, aligned=al), **tabs),
                    **dict(off, **kw))

    cases = [({}, q(10_000, 32, 32), LW), ({}, q(10_000, 32, 16), LW), ({"lw": 1}, q(10_000, 64, 32), LW),
             ({"lw": 1}, q(10_000, 16, 32), LW), ({"lw": 1}, q(10_000, 48, 32), LW),
             ({}, q(100, 32, 32), FLAT), ({}, q(10, 224, 112), FLAT),
             ({}, q(10_000, 16, 16), G16P), ({}, q(10_000, 16, 16, sc=True, res=True), G16P),
             ({"chunks": 2048}, q(10_000, 16, 16), G16P), ({}, q(10_000, 32, 16, flat=False), G16P), ({"lw": 1}, q(10_000, 16, 16), LW),
             ({"g16_pipe": 0}, q(10_000, 16, 16), G16), ({"g16_pipe": 0, "g16_ldsw": 0}, q(10_000, 32, 16, flat=False), G16),
             ({"g16": 0}, q(10_000, 16, 16, flat=False), PAIR), ({"g16": 0}, q(10_000, 16, 16, flat=False, sc=True), PAIR),
             ({}, q(10_000, 64, 64, flat=False), OS), ({}, q(3000, 64, 64, flat=False), OS), ({}, q(200, 19, 21), OS), ({}, q(100, 19, 21), OS),
             ({"block": 64, "split": 0, "g16": 0, "pair": 0}, q(100, 48, 224, flat=False), OS),
             # the capacity edge of the LDS-weight kernel: 64 groups per wave, three waves per bin
             ({}, q(64 * 3 * 1024, 32, 32), LW), ({}, q(64 * 3 * 1024 + 1, 32, 32), OS),
             ({"bins": 4, "lw": 1}, q(768, 32, 32), LW), ({"bins": 4, "lw": 1}, q(769, 32, 32), OS),
             ({"bins": 64}, q(12_288, 32, 32), LW), ({"bins": 64}, q(12_289, 32, 32), OS),
             ({"bins": 64, "lw": 1}, q(12_288, 112, 16, sc=True), LW), ({"bins": 64, "lw": 1}, q(12_289, 112, 16, sc=True), PAIR),
             # the widest input: 512 channels, 496 with a prologue
             ({}, q(100, 512, 32, flat=False), OS), ({}, q(100, 513, 32, flat=False), "error"),
             ({}, q(100, 816, 32, flat=False), "error"), ({}, q(10_000, 528, 16, flat=False), "error"),
             ({}, q(100, 496, 32, flat=False, sc=True), OS), ({}, q(100, 512, 32, flat=False, sc=True), "error"),
             ({}, q(10_000, 16, 16, steps=False, out2=True, osc=True, flat=False), "error"),
             ({}, q(10_000, 64, 64, nbr=False, steps=False, flat=False), "error")]
    desc = (ctypes.c_int * 10)()
    try:
        for kn, qq, fam in cases:
            _set_knobs(lib, kn)
            rc, want = head_plan(qq, kn)
            assert (FAMILY[want[0]] if rc == OK else "error") == (FAMILY[fam] if fam != "error" else fam), (kn, qq, want)
            assert _call(lib, qq, desc) == rc
            if rc == OK:
                assert list(desc) == want, (kn, qq)
    finally:
        _set_knobs(lib, {})


def test_dual_supported_asks_the_planner(lib):  # noqa: F811
    """gf_conv_dual_supported is the planner's answer for a level-1 call with a second output (K = 27, M_in = M_out,
    aligned pointers, no flat table); it agrees with the rules it replaced except beyond the step table's and the
    input's 32-bit limits, where those answered 1 for a call that then failed."""
    rng = np.random.default_rng(7)
    try:
        for kn in KNOB_SETS:
            _set_knobs(lib, kn)
            for ng, Cin, Cout, has_steps in itertools.product(GROUPS + [2_500_000, 4_300_000], [16, 32, 48, 6], [16, 32],
                                                              [0, 1]):
                M_out = max(ng * 16 - int(rng.integers(0, 16)), 0)
                for ld in {(M_out + 15) // 16 * 16, max(M_out - 16, 0), 40_000_000}:
                    q = dict(K=27, M_in=M_out, M_out=M_out, ld=ld, Cin=Cin, Cout=Cout, nbr=True, gmask=True,
                             steps=bool(has_steps), flat=False, sc=False, res=True, out2=True, osc=True,
                             aligned={k: True for k in ALIGN_KEYS})
                    planned = int(M_out > 0 and head_plan(q, kn)[0] == OK)
                    got = lib.gf_conv_dual_supported(M_out, ld, Cin, Cout, has_steps)
                    assert got == planned, (kn, M_out, ld, Cin, Cout, has_steps)
                    old = head_dual_supported(M_out, ld, Cin, Cout, has_steps, kn)
                    beyond = (ld // 16) * 7 * 256 >= 0xFFFFF000 or M_out * Cin * 4 > 0xFFFFFF00
                    assert got == old or (old == 1 and got == 0 and beyond), (kn, M_out, ld, Cin, Cout, has_steps)
    finally:
        _set_knobs(lib, {})
