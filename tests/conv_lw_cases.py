"""What test_conv_lw_cases_host.py, test_gpu_conv_lw_regimes.py and test_gpu_spconv.py share: the flat step table
(csrc/common.h GF_FLAT_*) restated in numpy, hand-built [27, ld] neighbour tables whose 16-row groups have prescribed
numbers of present offsets, the float64 forward reference of the LDS-weight convolution (csrc/spconv_lw.hip k_conv_lw),
the operands of the two legs and the case lists.

The kernel's bookkeeping is per WAVE: wave t (of three) of bin b takes the groups the table dealt to (round t, t + 3,
..., bin b), one descriptor per lane, and walks their step records as one stream with a ring of D gathers and D index
records in flight across the group boundaries; residual rows are requested one group ahead and awaited by a count of
consumed steps (`since < D`).  So a case is a table together with a bin count (dev knob gf_dev_conv_flat_bins): with a
few bins a table of a few hundred groups gives every wave a stream of many groups.  `wave_streams` yields each wave's
stream of group sizes from the restatement alone; the host test proves from it that the lists below reach every
regime.

Integer leg: sums of products of small integers are exact in fp32 in any order while every partial sum stays below
2^24 (asserted on the host), so the kernel's result must EQUAL the reference.  Gaussian leg: the same against a bound."""
import functools
import math
import zlib

import numpy as np

K = 27
WPS = 3  # waves per SIMD of k_conv_lw (GF_LW_WPB / 4): round j of a bin goes to wave j % WPS
LANES = 64  # a wave keeps one group descriptor per lane
BINS_DEFAULT = 1024  # GF_FLAT_BINS
FLAT_PAD = 32  # GF_FLAT_PAD: records of -1 behind the last step
X_LIM, W_LIM, RES_LIM = 3, 2, 3  # integer leg: features / weights / residual
SC_VALUES, SH_LIM = (1, 2), 3  # integer leg: prologue and epilogue scales, shifts in [-SH_LIM, SH_LIM]
SENTINEL = 7777.0  # what `out` and `out2` hold before the call (and rows behind M_out keep)


def _round16(n):
    return (int(n) + 15) // 16 * 16


def seed_of(*parts):
    return zlib.crc32(repr(parts).encode())


# ---------------------------------------------------------------------------------------------------------------
# the flat step table, restated
# ---------------------------------------------------------------------------------------------------------------
def group_masks(nbr, M):
    """Bit k of group g: any of the group's 16 rows (below M) has a neighbour at offset k."""
    nk = nbr.shape[0]
    ng = (M + 15) // 16
    pad = np.full((nk, ng * 16), -1, np.int32)
    pad[:, :M] = nbr[:, :M]
    present = (pad >= 0).reshape(nk, ng, 16).any(2)
    return (present * (1 << np.arange(nk, dtype=np.int64))[:, None]).sum(0).astype(np.uint32)


def flat_reference(nbr, M, K=27):
    """The table's step records: per 16-row group the present offsets, ascending; (records [S, 16], first step of
    every group [groups + 1], offset masks)."""
    ng = (M + 15) // 16
    pad = np.full((K, ng * 16), -1, np.int32)
    pad[:, :M] = nbr[:K, :M]
    recs, goff, masks = [], [0], []
    for g in range(ng):
        blk = pad[:, g * 16:(g + 1) * 16]
        ks = [k for k in range(K) if (blk[k] >= 0).any()]
        masks.append(sum(1 << k for k in ks))
        recs += [blk[k] for k in ks]
        goff.append(goff[-1] + len(ks))
    return np.array(recs, np.int32).reshape(-1, 16), np.array(goff), np.array(masks, np.uint32)


def flat_layout(ngroups, nbins, S):
    """Word offsets of the table's parts: (descriptors, step records, end) -- gf_flat_desc_at / gf_flat_steps_at."""
    d_at = (128 + 2 * ngroups + 1 + 63) // 64 * 64
    rounds = (ngroups + nbins - 1) // nbins
    s_at = d_at + (rounds + 1) * nbins * 4
    return d_at, s_at, s_at + (S + FLAT_PAD) * 16


def snake_slots(ngroups, nbins):
    """(round, bin) of every sorted position: round j runs over the bins forwards (j even) or backwards (j odd)."""
    p = np.arange(ngroups)
    j, x = p // nbins, p % nbins
    return j, np.where(j % 2 == 1, nbins - 1 - x, x)


def sorted_order(desc):
    """The descriptor rows [rounds + 1, nbins, 4] of a built table in the order of the sorted positions."""
    return np.concatenate([desc[j] if j % 2 == 0 else desc[j, ::-1] for j in range(desc.shape[0])])


def wave_streams(sizes, nbins):
    """The dealing: groups sorted by size (descending), dealt to the bins in snake order, round j of a bin to its wave
    j % WPS.  Returns {(bin, wave): [group sizes in the order the wave walks them]} for EVERY wave of the launch
    (nbins / 4 workgroups of 4 bins x WPS waves), idle ones included.  Groups of equal size are interchangeable, so the
    streams of sizes do not depend on how the builder orders them."""
    s = np.sort(np.asarray(sizes, np.int64))[::-1]
    rnd, b = snake_slots(s.size, nbins)
    streams = {(bb, t): [] for bb in range(nbins) for t in range(WPS)}
    for p in range(s.size):  # (ascending rounds: lane j // WPS of the wave)
        streams[(int(b[p]), int(rnd[p]) % WPS)].append(int(s[p]))
    return streams


# ---------------------------------------------------------------------------------------------------------------
# the launches of one call (gf_conv_lw)
# ---------------------------------------------------------------------------------------------------------------
def passes(Cin):
    """Input chunks (of 16 channels) per pass: wide inputs go through several passes of one or two chunks."""
    nch = Cin // 16
    npass = (nch + 1) // 2
    out, rest = [], nch
    for p in range(npass):
        out.append((rest + (npass - p) - 1) // (npass - p))
        rest -= out[-1]
    return out


def ring_depth(nch, ncb):
    """D: gathers (and index records) in flight, lw_launch's choice."""
    return 6 if nch == 2 and ncb == 2 else 8


def instantiations(form):
    """{(NCH, NCB, D, AFF)} of k_conv_lw<27, NCH, NCB, D, AFF, 12> a form's call launches."""
    ncb = form.Cout // 16
    return {(n, ncb, ring_depth(n, ncb), int(form.aff)) for n in passes(form.Cin)}


# ---------------------------------------------------------------------------------------------------------------
# hand-built tables
# ---------------------------------------------------------------------------------------------------------------
class Table:
    """name, bins the case runs under, M_in, M_out, ld, nbr int32 [27, ld], gmask uint32 [ld / 16], sizes [groups]."""

    def __init__(self, name, nbins, M_in, M_out, nbr, sizes):
        self.name, self.nbins, self.M_in, self.M_out = name, nbins, M_in, M_out
        self.nbr, self.ld, self.K = nbr, nbr.shape[1], nbr.shape[0]  # (K offsets: 27 here, 8 / 1 in conv_fwd_cases.py)
        self.ngroups = (M_out + 15) // 16
        self.gmask = np.zeros(self.ld // 16, np.uint32)
        self.gmask[: self.ngroups] = group_masks(nbr, M_out)
        self.sizes = np.array([bin(int(m)).count("1") for m in self.gmask[: self.ngroups]])
        assert (self.sizes == np.asarray(sizes)).all(), (name, self.sizes, sizes)

    def streams(self):
        return wave_streams(self.sizes, self.nbins)


def build_table(name, nbins, sizes, M_out=None, M_in=None, absent=0.3, shuffle=True, K=K):
    """A [K, ld] table whose group g has sizes[g] present offsets (in table order after an optional shuffle of
    `sizes`, so that the builder's sort has work to do).  A present offset's rows are random in [0, M_in) or, with
    probability `absent`, -1 -- but at least one of the group's rows below M_out has a neighbour (else the offset would
    not be present).  An entry of `sizes` may also be a tuple: exactly THESE offsets are the group's present ones."""
    rng = np.random.default_rng(seed_of("table", name))
    given = {}
    if any(isinstance(n, tuple) for n in sizes):  # prescribed offsets travel with their group through the shuffle
        spec = list(sizes)
        if shuffle:
            spec = [spec[i] for i in rng.permutation(len(spec) - 1)] + [spec[-1]]
        given = {g: sorted(n) for g, n in enumerate(spec) if isinstance(n, tuple)}
        sizes, shuffle = [len(n) if isinstance(n, tuple) else n for n in spec], False
    sizes = np.array(sizes, np.int64)
    if shuffle:
        last = sizes[-1]  # (the last group may be partial: it keeps its place)
        head = sizes[:-1].copy()
        rng.shuffle(head)
        sizes = np.concatenate([head, [last]])
    ng = sizes.size
    M_out = ng * 16 if M_out is None else M_out
    assert (M_out + 15) // 16 == ng
    M_in = M_out if M_in is None else M_in
    ld = max(_round16(M_out), 16)
    nbr = np.full((K, ld), -1, np.int32)
    for g in range(ng):
        valid = min(16, M_out - 16 * g)
        for k in (given[g] if g in given else rng.choice(K, int(sizes[g]), replace=False)):
            rows = rng.integers(0, M_in, valid).astype(np.int32)
            gone = rng.random(valid) < absent
            gone[rng.integers(0, valid)] = False
            nbr[k, 16 * g:16 * g + valid] = np.where(gone, -1, rows)
    return Table(name, nbins, M_in, M_out, nbr, sizes)


def _rounds(nbins, per_round, last=None):
    """Sizes of a table whose round j consists of nbins groups of per_round[j] offsets each (the last round of `last`
    groups): with sizes non-increasing, wave t of EVERY bin then walks per_round[t], per_round[t + 3], ..."""
    assert list(per_round) == sorted(per_round, reverse=True)
    out = []
    for j, n in enumerate(per_round):
        out += [n] * (last if last is not None and j == len(per_round) - 1 else nbins)
    return out


@functools.lru_cache(maxsize=None)
def table(name):
    rng = np.random.default_rng(seed_of("sizes", name))
    if name == "single28":  # one launch, 27 busy waves of ONE group with 27 ... 1 steps; bin 27 and two waves of every bin idle
        return build_table(name, 28, list(range(27, 0, -1)))
    if name == "s4a":  # wave 0: 9 8 5 3 1 / wave 1: 8 7 5 2 0 / wave 2: 8 6 4 1 0 (D = 8: first D + 1, D; later D, D - 1)
        return build_table(name, 4, _rounds(4, [9, 8, 8, 8, 7, 6, 5, 5, 4, 3, 2, 1, 1, 0, 0]))
    if name == "s4b":  # wave 0: 7 6 0 0 / wave 1: 6 5 0 0 / wave 2: 6 0 0 (D = 6: first D + 1, D; later D, D - 1); ragged end
        return build_table(name, 4, _rounds(4, [7, 6, 6, 6, 5, 0, 0, 0, 0, 0, 0], last=2), M_out=42 * 16 - 9, M_in=500)
    if name == "s4c":  # two groups per wave: 27 12 / 20 3 / 13 1
        return build_table(name, 4, _rounds(4, [27, 20, 13, 12, 3, 1]), M_in=77)
    if name == "s4d":  # a busy wave beside waves whose groups are all empty: 3 0 / 0 0 / 0
        return build_table(name, 4, _rounds(4, [3, 0, 0, 0, 0]))
    if name == "e4":  # a table without any neighbour: every stream starts (and ends) with empty groups
        return build_table(name, 4, [0] * 21, M_out=21 * 16 - 5, M_in=40)
    if name == "r8":  # random sizes over 8 bins, last round partial, last group partial
        return build_table(name, 8, rng.integers(0, 28, 59).tolist(), M_out=59 * 16 - 13, M_in=1200)
    if name == "few64":  # more bins than groups: 13 of the 16 workgroups idle
        return build_table(name, 64, rng.integers(1, 28, 10).tolist(), M_out=10 * 16 - 1, M_in=64)
    if name == "r64":  # three rounds over 64 bins (the odd one backwards), one group per wave
        return build_table(name, 64, rng.integers(0, 28, 150).tolist(), M_out=150 * 16 - 7)
    if name == "r1024":  # the default bin count on a small table: 256 workgroups, most of them idle
        return build_table(name, 1024, rng.integers(0, 28, 40).tolist(), M_out=40 * 16 - 3, M_in=333)
    if name == "one":  # a single output row
        return build_table(name, 1024, [5], M_out=1, M_in=9)
    if name == "sixteen":  # one full group
        return build_table(name, 4, [8], M_out=16, M_in=16)
    if name == "full4":  # 64 * 3 * 4 groups: a descriptor in every lane of every wave
        return build_table(name, 4, rng.integers(0, 28, 768).tolist(), M_out=768 * 16)
    if name == "over4":  # one group more than the waves' lanes hold: the planner must not take the LDS-weight kernel
        return build_table(name, 4, rng.integers(0, 28, 769).tolist(), M_out=768 * 16 + 1)
    raise KeyError(name)


TABLES = ["single28", "s4a", "s4b", "s4c", "s4d", "e4", "r8", "few64", "r64", "r1024", "one", "sixteen", "full4"]
EDGE_TABLE = "over4"


# ---------------------------------------------------------------------------------------------------------------
# operand forms
# ---------------------------------------------------------------------------------------------------------------
class Form:
    """Widths, fused prologue, residual ("none", "sep" = a buffer of its own, "inplace" = `out` itself), epilogue
    activation, second output (raw sums in `out`, the activated copy in `out2`)."""

    def __init__(self, Cin, Cout, aff, res, act, out2=False):
        assert res in ("none", "sep", "inplace") and (act or not out2)
        self.Cin, self.Cout, self.aff, self.res, self.act, self.out2 = Cin, Cout, bool(aff), res, bool(act), bool(out2)

    def key(self):
        return (self.Cin, self.Cout, self.aff, self.res, self.act, self.out2)

    def __str__(self):
        return "%dx%d%s-%s%s%s" % (self.Cin, self.Cout, "-aff" if self.aff else "", self.res, "-act" if self.act else "",
                                   "-out2" if self.out2 else "")


# every table: the three residual forms under both ring depths (32 -> 32: D = 6; every other width: D = 8)
BASE_FORMS = [Form(32, 32, 0, "none", 0), Form(32, 32, 1, "sep", 1, out2=True), Form(32, 32, 0, "inplace", 1),
              Form(16, 16, 1, "inplace", 0), Form(32, 16, 0, "sep", 1, out2=True), Form(16, 32, 1, "none", 1)]
# the multi-group tables s4a and r8: every width (one to four passes, windows of 2 + 1 and 2 + 2 chunks), the rest of
# the prologue x residual x epilogue x second-output combinations
WIDE_FORMS = [Form(16, 16, 0, "sep", 1, out2=True), Form(16, 32, 0, "inplace", 0), Form(32, 16, 1, "inplace", 1),
              Form(32, 32, 1, "inplace", 0), Form(32, 32, 0, "sep", 0), Form(32, 32, 1, "none", 1, out2=True),
              Form(48, 16, 0, "inplace", 1), Form(48, 32, 1, "sep", 0), Form(48, 32, 0, "none", 1, out2=True),
              Form(64, 16, 1, "none", 0), Form(64, 32, 0, "sep", 1), Form(64, 32, 1, "inplace", 1, out2=True),
              Form(112, 16, 0, "sep", 0), Form(112, 32, 1, "inplace", 1), Form(112, 32, 0, "none", 0)]
WIDE_TABLES = ["s4a", "r8"]
CASES = [(t, f) for t in TABLES for f in BASE_FORMS] + [(t, f) for t in WIDE_TABLES for f in WIDE_FORMS]
# (no second output: without a step table the kernels that take over have none)
EDGE_FORMS = [Form(32, 32, 1, "inplace", 1), Form(16, 16, 0, "sep", 1), Form(48, 32, 0, "none", 0)]


def case_id(case):
    return "%s-%s" % (case[0], case[1])


# ---------------------------------------------------------------------------------------------------------------
# operands and the reference
# ---------------------------------------------------------------------------------------------------------------
def operands(tbl, form, leg):
    """x [M_in, Cin], W [K, Cin, Cout] (K = the table's offsets), in_scale / in_shift [Cin], residual [M_out, Cout],
    out_scale / out_shift [Cout] as float32 (all of them, whether the form uses them or not)."""
    rng = np.random.default_rng(seed_of("operands", tbl.name, form.key(), leg))
    Cin, Cout, K = form.Cin, form.Cout, tbl.K
    if leg == "int":
        x = rng.integers(-X_LIM, X_LIM + 1, (tbl.M_in, Cin))
        W = rng.integers(-W_LIM, W_LIM + 1, (K, Cin, Cout))
        sc, sh = rng.choice(SC_VALUES, Cin), rng.integers(-SH_LIM, SH_LIM + 1, Cin)
        res = rng.integers(-RES_LIM, RES_LIM + 1, (tbl.M_out, Cout))
        osc, osh = rng.choice(SC_VALUES, Cout), rng.integers(-SH_LIM, SH_LIM + 1, Cout)
    else:
        x = rng.standard_normal((tbl.M_in, Cin))
        W = rng.standard_normal((K, Cin, Cout)) / math.sqrt(9 * Cin)
        sc, sh = rng.uniform(0.5, 1.5, Cin), 0.3 * rng.standard_normal(Cin)
        res = rng.standard_normal((tbl.M_out, Cout))
        osc, osh = rng.uniform(0.5, 1.5, Cout), 0.3 * rng.standard_normal(Cout)
    return tuple(np.ascontiguousarray(a, np.float32) for a in (x, W, sc, sh, res, osc, osh))


def int_bound(form, K=K):
    """Largest magnitude any partial sum, sum (+ residual) or epilogue value of the integer leg can reach."""
    a = max(SC_VALUES) * X_LIM + SH_LIM if form.aff else X_LIM
    s = K * form.Cin * a * W_LIM + (RES_LIM if form.res != "none" else 0)
    return max(SC_VALUES) * s + SH_LIM if form.act else s


def forward_ref(x, W, nbr, M_out, in_scale=None, in_shift=None, residual=None, out_scale=None, out_shift=None):
    """float64: out[o] = sum_k act(x[nbr[k][o]]) W[k] (+ residual), act(v) = max(v * in_scale + in_shift, 0); an ABSENT
    row (-1) contributes zero -- the kernel's own rule: the shift is dropped with the row.  Returns (raw sums, the
    epilogue's max(raw * out_scale + out_shift, 0) or None)."""
    a = x.astype(np.float64)
    if in_scale is not None:
        a = np.maximum(a * in_scale.astype(np.float64) + in_shift.astype(np.float64), 0.0)
    raw = np.zeros((M_out, W.shape[2]))
    for k in range(W.shape[0]):
        col = nbr[k, :M_out]
        o = np.nonzero(col >= 0)[0]
        raw[o] += a[col[o]] @ W[k].astype(np.float64)
    if residual is not None:
        raw += residual.astype(np.float64)
    act = None
    if out_scale is not None:
        act = np.maximum(raw * out_scale.astype(np.float64) + out_shift.astype(np.float64), 0.0)
    return raw, act


def expected(tbl, form, ops):
    """(what `out` must hold, what `out2` must hold or None) for a form's call."""
    x, W, sc, sh, res, osc, osh = ops
    raw, act = forward_ref(x, W, tbl.nbr, tbl.M_out, sc if form.aff else None, sh if form.aff else None,
                           res if form.res != "none" else None, osc if form.act else None, osh if form.act else None)
    if form.out2:
        return raw, act
    return (act if form.act else raw), None
