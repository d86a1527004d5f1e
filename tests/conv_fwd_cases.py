"""What test_conv_fwd_cases_host.py and test_gpu_conv_fwd_regimes.py share: the cases of the five forward families of
csrc/spconv_conv.hip that the LDS-weight suite (tests/conv_lw_cases.py, whose tables, forms, operands and float64
reference are reused here) does not cover -- k_conv_g16p, k_conv_g16, k_conv_pair, k_conv_os, k_conv_flat -- with

  * the STEP TABLE of k_conv_g16 / k_conv_g16p restated in numpy (spconv_rules.hip k_subm3): per 16-row group the
    present offsets in ascending order, four steps per 16-byte entry, -1 from the group's count n to
    max(4 * GF_STEP_PHA, round-up-4(n)), and behind the blocks [count, boundary 0 .. boundary count].  Everything the
    device builder leaves unwritten is POISON: step entries past a group's written blocks are valid input rows, boundary
    words past `count` are large group numbers, so a kernel that consumed either would give a wrong integer result, not
    a silent zero;
  * chunk boundaries set by hand (the kernel reads the count from the table, so a case chooses its own chunking) and the
    rule of k_group_chunks restated (chunk_cost, the integer floor rule, the tail);
  * per family a classifier that returns, from a case alone (table, chunking, form, knobs), the regime labels it
    reaches; the host test proves that the case lists reach every label of REQUIRED and that the planner sends every
    case to the instance it is meant for.

A case is a table, a form (conv_lw_cases.Form), the dev knobs that force its family and what the planner must answer."""
import functools

import numpy as np

from tests import conv_lw_cases as L
from tests.conv_lw_cases import Form, Table, build_table, seed_of  # noqa: F401  (re-exported)

STEP_BLKS, STEP_PHA = 7, 3  # common.h GF_STEP_BLKS, GF_STEP_PHA
CHUNKS_DEFAULT, CHUNKS_MAX, CHUNK_GROUP_COST = 3072, 4096, 3  # GF_CONV_CHUNKS, GF_CONV_CHUNKS_MAX, CHUNK_GROUP_COST
BOUND_POISON = 1 << 24  # "group numbers" no table of these tests has
MAX_CIN = 512  # CONV_MAX_CIN: conv_fwd_impl rejects wider inputs (496 with a prologue)
NONE, LW, FLAT, G16P, G16, PAIR, OS = range(7)  # gf_dev_conv_plan's family numbers
FAMILY = ["none", "lw", "flat", "g16p", "g16", "pair", "os"]


def _ceil(a, b):
    return (a + b - 1) // b


# ---------------------------------------------------------------------------------------------------------------
# the step table and its chunk boundaries, restated
# ---------------------------------------------------------------------------------------------------------------
def steps_words(ld):
    """gf_rules_steps_words"""
    return (ld // 16) * STEP_BLKS * 64 + CHUNKS_MAX + 16


def poison_buffer(ld, M_in):
    """A step-table buffer before any builder touched it: valid input rows in the blocks, large group numbers behind."""
    nblk = (ld // 16) * STEP_BLKS * 64
    buf = np.empty(steps_words(ld), np.int32)
    buf[:nblk] = (np.arange(nblk, dtype=np.int64) * 7 + 3) % max(M_in, 1)
    buf[nblk:] = BOUND_POISON + np.arange(buf.size - nblk)
    return buf


def write_step_blocks(buf, nbr, M_out, ld):
    """What k_subm3 writes into the blocks of every group of ld / 16 (rows from M_out on count as absent)."""
    ng = ld // 16
    blocks = buf[: ng * STEP_BLKS * 64].reshape(ng, STEP_BLKS, 16, 4)
    K = nbr.shape[0]
    pad = np.full((K, ld), -1, np.int32)
    pad[:, :M_out] = nbr[:, :M_out]
    for g in range(ng):
        blk = pad[:, 16 * g:16 * g + 16]
        ks = [k for k in range(K) if (blk[k] >= 0).any()]
        for s, k in enumerate(ks):
            blocks[g, s // 4, :, s % 4] = blk[k]
        for s in range(len(ks), max(4 * STEP_PHA, _ceil(len(ks), 4) * 4)):
            blocks[g, s // 4, :, s % 4] = -1
    return buf


def written_blocks(n):
    """Blocks of a group of n present offsets the builder writes; the rest keeps what the buffer held."""
    return max(STEP_PHA, _ceil(n, 4))


def write_bounds(buf, ld, bounds):
    """[count, boundary 0 .. boundary count] at word (ld / 16) * GF_STEP_BLKS * 64."""
    at = (ld // 16) * STEP_BLKS * 64
    count = len(bounds) - 1
    assert 1 <= count <= CHUNKS_MAX and bounds[0] == 0 and (np.diff(bounds) >= 0).all()
    buf[at] = count
    buf[at + 1: at + 2 + count] = bounds
    return buf


def step_table(T, bounds):
    """The whole buffer of gf_rules_steps_words(ld) words for a table and a chunking, poison where nothing is written."""
    assert bounds[-1] == T.ngroups
    return write_bounds(write_step_blocks(poison_buffer(T.ld, T.M_in), T.nbr, T.M_out, T.ld), T.ld, bounds)


def chunk_cost(n):
    """Cost of a group of n present offsets in steps (spconv_rules.hip chunk_cost)."""
    return n + CHUNK_GROUP_COST + (8 if n > 4 * STEP_PHA else 0)


def group_chunks(sizes, nchunks):
    """k_group_chunks: chunk c starts at the first group whose preceding cost `before` reaches c * C / nchunks, i.e. group
    g writes the boundaries c with floor(prev * nchunks / C) < c <= floor(before * nchunks / C); the boundaries behind
    the last group's start, and boundary `nchunks`, are the group count.  Returns the nchunks + 1 boundaries."""
    cost = [chunk_cost(int(n)) for n in sizes]
    ng = len(cost)
    C = sum(cost) if sum(cost) > 0 else 1
    out = [None] * (nchunks + 1)
    before = 0
    for g in range(ng):
        c_hi = before * nchunks // C
        c_lo = (before - cost[g - 1]) * nchunks // C + 1 if g > 0 else 0
        for c in range(c_lo, min(c_hi, nchunks - 1) + 1):
            out[c] = g
        before += cost[g]
    last = (C - cost[ng - 1]) * nchunks // C + 1 if ng > 0 else 0
    for c in range(last, nchunks + 1):
        out[c] = ng
    assert None not in out
    return out


def chunking(name, sizes):
    """Boundaries of a named chunking of a table's groups."""
    ng = len(sizes)
    if name == "each":  # one group per chunk
        return list(range(ng + 1))
    if name == "few3":  # fewer chunks than any workgroup has waves
        return [0, ng // 3, ng // 3 * 2, ng]
    if name == "holes":  # empty chunks at the start, in the middle and at the end; chunks of 1, 2, 3 and 5 groups
        assert ng > 11
        return [0, 0, 1, 3, 3, 3, 6, 11, ng, ng, ng]
    if name == "big":  # one chunk of every group (more than 64: the per-lane masks run out) beside three empty ones
        assert ng >= 70
        return [0, 0, ng, ng, ng]
    if name.startswith("rule"):  # the device builder's equal-cost rule
        return group_chunks(sizes, int(name[4:]))
    raise KeyError(name)


# ---------------------------------------------------------------------------------------------------------------
# tables
# ---------------------------------------------------------------------------------------------------------------
def identity_table(name, M_out, M_in):
    """K = 1 without a table: output row o reads input row o."""
    ld = max(L._round16(M_out), 16)
    nbr = np.full((1, ld), -1, np.int32)
    nbr[0, :M_out] = np.arange(M_out)
    return Table(name, 0, M_in, M_out, nbr, [1] * _ceil(M_out, 16))


EVERY_SIZE = [n for n in range(28) for _ in range(3)] + [9]  # 85 groups: every size three times, a partial last one
PAIR27 = [tuple(range(27)), 0, 0, 5, tuple(range(0, 27, 2)), tuple(range(1, 27, 2)), (3, 7, 13, 20), (3, 7, 13, 20), 0, 0,
          (0, 13, 26), (1, 13), 11]
PAIR8 = [tuple(range(8)), 0, 0, 5, (0, 2, 4, 6), (1, 3, 5, 7), (2, 5), (2, 5), 0, 0, (0, 7), (3, 7), 4]


@functools.lru_cache(maxsize=None)
def table(name):
    rng = np.random.default_rng(seed_of("fwd-sizes", name))
    if name == "every":  # groups of every size 0 .. 27, shuffled, the last group partial
        return build_table(name, 0, EVERY_SIZE, M_out=85 * 16 - 7, M_in=900)
    if name == "one":
        return build_table(name, 0, [5], M_out=1, M_in=9)
    if name == "sixteen":
        return build_table(name, 0, [14], M_out=16, M_in=16)
    if name == "three":  # fewer groups than a workgroup of k_conv_g16 has waves
        return build_table(name, 0, [13, 27, 2], M_out=3 * 16 - 4, M_in=30)
    if name == "pair27":  # partner groups (27, 0), (0, 5), disjoint, identical, both empty, two overlapping ones; a lone last group
        return build_table(name, 0, PAIR27, M_out=13 * 16 - 9, M_in=150, shuffle=False)
    if name == "pair8":
        return build_table(name, 0, PAIR8, M_out=13 * 16 - 3, M_in=77, shuffle=False, K=8)
    if name == "os37":  # random sizes, ragged end, M_in != M_out
        return build_table(name, 0, rng.integers(0, 28, 37).tolist(), M_out=37 * 16 - 11, M_in=700)
    if name == "os37k8":
        return build_table(name, 0, rng.integers(0, 9, 37).tolist(), M_out=37 * 16 - 5, M_in=301, K=8)
    if name == "thin":  # 0 .. 3 present offsets per group: fewer steps than the 4 (16) waves that share an item
        return build_table(name, 0, [0, 1, 2, 3, 1, 0, 3, 2, 1], M_out=9 * 16 - 6, M_in=99)
    if name == "none9":  # no neighbour at all
        return build_table(name, 0, [0] * 9, M_out=9 * 16 - 2, M_in=20)
    if name == "os2048":  # 2048 groups: two column blocks per wave of the four-wave shape
        return build_table(name, 0, rng.integers(0, 28, 2048).tolist(), M_out=2048 * 16 - 3, M_in=5000)
    if name == "os2047":  # with 144 output channels 2047 * 9 = 18 423 items for a grid of 16 384
        return build_table(name, 0, rng.integers(0, 28, 2047).tolist(), M_out=2047 * 16 - 5, M_in=9000)
    if name == "f17":
        return build_table(name, 0, [27, 8], M_out=17, M_in=40)
    if name == "f17k8":
        return build_table(name, 0, [8, 3], M_out=17, M_in=9, K=8)
    if name == "f1":
        return build_table(name, 0, [6], M_out=1, M_in=5)
    if name == "f16":
        return build_table(name, 0, [19], M_out=16, M_in=33)
    if name == "id17":
        return identity_table(name, 17, 21)
    if name == "id40":
        return identity_table(name, 40, 40)
    raise KeyError(name)


# ---------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------
class Case:
    """family, table name, form, the dev knobs (test_conv_plan._set_knobs' names) and what the planner must answer:
    `want` = the family's template parameters (ConvPlan.p, leading ones).  chunks: the named chunking of a step-table
    case.  gmask / nbr: whether the call passes them; misaligned: the input is a view 4 bytes off."""

    def __init__(self, family, tname, form, knobs, want, chunks=None, gmask=True, nbr=True, misaligned=False):
        self.family, self.tname, self.form, self.knobs, self.want = family, tname, form, dict(knobs), list(want)
        self.chunks, self.gmask, self.nbr, self.misaligned = chunks, gmask, nbr, misaligned

    @property
    def table(self):
        return table(self.tname)

    @property
    def steps(self):
        return self.family in (G16P, G16)

    def bounds(self):
        return chunking(self.chunks, self.table.sizes) if self.chunks else None

    def id(self):
        kn = "-".join("%s%d" % (k, v) for k, v in sorted(self.knobs.items()) if k not in ("flat", "g16", "split", "pair"))
        return "-".join(x for x in (FAMILY[self.family], self.tname, str(self.form), self.chunks, kn,
                                    "" if self.gmask else "nomask", "" if self.nbr else "notable",
                                    "misaligned" if self.misaligned else "") if x)

    def query(self):
        """The call as test_conv_plan._call takes it."""
        T, f = self.table, self.form
        al = dict({k: True for k in ("in", "sc", "out", "res", "out2", "osc")}, **{"in": not self.misaligned})
        return dict(K=T.K, M_in=T.M_in, M_out=T.M_out, ld=T.ld, Cin=f.Cin, Cout=f.Cout, nbr=self.nbr, gmask=self.gmask,
                    steps=self.steps, flat=False, sc=f.aff, res=f.res != "none", out2=f.out2, osc=f.act, aligned=al)

    def plan(self):
        """The ten words gf_dev_conv_plan must answer: family, p[0..5], grid, block, dynamic LDS bytes."""
        T, f, w = self.table, self.form, self.want
        ng, nch, ncb = T.ngroups, _ceil(f.Cin, 16), _ceil(f.Cout, 16)
        aff, res = int(f.aff), int(f.res != "none")
        if self.family == G16P:
            nchw, ldsw, wpb = w
            return [G16P, nchw, ldsw, wpb, aff, res, 0, _ceil(CHUNKS_MAX, wpb), 64 * wpb, T.K * nch * 1024 * ldsw]
        if self.family == G16:
            nchw, ldsw, gpw = w
            return [G16, nchw, ldsw, gpw, aff, res, 0, _ceil(ng, 4 * gpw), 256, T.K * nch * 1024 * ldsw]
        if self.family == PAIR:
            return [PAIR, aff, 0, 0, 0, 0, 0, _ceil(_ceil(ng, 2), 4), 256, 0]
        if self.family == FLAT:
            return [FLAT, w[0], 0, 0, 0, 0, 0, ng * ncb, 1024, 0]
        ncbw, sw, vec = w
        nitems = ng * _ceil(ncb, ncbw)
        block = 64 * sw if sw else (self.knobs.get("block") or 256)
        grid = min(nitems if sw else _ceil(nitems, block // 64), 256 * 64)
        return [OS, ncbw, sw, vec, 0, 0, 0, grid, block, 0]


def case_id(c):
    return c.id()


RES = ["none", "sep", "inplace"]
G16P_KNOBS = dict(g16=1, g16_pipe=1, flat=0)
G16_KNOBS = dict(g16=1, g16_pipe=0, flat=0)
PAIR_KNOBS = dict(split=0, pair=1, g16=0, flat=0)
OS0_KNOBS = dict(split=0, pair=0, g16=0, flat=0)
OS4_KNOBS = dict(split=1, wide=0, g16=0, flat=0)
OS16_KNOBS = dict(split=1, wide=1, g16=0, flat=0)
FLAT_KNOBS = dict(flat=1)
G16P_CHUNKINGS = ["each", "few3", "holes", "big", "rule4096", "rule12", "rule3072"]  # (7: coprime to the 4 WPBs)


def _g16p_cases():
    out, i = [], 0
    for nch in (1, 2):
        for aff in (0, 1):
            for res in (0, 1):
                for ldsw in (0, 1):
                    for wpb in (4, 8, 12, 16):  # all 64 instances on the every-size table, chunkings in turn
                        act = i % 3 != 0
                        form = Form(16 * nch, 16, aff, RES[1 + (i // 4) % 2] if res else "none", act, out2=act and i % 5 < 3)
                        out.append(Case(G16P, "every", form, dict(G16P_KNOBS, g16_ldsw=ldsw, wpb=wpb), [nch, ldsw, wpb],
                                        chunks=G16P_CHUNKINGS[i % 7]))
                        i += 1
    for tname in ("one", "sixteen"):  # a single row, a single full group
        for nch, wpb, ldsw, form in [(1, 12, 1, Form(16, 16, 1, "sep", 1, out2=True)), (2, 4, 0, Form(32, 16, 1, "inplace", 0)),
                                     (2, 16, 1, Form(32, 16, 0, "none", 1))]:
            out.append(Case(G16P, tname, form, dict(G16P_KNOBS, g16_ldsw=ldsw, wpb=wpb), [nch, ldsw, wpb], chunks="each"))
    # the planner's own choice of the waves per workgroup: 12 at 16 channels, 4 at 32 (chunk knob at its default)
    out.append(Case(G16P, "every", Form(16, 16, 1, "sep", 1, out2=True), G16P_KNOBS, [1, 1, 12], chunks="rule3072"))
    out.append(Case(G16P, "every", Form(32, 16, 1, "sep", 1, out2=True), G16P_KNOBS, [2, 1, 4], chunks="rule3072"))
    return out


def _g16_cases():
    out, i = [], 0
    for nch in (1, 2):
        for aff in (0, 1):
            for res in (0, 1):
                for ldsw in (0, 1):
                    for gpw in (1, 2, 3):
                        form = Form(16 * nch, 16, aff, RES[1 + i % 2] if res else "none", i % 3 == 1)
                        out.append(Case(G16, "every", form, dict(G16_KNOBS, g16_ldsw=ldsw, g16_gpw=gpw), [nch, ldsw, gpw]))
                        i += 1
    for nch, ldsw, gpw, form in [(1, 1, 2, Form(16, 16, 1, "sep", 1)), (2, 0, 1, Form(32, 16, 1, "inplace", 0)),
                                 (2, 1, 3, Form(32, 16, 0, "none", 1))]:
        for tname in ("three", "one"):
            out.append(Case(G16, tname, form, dict(G16_KNOBS, g16_ldsw=ldsw, g16_gpw=gpw), [nch, ldsw, gpw]))
    return out


def _pair_cases():
    forms27 = [Form(16, 16, 1, "sep", 1), Form(16, 16, 0, "none", 0), Form(32, 16, 1, "inplace", 0), Form(48, 5, 1, "sep", 1),
               Form(128, 16, 0, "sep", 1), Form(128, 5, 1, "none", 0), Form(32, 5, 0, "inplace", 1), Form(48, 16, 0, "none", 1)]
    forms8 = [Form(16, 16, 1, "sep", 1), Form(32, 5, 1, "inplace", 0), Form(128, 16, 0, "none", 1), Form(48, 16, 1, "none", 0)]
    return ([Case(PAIR, "pair27", f, PAIR_KNOBS, []) for f in forms27] + [Case(PAIR, "pair8", f, PAIR_KNOBS, []) for f in forms8]
            + [Case(PAIR, "one", Form(16, 16, 1, "sep", 1), PAIR_KNOBS, [])])


def _os_cases():
    out = []
    # one wave per item: 1 .. 8 column blocks per wave, 160 channels = two items per group, partial last blocks
    for i, Cout in enumerate([16, 32, 48, 64, 80, 96, 112, 128, 160, 21, 40]):
        ncbw = min(_ceil(Cout, 16), 8)
        block = [256, 64, 128][i % 3]
        form = Form([16, 32, 48][i % 3], Cout, i % 2, RES[i % 3], i % 4 < 2)
        out.append(Case(OS, "os37", form, dict(OS0_KNOBS, block=block), [ncbw, 0, 1]))
    for Cin, Cout, mis, form_kw in [(6, 32, False, (1, "sep", 1)), (19, 21, False, (1, "inplace", 0)), (32, 48, True, (1, "sep", 1)),
                                    (19, 112, False, (0, "none", 1))]:  # the scalar gathers: odd widths, a misaligned input
        out.append(Case(OS, "os37", Form(Cin, Cout, *form_kw), OS0_KNOBS, [min(_ceil(Cout, 16), 8), 0, 0], misaligned=mis))
    out.append(Case(OS, "os37", Form(32, 64, 1, "sep", 1), OS0_KNOBS, [4, 0, 1], gmask=False))
    out.append(Case(OS, "os37k8", Form(32, 48, 1, "inplace", 1), OS0_KNOBS, [3, 0, 1]))
    out.append(Case(OS, "id40", Form(32, 32, 1, "sep", 0), OS0_KNOBS, [2, 0, 1], gmask=False, nbr=False))
    # four waves per item
    for tname, form in [("os37", Form(32, 40, 1, "sep", 1)), ("os37", Form(19, 16, 0, "inplace", 0)),
                        ("thin", Form(16, 32, 1, "sep", 1)), ("none9", Form(16, 16, 1, "inplace", 1)),
                        ("os37k8", Form(16, 21, 0, "none", 1))]:
        out.append(Case(OS, tname, form, OS4_KNOBS, [1, 4, int(form.Cin % 16 == 0)]))
    out.append(Case(OS, "os37", Form(16, 32, 0, "sep", 0), OS4_KNOBS, [1, 4, 1], gmask=False))
    out.append(Case(OS, "os2048", Form(16, 40, 1, "sep", 1), OS4_KNOBS, [2, 4, 1]))
    out.append(Case(OS, "os2048", Form(16, 16, 0, "none", 0), OS4_KNOBS, [1, 4, 1]))
    out.append(Case(OS, "os2047", Form(16, 144, 1, "sep", 0), OS4_KNOBS, [1, 4, 1]))  # a second item per workgroup
    # sixteen waves per item
    for tname, form in [("os37", Form(16, 16, 1, "sep", 1)), ("thin", Form(32, 21, 1, "inplace", 0)),
                        ("none9", Form(48, 32, 1, "sep", 1)), ("f17", Form(448, 224, 1, "sep", 1)),
                        ("os37", Form(6, 16, 0, "none", 0)), ("os37k8", Form(64, 32, 0, "inplace", 1)),
                        ("id17", Form(48, 16, 1, "none", 1))]:
        out.append(Case(OS, tname, form, OS16_KNOBS, [1, 16, int(form.Cin % 16 == 0)], gmask=tname != "id17",
                        nbr=tname != "id17"))
    return out


FLAT_STEPS = {1: (1, 16), 15: (1, 240), 8: (8, 16), 16: (8, 32), 27: (27, 16), 64: (8, 128), 128: (8, 256), 81: (27, 48),
              135: (27, 80), 243: (27, 144), 270: (27, 160), 378: (27, 224)}  # steps per item -> (K, Cin)
FLAT_TABLES = {1: ["id17", "id40"], 8: ["f17k8"], 27: ["f17", "f1", "f16"]}
FLAT_LEAVES = (27, 240)  # 405 steps: beyond the flat kernel's six batches


def _flat_cases():
    out, i = [], 0
    for steps, (K, Cin) in sorted(FLAT_STEPS.items()):
        for tname in FLAT_TABLES[K][: 1 if steps not in (1, 27, 270) else 3]:
            form = Form(Cin, [16, 40, 112][i % 3], (i >> 0) & 1, RES[(i >> 1) % 3], (i >> 2) & 1)
            out.append(Case(FLAT, tname, form, FLAT_KNOBS, [4 if steps <= 256 else 6], nbr=K != 1, gmask=K != 1))
            i += 1
    for aff in (0, 1):  # every prologue x residual x activation form
        for res in RES:
            for act in (0, 1):
                out.append(Case(FLAT, "f17", Form(16, 40, aff, res, act), FLAT_KNOBS, [4]))
    return out


def _flat_edge_cases():
    """405 steps per item: the planner leaves the flat kernel (for the sixteen-wave shape of k_conv_os)."""
    return [Case(OS, "f17", Form(FLAT_LEAVES[1], Cout, aff, res, act), FLAT_KNOBS, [1, 16, 1])
            for Cout, aff, res, act in [(16, 1, "sep", 1), (40, 0, "inplace", 0)]]


CASES = {"g16p": _g16p_cases(), "g16": _g16_cases(), "pair": _pair_cases(), "os": _os_cases(),
         "flat": _flat_cases() + _flat_edge_cases()}
ALL_CASES = [c for fam in CASES.values() for c in fam]


# ---------------------------------------------------------------------------------------------------------------
# regimes
# ---------------------------------------------------------------------------------------------------------------
def _form_labels(f):
    return {"res:" + f.res, "aff:%d" % f.aff, "act:%d" % f.act}


def size_labels(nch, sizes):
    """What a group of n present offsets makes k_conv_g16p do: below 8 steps the multiplications of absent steps run (on
    zeros), from 8 on they are skipped; NS = 12 (8 at two input chunks) steps are pipelined, the rest runs in trips
    of two blocks, the last of which is the odd fifth block at two chunks."""
    NS = 4 * (STEP_PHA if nch == 1 else 2)
    out = set()
    for n in set(int(s) for s in sizes):
        out.add("n%d:%d" % (nch, n))
        if n > NS:
            trips = _ceil(n - NS, 8)
            out.add("tail%d:%d%s" % (nch, trips, "-odd-block" if (trips * 2 > STEP_BLKS - NS // 4) else ""))
    return out


def chunk_labels(bounds, wpb, ldsw):
    count, lens = len(bounds) - 1, np.diff(bounds)
    busy = np.nonzero(lens)[0]
    out = set()
    if (lens == 1).all() and count > wpb and count % wpb:
        out.add("one-group-per-chunk")
    if count % wpb and ldsw:
        out.add("waves-past-count-before-barrier")
    if count < wpb and ldsw and wpb in (12, 16):
        out.add("count<wpb:%d" % wpb)
    if busy.size:
        if lens[0] == 0:
            out.add("empty-first")
        if lens[-1] == 0:
            out.add("empty-last")
        if (lens[busy[0]: busy[-1]] == 0).any():
            out.add("empty-middle")
    out |= {"len:%d" % n for n in (1, 2, 3, 5) if (lens == n).any()}
    if (lens >= 70).any() and (lens == 0).sum() >= 3:
        out.add("mask-fallback")
    if count == CHUNKS_MAX:
        out.add("count:4096")
    return out


def labels(c):
    """The regime labels a case reaches (all of them in REQUIRED[family])."""
    T, f = c.table, c.form
    nch, ncb = _ceil(f.Cin, 16), _ceil(f.Cout, 16)
    out = set()
    if c.family == G16P:
        nchw, ldsw, wpb = c.want
        out |= {"inst:%d%d%d%d:%d" % (nchw, f.aff, f.res != "none", ldsw, wpb), "res:" + f.res, "act:%d" % f.act}
        out |= size_labels(nch, T.sizes) | chunk_labels(c.bounds(), wpb, ldsw)
        if f.out2:
            out.add("out2:" + ("res" if f.res != "none" else "nores"))
        if T.M_out in (1, 16):
            out.add("M_out:%d" % T.M_out)
        if T.M_out % 16 and T.ngroups > 1:
            out.add("partial-last-group")
    elif c.family == G16:
        nchw, ldsw, gpw = c.want
        out |= {"inst:%d%d%d%d" % (nchw, f.aff, f.res != "none", ldsw), "gpw:%d:ldsw%d" % (gpw, ldsw), "res:" + f.res,
                "act:%d" % f.act}
        out |= {s for s in size_labels(nch, T.sizes) if s.startswith("n")}
        if T.ngroups % (4 * gpw) and T.ngroups > 4 * gpw:
            out.add("groups-not-multiple")
        if T.ngroups < 4:
            out.add("groups<4")
    elif c.family == PAIR:
        out |= _form_labels(f) | {"K:%d" % T.K, "Cin:%d" % f.Cin, "Cout:%d" % f.Cout}
        s = [set(np.nonzero([(int(m) >> k) & 1 for k in range(T.K)])[0].tolist()) for m in T.gmask[: T.ngroups]]
        for a, b in zip(s[0::2], s[1::2]):
            if len(a) == T.K and not b:
                out.add("pair:full+empty")
            elif not a and len(b) == 5:
                out.add("pair:empty+5")
            elif a and b and not (a & b):
                out.add("pair:disjoint")
            elif a and a == b:
                out.add("pair:identical")
            elif not a and not b:
                out.add("pair:union-empty")
            elif a and b:
                out.add("pair:overlapping")
        if T.ngroups % 2:
            out.add("lone-last-group")
        if T.M_out % 16:
            out.add("ragged")
        if T.M_in != T.M_out:
            out.add("M_in!=M_out")
        if _ceil(_ceil(T.ngroups, 2), 4) > 1:
            out.add("blocks>1")
    elif c.family == OS:
        ncbw, sw, vec = c.want
        out |= {"inst:%d:%d:%d" % (ncbw, sw, vec), "sw%d:res:%s" % (sw, f.res), "sw%d:aff:%d" % (sw, f.aff),
                "sw%d:act:%d" % (sw, f.act), "K:%d" % T.K}
        nsteps = set((T.sizes * nch).tolist())
        if sw == 0:
            out.add("block:%d" % (c.knobs.get("block") or 256))
            if _ceil(ncb, ncbw) > 1:
                out.add("nsplit:2")
            if f.Cout % 16:
                out.add("Cout:%d" % f.Cout)
            if not vec:
                out.add("scalar:" + ("misaligned" if c.misaligned else "Cin%d" % f.Cin))
            if ncbw > 2 and f.res != "none" and f.act:
                out.add("late-residual-and-activation")
        if sw == 4:
            if any(0 < n < 4 for n in nsteps):
                out.add("sw4:steps<waves")
            if c.plan()[7] < T.ngroups * _ceil(ncb, ncbw):
                out.add("second-item" + ("-aff-res" if f.aff and f.res != "none" else ""))
        if sw == 16:
            if any(0 < n < 16 for n in nsteps):
                out.add("sw16:steps<16")
            if nsteps == {0}:
                out.add("sw16:no-steps")
            if (f.Cin, f.Cout) == (448, 224):
                out.add("sw16:448x224")
        if not c.gmask and c.nbr:
            out.add("gmask-null:sw%d" % sw)
        if not c.nbr:
            out.add("no-table")
        if T.M_in != T.M_out and T.K == 8:
            out.add("K8:M_in!=M_out")
        if (T.K, f.Cin) == FLAT_LEAVES:
            out.add("left-flat:405")
    elif c.family == FLAT:
        out |= {"steps:%d" % (T.K * nch), "maxb:%d" % c.want[0], "Cout:%d" % f.Cout, "M_out:%d" % T.M_out,
                "form:%d:%s:%d" % (f.aff, f.res, f.act)}
    return out


def _required():
    g16p = {"inst:%d%d%d%d:%d" % (n, a, r, l, w) for n in (1, 2) for a in (0, 1) for r in (0, 1) for l in (0, 1)
            for w in (4, 8, 12, 16)}
    g16p |= {"res:" + r for r in RES} | {"act:0", "act:1", "out2:res", "out2:nores", "M_out:1", "M_out:16", "partial-last-group"}
    g16p |= {"n%d:%d" % (n, s) for n in (1, 2) for s in range(28)}
    g16p |= {"tail1:1", "tail1:2", "tail2:1", "tail2:2", "tail2:3-odd-block"}
    g16p |= {"one-group-per-chunk", "waves-past-count-before-barrier", "count<wpb:12", "count<wpb:16", "empty-first",
             "empty-middle", "empty-last", "len:1", "len:2", "len:3", "len:5", "mask-fallback", "count:4096"}
    g16 = {"inst:%d%d%d%d" % (n, a, r, l) for n in (1, 2) for a in (0, 1) for r in (0, 1) for l in (0, 1)}
    g16 |= {"gpw:%d:ldsw%d" % (g, l) for g in (1, 2, 3) for l in (0, 1)} | {"res:" + r for r in RES} | {"act:0", "act:1"}
    g16 |= {"n%d:%d" % (n, s) for n in (1, 2) for s in range(28)} | {"groups-not-multiple", "groups<4"}
    pair = {"res:" + r for r in RES} | {"aff:0", "aff:1", "act:0", "act:1", "K:27", "K:8", "Cin:16", "Cin:32", "Cin:48", "Cin:128",
                                       "Cout:16", "Cout:5", "pair:full+empty", "pair:empty+5", "pair:disjoint", "pair:identical",
                                       "pair:union-empty", "pair:overlapping", "lone-last-group", "ragged", "M_in!=M_out",
                                       "blocks>1"}
    os_ = {"inst:%d:0:1" % n for n in range(1, 9)} | {"inst:%d:0:0" % n for n in (2, 3, 7)}
    os_ |= {"inst:1:4:1", "inst:1:4:0", "inst:2:4:1", "inst:1:16:1", "inst:1:16:0"}
    os_ |= {"sw%d:res:%s" % (s, r) for s in (0, 4, 16) for r in RES} | {"sw%d:%s:%d" % (s, w, v) for s in (0, 4, 16)
                                                                       for w in ("aff", "act") for v in (0, 1)}
    os_ |= {"K:27", "K:8", "K:1", "block:64", "block:128", "block:256", "nsplit:2", "Cout:21", "Cout:40", "scalar:Cin6",
            "scalar:Cin19", "scalar:misaligned", "late-residual-and-activation", "sw4:steps<waves", "second-item-aff-res",
            "sw16:steps<16", "sw16:no-steps", "sw16:448x224", "gmask-null:sw0", "gmask-null:sw4", "no-table",
            "K8:M_in!=M_out", "left-flat:405"}
    flat = {"steps:%d" % s for s in FLAT_STEPS} | {"maxb:4", "maxb:6", "Cout:16", "Cout:40", "Cout:112", "M_out:1",
                                                   "M_out:16", "M_out:17", "M_out:40"}
    flat |= {"form:%d:%s:%d" % (a, r, t) for a in (0, 1) for r in RES for t in (0, 1)}
    return {"g16p": g16p, "g16": g16, "pair": pair, "os": os_, "flat": flat}


REQUIRED = _required()


def reciprocal_exact(K, nch):
    """(s * ceil(65536 / NCH)) >> 16 == s // NCH for every step s < K * NCH (k_conv_os, conv_flat_item)."""
    s = np.arange(K * nch, dtype=np.int64)
    return bool((((s * _ceil(65536, nch)) >> 16) == s // nch).all())


# ---------------------------------------------------------------------------------------------------------------
# voxel sets for device-built tables
# ---------------------------------------------------------------------------------------------------------------
VOXEL_SHAPE = (48, 40, 36)


def voxel_set(name):
    """int32 [M, 4] (batch 0), unique: a dense block, a plane, a line and isolated voxels ("mid": shuffled rows)."""
    rng = np.random.default_rng(seed_of("voxels", name))
    if name == "five":
        v = np.array([[1, 1, 1], [1, 1, 2], [2, 2, 2], [9, 9, 9], [30, 20, 10]])
    else:
        n = 26 if name == "big" else 7  # big: 17 576 voxels in the block alone, more than one group per thread
        blk = np.stack(np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij"), -1).reshape(-1, 3) + 1
        pl = np.stack(np.meshgrid(np.arange(30, 31), np.arange(2, 30), np.arange(3, 33), indexing="ij"), -1).reshape(-1, 3)
        ln = np.stack([np.full(25, 40), np.arange(5, 30), np.full(25, 7)], -1)
        iso = np.stack(np.meshgrid(np.arange(34, 47, 3), np.arange(32, 40, 3), np.arange(1, 36, 3), indexing="ij"), -1).reshape(-1, 3)
        v = np.concatenate([blk, pl, ln, iso])
    v = np.unique(v, axis=0)  # (sorted: the isolated voxels, the line and the plane give groups of 1, 3 and 9 offsets)
    if name != "big":
        v = v[rng.permutation(v.shape[0])]
    assert (v >= 0).all() and (v < np.array(VOXEL_SHAPE)).all()
    return np.ascontiguousarray(np.concatenate([np.zeros((v.shape[0], 1), np.int64), v], 1).astype(np.int32))
