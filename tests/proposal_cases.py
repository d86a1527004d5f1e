"""Float64 statements and the cases of the proposal stage: generate_proposal's fused statistics, select and membership
scatter (csrc/proposal.hip, csrc/proposal_rows.h), the bit-packed mask intersections and matrix NMS (csrc/batch_post.hip).
Shared by tests/test_proposal_cases_host.py (holds the cases and statements to account, no GPU), tests/golden/
make_matrix_nms_golden.py (the reference's picks on the matrix NMS cases) and tests/test_gpu_proposal_regimes.py.

Plain numpy with float64 inside; nothing here comes from geoformer_amd's kernels.

STATEMENTS
  stats_statement / stats_fs_statement   model/geoformer/geoformer.py:193-262 / geoformer_fs.py:205-238
  select_statement, scatter_statement, intersections_statement
  decayed_scores / picks_statement       util/utils_3d.py:95-141.  Every mask of every case is NON-EMPTY:
      generate_proposal never emits an empty mask (npoints >= npoint_thresh >= 1), and the reference's 0/0 IoU of two
      empty masks is outside this statement (decayed_scores asserts it).

MARGINS are conditions on the INPUTS, asserted when a case is built (a case that misses one is re-drawn or nudged, the
condition is never relaxed):
  LOGIT_MARGIN  no logit has |sigmoid64(x) - logit_thresh| < 1e-6 (at least 16 fp32 ulp of a sigmoid near 0.5), so the
                member counts, the membership rows and `sel` are exact integers whatever the rounding of expf;
  SCORE_MARGIN  every query whose other two acceptance conditions hold has |mask_score - score_thresh| > 1e-4 relative
                (few-shot: the same for sim against sim_thresh), so `final` is exact.

SWEEP THRESHOLDS of a matrix NMS case and kernel (what makes the picks a strong check): sort the finite float64 decayed
scores; a gap between neighbours lo < hi is USABLE when (hi - lo) / hi > GAP_REL = 1e-4 -- about 100 times what an fp32
evaluation of the expression can move a score (roughly ten roundings, ~1e-6); a condition on inputs, not a tolerance.
The thresholds are midpoints of usable gaps: every usable gap for n <= 65, 16 evenly spaced over the usable ones for larger
n, plus the standard 0.05 and 0.5 where no decayed score lies within GAP_REL / 2 relative of them (the distance the midpoint
of a just-usable gap keeps).  At most GAP_CAP = 5 % of a random case's gaps may be unusable.

HAND-BUILT MATRIX NMS CASES (sigma = 2; decayed scores by original index, gaussian | linear):
  one      n = 1, score 0.7:                      [0.7] | [0.7]
  pair     [0:1], [0:2]: IoU exactly 0.5, scores 0.9, 0.8, one class:
                                                   [0.9, 0.8 e^-0.5 = 0.485225] | [0.9, 0.4]
  chain3   A = [0:30], B = [10:40], C = [18:40] of one class, scores 0.9 / 0.8 / 0.7: iou(A,B) = 0.5, iou(B,C) = 22/30,
           iou(A,C) = 0.3.  C's coefficient is row B's compensated ratio f(22/30) / f(0.5), below row A's f(0.3):
                                                   [0.9, 0.485225, 0.7 e^(-2 (484/900 - 1/4)) = 0.393674] |
                                                   [0.9, 0.4, 0.7 (8/30) / 0.5 = 0.373333]
           (without the division C would be 0.238776 | 0.186667)
  chain3x  chain3 with B in another class: B is untouched, C decays by f(0.3) alone:
                                                   [0.9, 0.8, 0.7 e^-0.18 = 0.584689] | [0.9, 0.8, 0.49]
  dup3     three identical masks [0:20] of one class, scores 0.9 / 0.8 / 0.7, and a disjoint mask [30:50], score 0.6:
                                                   [0.9, 0.8 e^-2 = 0.108268, 0.7 e^-2 = 0.094735, 0.6] |
                                                   [0.9, 0, NaN, 0.6]
           linear: the third copy meets (1 - 1) / (1 - 1) = 0/0 in row B, the disjoint mask meets 1/0 = inf in rows B and
           C (its minimum is row A's 1); gaussian: everything stays finite.  A NaN decayed score is never kept.
  ties     five disjoint masks, scores [0.7, 0.9, 0.7, 0.7, 0.7]: nothing decays, rank order [1, 0, 2, 3, 4].
"""
import functools
from typing import NamedTuple

import numpy as np

LOGIT_MARGIN = 1e-6
SCORE_MARGIN = 1e-4
GAP_REL = 1e-4
GAP_CAP = 0.05
SIGMA = 2.0
KERNELS = ("gaussian", "linear")
STD_THRESHOLDS = (0.05, 0.5)

STATS_N = (1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8193)  # wave, workgroup, one trip (4 x 1024), third trip
STATS_NQ = 8
LOGIT_THRESH = 0.5
SCORE_THRESH = 0.7  # above logit_thresh: a mean of members' probabilities can fall on either side of it
SIM_THRESH = 0.6


# ---- statements -------------------------------------------------------------------------------------------------------
def sigmoid64(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def _mask_stats(logits, logit_thresh):
    p = sigmoid64(logits)
    member = p >= logit_thresh
    n = member.sum(1)
    mask_score = (p * member).sum(1) / (n + 1e-6)
    return member, n, mask_score


def stats_statement(logits, cls_logits, sem_prob, logit_thresh, score_thresh, npoint_thresh, min_class):
    """generate_proposal's statistics (geoformer.py:193-262) of logits [nq, N], cls_logits [nq, ncls] and sem_prob
    [N, ncls] (probabilities): dict of cls_pred (the FIRST maximum of the class logits), npoints, mask_score, sem_score,
    score = mask_score * sqrt(softmax[cls]) * sem_score (float64) and final (0/1)."""
    c = np.asarray(cls_logits, np.float64)
    cls = np.argmax(c, 1)  # first occurrence
    e = np.exp(c - c.max(1, keepdims=True))
    cls_score = (e / e.sum(1, keepdims=True))[np.arange(c.shape[0]), cls]
    member, n, mask_score = _mask_stats(logits, logit_thresh)
    sem = np.asarray(sem_prob, np.float64)[:, cls].T  # [nq, N]
    sem_score = (sem * member).sum(1) / (n + 1e-6)
    final = (cls >= min_class) & (n >= npoint_thresh) & (mask_score >= score_thresh)
    return {"cls_pred": cls.astype(np.int64), "npoints": n.astype(np.int64), "mask_score": mask_score,
            "sem_score": sem_score, "score": mask_score * np.sqrt(cls_score) * sem_score,
            "final": final.astype(np.int64)}


def stats_fs_statement(logits, sim, logit_thresh, score_thresh, npoint_thresh, sim_thresh):
    """The few-shot form (geoformer_fs.py:205-238): score = mask_score * sim ** 0.5, NaN for a negative similarity;
    final = sim >= sim_thresh and n >= npoint_thresh and mask_score >= score_thresh (0 for a negative similarity)."""
    s = np.asarray(sim, np.float64)
    _, n, mask_score = _mask_stats(logits, logit_thresh)
    with np.errstate(invalid="ignore"):
        score = mask_score * np.sqrt(s)
    final = (s >= sim_thresh) & (n >= npoint_thresh) & (mask_score >= score_thresh)
    return {"npoints": n.astype(np.int64), "mask_score": mask_score, "score": score, "final": final.astype(np.int64)}


def select_statement(final):
    """The accepted queries in ascending order."""
    return np.nonzero(np.asarray(final) != 0)[0].astype(np.int64)


def scatter_statement(logits, sel, fg_idxs, logit_thresh, num_points):
    """0/1 int32 rows [len(sel), num_points]: row i has a 1 at fg_idxs[p] for every member p of query sel[i]."""
    member = sigmoid64(np.asarray(logits)[np.asarray(sel, np.int64)]) >= logit_thresh
    out = np.zeros((len(sel), int(num_points)), np.int32)
    fg = np.asarray(fg_idxs, np.int64)
    for i in range(len(sel)):
        out[i, fg[member[i]]] = 1
    return out


def intersections_statement(masks):
    """The int64 m @ m.T (the product runs in float64, exact on 0/1 entries: every count is far below 2^53)."""
    m = (np.asarray(masks) != 0).astype(np.float64)
    return np.rint(m @ m.T).astype(np.int64)


def rank_order(scores):
    """Original indices by descending score, equal scores by ascending index."""
    return np.argsort(-np.asarray(scores, np.float64), kind="stable")


def decayed_scores(masks, scores, cats, kernel, sigma=SIGMA, mutant=None, inter=None):
    """Float64 restatement of util/utils_3d.py:95-141: the decayed score of every proposal, by ORIGINAL index.  Rank is
    descending score, equal scores by ascending index; inf / NaN propagate as numpy's min / max propagate them (a NaN in a
    column makes the column's coefficient NaN).  Every mask must be non-empty.
    mutant: None, or one of MUTANTS -- deliberately wrong statements that the sweep thresholds must tell apart.
    inter: intersections_statement(masks) where the caller already has it."""
    scores = np.asarray(scores, np.float64)
    n = scores.shape[0]
    order = rank_order(scores)
    inter = intersections_statement(masks) if inter is None else inter
    inter = inter[order][:, order].astype(np.float64)
    d = np.diag(inter)
    assert (d > 0).all(), "empty mask: outside the statement"
    iou = inter / (d[:, None] + d[None, :] - inter)
    c = np.asarray(cats)[order]
    same = np.ones((n, n)) if mutant == "class_agnostic" else (c[:, None] == c[None, :]).astype(np.float64)
    x = iou * np.triu(same, 1)  # x[r, a]: row r ranks above column a, same class
    comp = x.max(0) if n else np.zeros(0)
    comp_of = comp[None, :] if mutant == "comp_from_column" else comp[:, None]  # (the right one: row r's own)
    with np.errstate(divide="ignore", invalid="ignore"):
        if kernel == "gaussian":
            num, den = np.exp(-sigma * x ** 2), np.exp(-sigma * comp_of ** 2)
        elif kernel == "linear":
            num, den = 1.0 - x, 1.0 - comp_of
        else:
            raise NotImplementedError(kernel)
        coef = (num if mutant == "no_compensation" else num / den).min(0) if n else np.zeros(0)
        out = np.empty(n)
        out[order] = scores[order] * coef
    return out


MUTANTS = ("no_compensation", "class_agnostic", "comp_from_column")


def picks_from_decayed(decayed, scores, thresh):
    with np.errstate(invalid="ignore"):
        return [int(i) for i in rank_order(scores) if decayed[i] >= thresh]  # NaN >= t is False


def picks_statement(masks, scores, cats, kernel, thresh, sigma=SIGMA, mutant=None):
    """The kept proposals' original indices in rank order."""
    return picks_from_decayed(decayed_scores(masks, scores, cats, kernel, sigma, mutant), scores, thresh)


# ---- sweep thresholds -------------------------------------------------------------------------------------------------
def gaps(decayed):
    """(lo, hi, usable) of every gap between neighbouring finite decayed scores, ascending."""
    v = np.sort(decayed[np.isfinite(decayed)])
    lo, hi = v[:-1], v[1:]
    with np.errstate(divide="ignore", invalid="ignore"):
        usable = np.where(hi > 0, (hi - lo) / np.where(hi > 0, hi, 1.0) > GAP_REL, False)
    return lo, hi, usable


def std_usable(decayed, t):
    """A standard threshold is usable when no decayed score lies within GAP_REL / 2 relative of it."""
    v = decayed[np.isfinite(decayed)]
    return bool((np.abs(v - t) > 0.5 * GAP_REL * np.maximum(v, t)).all())


def sweep_midpoints(decayed, n):
    """The midpoints of the usable gaps that the sweep takes: all for n <= 65, 16 evenly spaced ones for larger n."""
    lo, hi, usable = gaps(decayed)
    mids = (0.5 * (lo + hi))[usable]
    if n > 65 and len(mids) > 16:
        mids = mids[np.round(np.linspace(0, len(mids) - 1, 16)).astype(np.int64)]
    return [float(t) for t in mids]


def sweep_thresholds(decayed, n):
    """(sorted thresholds, share of unusable gaps)."""
    usable = gaps(decayed)[2]
    thr = set(sweep_midpoints(decayed, n)) | {t for t in STD_THRESHOLDS if std_usable(decayed, t)}
    return tuple(sorted(thr)), (float((~usable).mean()) if len(usable) else 0.0)


# ---- statistics cases -------------------------------------------------------------------------------------------------
class StatsCase(NamedTuple):
    name: str
    logits: np.ndarray  # fp32 [nq, N]
    cls_logits: np.ndarray  # fp32 [nq, ncls]
    sem_prob: np.ndarray  # fp32 [N, ncls]
    sim: np.ndarray  # fp32 [nq] (the few-shot form)
    logit_thresh: float
    score_thresh: float
    npoint_thresh: int
    min_class: int
    sim_thresh: float

    def statement(self):
        return stats_statement(self.logits, self.cls_logits, self.sem_prob, self.logit_thresh, self.score_thresh,
                               self.npoint_thresh, self.min_class)

    def statement_fs(self):
        return stats_fs_statement(self.logits, self.sim, self.logit_thresh, self.score_thresh, self.npoint_thresh,
                                  self.sim_thresh)


def _logit(p):
    return float(np.log(p / (1.0 - p)))


def logit_margin_ok(logits, logit_thresh):
    return bool((np.abs(sigmoid64(logits) - logit_thresh) >= LOGIT_MARGIN).all())


def check_stats_margins(c):
    """Raises AssertionError unless the case meets LOGIT_MARGIN and SCORE_MARGIN (both forms)."""
    assert logit_margin_ok(c.logits, c.logit_thresh), (c.name, "a logit within LOGIT_MARGIN of logit_thresh")
    s = c.statement()
    others = (s["cls_pred"] >= c.min_class) & (s["npoints"] >= c.npoint_thresh)
    far = np.abs(s["mask_score"] - c.score_thresh) > SCORE_MARGIN * c.score_thresh
    assert far[others].all(), (c.name, "mask_score within SCORE_MARGIN of score_thresh")
    f = c.statement_fs()
    sim = c.sim.astype(np.float64)
    others = (f["npoints"] >= c.npoint_thresh) & (f["mask_score"] >= c.score_thresh)
    assert (np.abs(sim - c.sim_thresh) > SCORE_MARGIN * c.sim_thresh)[others].all(), (c.name, "sim within SCORE_MARGIN")
    others = (sim >= c.sim_thresh) & (f["npoints"] >= c.npoint_thresh)
    assert far[others].all(), (c.name, "few-shot mask_score within SCORE_MARGIN of score_thresh")


def _draw_stats(name, rng, N, ncls, min_class, npoint_thresh):
    """The planted rows (nq = 8):
      0  all members (constant logit 8)               4  predicted class min_class - 1 (where such a class exists;
      1  no member (constant logit -8)                   with ncls <= min_class every class is below it)
      2  exactly min(npoint_thresh, N) members        5  two equal maximal class logits k1 < k2, with
      3  one fewer                                        k1 < min_class <= k2 where ncls allows: the lower index wins
      6 / 7  constant logits whose mask_score is score_thresh * (1 +- 4 SCORE_MARGIN)
    Rows 2-5 have random logits.  Rows other than 4 and 5 predict a class >= min_class where ncls has one, so that the
    count and the score decide `final`."""
    nq = STATS_NQ
    x = (rng.normal(0, 3, (nq, N)) + rng.normal(0, 2, (nq, 1))).astype(np.float32)
    x[0], x[1] = 8.0, -8.0
    for row, k in ((2, min(npoint_thresh, N)), (3, min(npoint_thresh - 1, N))):
        mag = np.abs(x[row]) + 1.0  # every member's probability is above score_thresh: the count decides
        on = np.zeros(N, bool)
        on[rng.choice(N, k, replace=False)] = True
        x[row] = np.where(on, mag, -mag)
    x[6] = _logit(SCORE_THRESH * (1 + 4 * SCORE_MARGIN))
    x[7] = _logit(SCORE_THRESH * (1 - 4 * SCORE_MARGIN))
    near = np.abs(sigmoid64(x) - LOGIT_THRESH) < LOGIT_MARGIN  # nudged away, sign kept
    x[near] = np.where(x[near] < 0, -0.01, 0.01)
    c = rng.normal(0, 2, (nq, ncls)).astype(np.float32)
    top = np.float32(np.abs(c).max() + 6.0)
    for q in range(nq):
        if q == 4:
            if 0 <= min_class - 1 < ncls:
                c[q, min_class - 1] = top
        elif q == 5:
            if ncls >= 2:
                k1, k2 = (min_class - 1, int(rng.integers(min_class, ncls))) if 1 <= min_class < ncls else (0, ncls - 1)
                c[q, k1] = c[q, k2] = top
        elif ncls > min_class:
            c[q, int(rng.integers(min_class, ncls))] = top
    sem = rng.normal(0, 1, (N, ncls))
    sem = np.exp(sem - sem.max(1, keepdims=True))
    sem = (sem / sem.sum(1, keepdims=True)).astype(np.float32)
    # few-shot similarities: just above sim_thresh on the all-member row, just below on the row with exactly
    # npoint_thresh members (there the similarity decides), one negative (NaN score), the rest on both sides
    sim = np.array([SIM_THRESH * (1 + 4 * SCORE_MARGIN), 0.9, SIM_THRESH * (1 - 4 * SCORE_MARGIN), -0.2, 0.3, 0.8,
                    0.95, 0.61], np.float32)
    return StatsCase(name, x, c, sem, sim, LOGIT_THRESH, SCORE_THRESH, int(npoint_thresh), int(min_class), SIM_THRESH)


def make_stats_case(name, seed, N, ncls, min_class, npoint_thresh=None):
    """A case that meets its margins: re-drawn (never relaxed) until it does."""
    npoint_thresh = max(1, min(100, N // 2)) if npoint_thresh is None else npoint_thresh
    for attempt in range(32):
        c = _draw_stats(name, np.random.default_rng([seed, N, ncls, min_class, attempt]), N, ncls, min_class,
                        npoint_thresh)
        try:
            check_stats_margins(c)
        except AssertionError:
            continue
        return c
    raise AssertionError(f"{name}: no draw met the margins")


@functools.lru_cache(maxsize=None)
def stats_cases():
    out = {}
    for N in STATS_N:
        for ncls in (1, 2, 20):
            for min_class in (0, 4):
                name = f"N{N}-c{ncls}-m{min_class}"
                out[name] = make_stats_case(name, 11, N, ncls, min_class)
    return out


def depth(N):
    """Longest chain of fp32 additions behind one sum of the statistics kernels: a thread adds at most
    4 * ceil(N / 4096) terms, then 6 butterfly levels and 16 serial adds over the waves."""
    return 4 * -(-N // 4096) + 22


def score_rel_tol(N, ncls):
    """Twice the first-order bound on the score's relative error (the derivation is in tests/test_gpu_proposal_regimes.py)."""
    return (2 * depth(N) + ncls + 16) * 2.0 ** -23


def score_rel_tol_fs(N):
    """The few-shot score: one such mean times sqrtf(sim)."""
    return (depth(N) + 16) * 2.0 ** -23


BATCHED_STATS_N = {"empty-first": (0, 65, 4097, 1024), "empty-middle": (63, 1025, 0, 8193),
                   "empty-last": (4096, 1, 1023, 0)}
BATCHED_NPOINT_THRESH = 30


@functools.lru_cache(maxsize=None)
def batched_stats_cases():
    """name -> tuple of S = 4 StatsCase (one launch: the same thresholds, ncls = 20, min_class = 4).  The test lays the
    scenes' sem_prob side by side in one class-major sem_t, so every scene has its own foreground offset."""
    return {name: tuple(make_stats_case(f"{name}-s{b}-N{N}", 23 + b, N, 20, 4, BATCHED_NPOINT_THRESH)
                        for b, N in enumerate(Ns)) for name, Ns in BATCHED_STATS_N.items()}


# ---- select cases -----------------------------------------------------------------------------------------------------
SELECT_NQ = (0, 1, 63, 64, 65, 1023, 1024, 1025, 2049)  # a wave, one 1024-query pass, the start of a third pass
SELECT_FLAGS = ("all", "none", "alternating", "random")


class SelectCase(NamedTuple):
    name: str
    final: np.ndarray  # int32 [nq]
    cls_pred: np.ndarray  # int32 [nq]
    scores: np.ndarray  # fp32 [nq]


def _select_case(nq, flags, seed=0):
    rng = np.random.default_rng([31, nq, SELECT_FLAGS.index(flags), seed])
    final = {"all": np.ones(nq), "none": np.zeros(nq), "alternating": np.arange(nq) % 2,
             "random": rng.random(nq) < 0.3}[flags].astype(np.int32)
    return SelectCase(f"nq{nq}-{flags}", final, rng.integers(0, 20, nq).astype(np.int32),
                      rng.random(nq).astype(np.float32))


@functools.lru_cache(maxsize=None)
def select_cases():
    return {c.name: c for c in (_select_case(nq, f) for nq in SELECT_NQ for f in SELECT_FLAGS)}


@functools.lru_cache(maxsize=None)
def batched_select_cases():
    """name -> S = 3 SelectCase of one nq."""
    out = {}
    for nq in SELECT_NQ:
        out[f"nq{nq}-a"] = tuple(_select_case(nq, f) for f in ("all", "none", "alternating"))
        out[f"nq{nq}-b"] = (_select_case(nq, "random"), _select_case(nq, "all", 1), _select_case(nq, "random", 1))
    return out


# ---- scatter cases ----------------------------------------------------------------------------------------------------
SCATTER_N = (1, 255, 256, 257, 1023, 1024, 1025, 2049)  # a workgroup, one trip of a workgroup (4 x 256), a third block
SCATTER_NQ = 6


class ScatterCase(NamedTuple):
    name: str
    logits: np.ndarray  # fp32 [nq, N]
    sel: np.ndarray  # int32 [n_sel]: holds the first and the last query
    fg_idxs: np.ndarray  # int64 [N]: a sorted subset of the scene's points (never outside the scene)
    num_points: int
    logit_thresh: float

    def statement(self):
        return scatter_statement(self.logits, self.sel, self.fg_idxs, self.logit_thresh, self.num_points)


def _scatter_case(N, sel=(0, 2, 3, SCATTER_NQ - 1)):
    rng = np.random.default_rng([41, N])
    x = rng.normal(0, 3, (SCATTER_NQ, N)).astype(np.float32)
    near = np.abs(sigmoid64(x) - LOGIT_THRESH) < LOGIT_MARGIN
    x[near] = np.where(x[near] < 0, -0.01, 0.01)
    num_points = N + N // 2
    fg = np.sort(rng.choice(num_points, N, replace=False)).astype(np.int64)
    c = ScatterCase(f"N{N}", x, np.asarray(sel, np.int32), fg, num_points, LOGIT_THRESH)
    assert logit_margin_ok(c.logits, c.logit_thresh) and 0 <= fg.min() and fg.max() < num_points
    assert 0 in c.sel and SCATTER_NQ - 1 in c.sel
    return c


@functools.lru_cache(maxsize=None)
def scatter_cases():
    return {c.name: c for c in (_scatter_case(N) for N in SCATTER_N)}


BATCHED_SCATTER = {"empty-first": (257, 1, 1025, 256), "empty-middle": (255, 2049, 1024, 1023),
                   "empty-last": (1023, 256, 1, 2049)}  # the scene named by the key accepts no query (count 0)
BATCHED_SCATTER_EMPTY = {"empty-first": 0, "empty-middle": 2, "empty-last": 3}
BATCHED_SCATTER_PT0 = 17  # the first scene's point offset in the batch (every pt_off is nonzero)


@functools.lru_cache(maxsize=None)
def batched_scatter_cases():
    """name -> tuple of S = 4 (ScatterCase, count): the scene's first `count` entries of sel are its accepted queries."""
    out = {}
    for name, Ns in BATCHED_SCATTER.items():
        sels = [(0, SCATTER_NQ - 1), (SCATTER_NQ - 1, 0, 3), (0, 1, 2, 3, 4, SCATTER_NQ - 1), (2, 0, SCATTER_NQ - 1)]
        out[name] = tuple((_scatter_case(N, sels[b]), 0 if b == BATCHED_SCATTER_EMPTY[name] else len(sels[b]))
                          for b, N in enumerate(Ns))
    return out


# ---- intersection cases -----------------------------------------------------------------------------------------------
INTERSECTION_SIZES = ((1, 1), (2, 63), (3, 64), (3, 65), (5, 4097), (65, 700), (200, 3000), (64, 33281), (1024, 130))
# (64, 33281): 64 * 521 = 33344 packing waves; n = 200: 40000 pairs; n = 1024: 1048576 pairs -- all above the
# 4 * 8192 = 32768 that one batched launch covers without striding
BATCH_STRIDE_LIMIT = 4 * 8192


@functools.lru_cache(maxsize=None)
def intersection_cases():
    """name -> int32 0/1 masks [n, N]: row 0 all-zero and row 1 all-one where n allows (n = 1: all-one), the rest random;
    every N but 64 leaves a partial last word."""
    out = {}
    for n, N in INTERSECTION_SIZES:
        rng = np.random.default_rng([53, n, N])
        m = (rng.random((n, N)) < 0.3).astype(np.int32)
        m[0] = 1 if n == 1 else 0
        if n >= 2:
            m[1] = 1
        out[f"n{n}-N{N}"] = m
    return out


# ---- matrix NMS cases -------------------------------------------------------------------------------------------------
class NmsCase(NamedTuple):
    name: str
    masks: np.ndarray  # uint8 [n, N], every row non-empty
    scores: np.ndarray  # fp32 [n]
    cats: np.ndarray  # int64 [n]
    distinct: bool  # distinct scores (the reference's argsort leaves the order of equal scores unspecified)
    random: bool
    n_classes: int  # of the generator (0: hand-built)

    @property
    def n(self):
        return self.scores.shape[0]


def run_masks(rng, n, N):
    """The generator of tests/golden/make_greedy_nms_golden.py::run_masks: n overlapping runs of the N points (IoUs
    spread over [0, 1]), every third with a hole; distinct scores (k + 1) / (n + 1)."""
    masks = np.zeros((n, N), np.uint8)
    for i in range(n):
        ln = int(rng.integers(N // 50 + 1, N // 4 + 2))
        s = int(rng.integers(0, N - ln + 1))
        masks[i, s:s + ln] = 1
        if i % 3 == 0:
            masks[i, s + ln // 3:s + ln // 3 + ln // 10] = 0
    scores = ((rng.permutation(n) + 1) / (n + 1)).astype(np.float32)
    return masks, scores


NMS_RANDOM_SIZES = ((16, 300), (17, 300), (63, 700), (64, 700), (65, 700), (200, 3000), (1024, 4096))
NMS_HAND = ("one", "pair", "chain3", "chain3x", "dup3", "ties")


def _hand(name, N, runs, scores, cats):
    m = np.zeros((len(runs), N), np.uint8)
    for i, (a, b) in enumerate(runs):
        m[i, a:b] = 1
    s = np.asarray(scores, np.float32)
    return NmsCase(name, m, s, np.asarray(cats, np.int64), len(set(s.tolist())) == len(s), False, 0)


@functools.lru_cache(maxsize=None)
def nms_cases():
    out = {}
    for c in (_hand("one", 64, [(5, 20)], [0.7], [0]),
              _hand("pair", 64, [(0, 1), (0, 2)], [0.9, 0.8], [0, 0]),
              _hand("chain3", 64, [(0, 30), (10, 40), (18, 40)], [0.9, 0.8, 0.7], [0, 0, 0]),
              _hand("chain3x", 64, [(0, 30), (10, 40), (18, 40)], [0.9, 0.8, 0.7], [0, 1, 0]),
              _hand("dup3", 64, [(0, 20), (0, 20), (0, 20), (30, 50)], [0.9, 0.8, 0.7, 0.6], [0, 0, 0, 0]),
              _hand("ties", 320, [(64 * i, 64 * i + 64) for i in range(5)], [0.7, 0.9, 0.7, 0.7, 0.7], [0] * 5)):
        out[c.name] = c
    for n, N in NMS_RANDOM_SIZES:
        rng = np.random.default_rng([67, n, N])
        masks, scores = run_masks(rng, n, N)
        cats = rng.integers(0, 3, n).astype(np.int64)
        assert masks.any(1).all()
        out[f"r{n}"] = NmsCase(f"r{n}", masks, scores, cats, True, True, 3)
        out[f"r{n}-same"] = NmsCase(f"r{n}-same", masks, scores, np.zeros(n, np.int64), True, True, 1)
        out[f"r{n}-distinct"] = NmsCase(f"r{n}-distinct", masks, scores, np.arange(n, dtype=np.int64), True, True, n)
    return out


def nms_case_ids():
    return list(nms_cases())


def golden_case_ids():
    """The cases of tests/golden/matrix_nms_sizes.npz: hand-built with distinct scores, and the 3-class random ones."""
    return [k for k, c in nms_cases().items() if c.distinct and (not c.random or c.n_classes == 3)]


@functools.lru_cache(maxsize=None)
def _nms_inter(n, N):
    return intersections_statement(nms_cases()[f"r{n}"].masks)  # (the three category variants share the masks)


@functools.lru_cache(maxsize=None)
def nms_decayed(name, kernel, mutant=None):
    c = nms_cases()[name]
    inter = _nms_inter(*c.masks.shape) if c.random else None
    return decayed_scores(c.masks, c.scores, c.cats, kernel, SIGMA, mutant, inter)


@functools.lru_cache(maxsize=None)
def nms_sweep(name, kernel):
    """(thresholds, share of unusable gaps) of a case and kernel."""
    return sweep_thresholds(nms_decayed(name, kernel), nms_cases()[name].n)


def nms_picks(name, kernel, thresh, mutant=None):
    return picks_from_decayed(nms_decayed(name, kernel, mutant), nms_cases()[name].scores, thresh)
