"""Furthest point sampling: the launch planner restated in numpy, a point generator and the sizes of the GPU tests
(tests/test_gpu_fps_regimes.py), shared with the host test that proves the table (tests/test_fps_plan_host.py).

The restatement is written from the comments and constants of csrc/pointops.hip, not from its planner code: a workgroup
has FPS_WAVES waves of which every fourth (wave 0's SIMD) holds no points; "~2.5 points per lane" decides the number of
cooperating workgroups, at most FPS_MAXG; the points per lane follow, and the smallest instantiation that holds them;
a launch takes as many point sets as keep all cooperating waves resident (1024 waves); ties are decided by the
reference's block size (oracle/gf_oracle.c orc_fps_block: the largest power of two <= n, capped at 512)."""
from typing import NamedTuple

import numpy as np

FPS_WAVES, FPS_MAXG, FPS_KPUB, FPS_K = 16, 16, 4, 16
FPS_PW = FPS_WAVES - FPS_WAVES // 4  # waves of a workgroup that hold points
LANES = FPS_PW * 64  # 768 point-holding lanes per workgroup
LADDER = (1, 2, 3, 4, 5, 6, 8, 12, 16, 20, 22)  # points per lane of the k_fps instantiations
RESIDENT_WAVES = 1024
N_MAX = FPS_MAXG * LANES * LADDER[-1]  # 270 336
INDEX_BITS = 22  # of the tie-break key


def oracle_block(n):
    """orc_fps_block"""
    p = 1
    while p * 2 <= n and p < 512:
        p *= 2
    return p


def plan_many(ns):
    """(ok, G, P, inst, bs_log2, per_launch) as int64 arrays over the sizes `ns` (ok False: the call refuses the size;
    the other columns are then meaningless)."""
    n = np.asarray(ns, dtype=np.int64)
    assert (n >= 1).all()
    G = np.clip(-(-(2 * n) // (5 * LANES)), 1, FPS_MAXG)  # ceil(n / (2.5 * 768))
    P = -(-n // (G * LANES))
    ok = (P <= LADDER[-1]) & (n < (1 << INDEX_BITS))
    ladder = np.asarray(LADDER, dtype=np.int64)
    inst = ladder[np.minimum(np.searchsorted(ladder, P, side="left"), len(ladder) - 1)]
    bs_log2 = np.minimum(np.floor(np.log2(n)).astype(np.int64), 9)
    per_launch = np.maximum(RESIDENT_WAVES // (G * FPS_WAVES), 1)
    return ok, G, P, inst, bs_log2, per_launch


class Plan(NamedTuple):
    G: int
    P: int
    inst: int
    bs_log2: int
    per_launch: int


def plan(n):
    """Plan of one size, None where the call refuses it."""
    cols = plan_many([n])
    return Plan(*(int(c[0]) for c in cols[1:])) if cols[0][0] else None


# ---- points --------------------------------------------------------------------------------------------------------
KINDS = ("room", "lattice", "sparse", "origin")
# |p|^2 <= 1e-3 is never picked (sampling_gpu.cu:104): three inside, the last one just outside (1.025e-3)
_NEAR_ORIGIN = np.array([[0.0, 0.0, 0.0], [0.02, 0.01, 0.0], [0.03, 0.0, 0.009], [-0.01, 0.02, 0.02], [0.03, 0.01, 0.005]],
                        dtype=np.float32)


def _room(rng, n):
    return rng.uniform([-4.0, -4.0, 0.0], [4.0, 4.0, 3.0], (n, 3)).astype(np.float32)


def points(n, seed, kind, origin0=False):
    """fp32 [n,3].  "room": uniform in [-4,4] x [-4,4] x [0,3].  "lattice": the same rounded to quarters -- exact distance
    ties everywhere, the (bit-reversed k mod bs, k) key decides.  "sparse": everything inside |p| < 0.015 (never picked)
    but about 40 points spread over the index range, 12 of them exact duplicates of one.  "origin": no point can be picked.
    n > 40: "room" and "lattice" get 30 exact duplicates of one point and five points at the origin's rim (four inside
    the rule, one outside) at random indices.  origin0: point 0 itself lies at the origin."""
    assert kind in KINDS
    rng = np.random.default_rng([n, seed, KINDS.index(kind)])
    if kind in ("room", "lattice"):
        p = _room(rng, n)
        if kind == "lattice":
            p = (np.round(p * 4) / 4).astype(np.float32)
        if n > 40:
            where = rng.permutation(n)[:35]
            p[where[:30]] = p[where[0]]
            p[where[30:]] = _NEAR_ORIGIN
    else:
        p = rng.uniform(-0.008, 0.008, (n, 3)).astype(np.float32)  # |p| <= 0.0139
        p[rng.permutation(n)[:max(n // 8, 1)]] = 0.0
        if kind == "sparse":
            k = 28 if n > 40 else max(n // 3, 1)
            where = np.unique(np.linspace(0, n - 1, k).astype(np.int64))
            if n > 40:
                where = np.unique(np.clip(where + rng.integers(-(n // 60), n // 60 + 1, where.shape[0]), 0, n - 1))
            p[where] = _room(rng, where.shape[0]) + np.float32(0.5)  # (clear of the origin)
            if n > 40:
                free = np.setdiff1d(np.arange(n), where)
                p[rng.permutation(free)[:12]] = p[where[where.shape[0] // 2]]
    if origin0:
        p[0] = 0.0
    return np.ascontiguousarray(p)


def eligible(p):
    """Which points can be picked.  (The generator keeps |p|^2 at least 1.9 % away from 1e-3, so fp32 rounding of the
    kernel's own sum cannot decide differently.)"""
    mag = (p.astype(np.float64) ** 2).sum(1)
    assert (np.abs(mag - 1e-3) > 1.5e-5).all()
    return mag > 1e-3


# ---- sizes ---------------------------------------------------------------------------------------------------------
class Size(NamedTuple):
    n: int
    G: int  # what the planner must answer for n: asserted by the host test and by every GPU case before it runs
    inst: int


G_SWEEP = tuple(Size(1920 * g, g, 3) for g in range(1, 16))
SMALL = (Size(1, 1, 1), Size(2, 1, 1), Size(3, 1, 1), Size(7, 1, 1), Size(100, 1, 1), Size(511, 1, 1), Size(512, 1, 1),
         Size(768, 1, 1), Size(769, 1, 2), Size(1023, 1, 2), Size(1536, 1, 2), Size(1537, 1, 3), Size(1921, 2, 2),
         Size(3073, 2, 3), Size(6144, 4, 2))
# G = 16: both ends of every instantiation (P = 7, 9, 13, 17, 21 leave slots empty on every lane)
LADDER16 = (Size(28801, 16, 3), Size(36864, 16, 3), Size(36865, 16, 4), Size(49152, 16, 4), Size(49153, 16, 5),
            Size(61440, 16, 5), Size(61441, 16, 6), Size(73728, 16, 6), Size(73729, 16, 8), Size(86017, 16, 8),
            Size(98304, 16, 8), Size(98305, 16, 12), Size(147456, 16, 12), Size(147457, 16, 16), Size(196608, 16, 16),
            Size(196609, 16, 20), Size(245760, 16, 20), Size(245761, 16, 22), Size(270336, 16, 22))
LADDER16_P = (3, 3, 4, 4, 5, 5, 6, 6, 7, 8, 8, 9, 12, 13, 16, 17, 20, 21, 22)
SIZES = G_SWEEP + SMALL + LADDER16
SIZE_KINDS = ("room", "lattice")


def picks_for(n):
    return 300 if n <= 150_000 else 200


PRODUCTION = (Size(49152, 16, 4), 2048)  # the eval forward's largest draw, at its number of picks

EDGE_SIZES = (Size(3000, 2, 2), Size(13440, 7, 3), Size(40000, 16, 4))
EDGE_M = (1, 2, 16, 17, 18)
EDGE_PICKS = 64  # more than "sparse" has points to pick
OVERDRAW = (Size(2000, 2, 2), 2100)  # m > n


class Batch(NamedTuple):
    b: int
    size: Size
    launches: tuple  # point sets per launch


BATCHES = (Batch(5, Size(30000, 16, 3), (4, 1)), Batch(9, Size(30000, 16, 3), (4, 4, 1)),
           Batch(65, Size(500, 1, 1), (64, 1)), Batch(6, Size(20000, 11, 3), (5, 1)))
BATCH_PICKS = 200

RESUME_SIZES = (Size(30000, 16, 3), Size(49152, 16, 4))
RESUME_BATCH = (2, Size(5000, 3, 3))
RESUME_M = 512
RESUME_M0 = (1, 2, 16, 17, 18, 33, 128, 256, 511, 512)

DRAW_FPS_M = 256
DRAW = ((45_000, Size(40000, 16, 4)), (400, Size(300, 1, 1)))  # (points drawn from, k)
DRAW_SHORT = (400, 200)  # k < fps_m: no sampling launch


def all_sizes():
    """Every Size a GPU case runs at."""
    return (SIZES + (PRODUCTION[0],) + EDGE_SIZES + (OVERDRAW[0],) + tuple(bt.size for bt in BATCHES) + RESUME_SIZES
            + (RESUME_BATCH[1],) + tuple(k for _, k in DRAW))
