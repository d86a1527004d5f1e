"""The spatial hash grid of csrc/geodesic.hip (build_point_grid, walked by k_knn_radius and k_ball_query_grid) restated in
numpy, point generators and the cases of the GPU tests (tests/test_gpu_grid_regimes.py), shared with the host test that
proves that the cases reach the regimes they are named for (tests/test_grid_cases_host.py).

The restatement is written from the comments and constants of geodesic.hip, not from its code: cells of radius x 1.001
(fp32), a point's cell is the floor of coordinate x (1 / cell) per axis, a cell's bucket is the xor of its three
coordinates times three large primes (uint32) masked to the table; the table is the smallest power of two that is at
least 1024 and at least 4 n, at most 2^26; its prefix scan takes 1024 buckets per workgroup, and more than 256 workgroups
make the scan's top level loop with a carry; both kernels hold 1024 in-radius candidates per query."""
from typing import NamedTuple

import numpy as np

KNN_CAP = BQG_CAP = 1024
T_MIN, T_MAX = 1 << 10, 1 << 26
SCAN_ITEMS = 1024  # buckets per workgroup of the prefix scan
SCAN_TOP = 256  # workgroup sums one pass of the scan's top level takes
PRIMES = (73856093, 19349663, 83492791)
RADIUS = 0.05  # the geodesic graph's
LATTICE_STEP = 2.0 ** -4


def table_size(n):
    t = T_MIN
    while t < 4 * n and t < T_MAX:
        t *= 2
    return t


def scan_blocks(t):
    return -(-t // SCAN_ITEMS)


def inv_cell(radius):
    return np.float32(1.0) / (np.float32(radius) * np.float32(1.001))


def cell_of(p, radius):
    """int64 [..., 3]: the cells of the fp32 points p."""
    p = np.asarray(p)
    assert p.dtype == np.float32
    return np.floor(p * inv_cell(radius)).astype(np.int64)  # (fp32 product, rounded once)


def bucket_of(cells, t):
    """int64 [...]: the buckets of the cells [..., 3] in a table of t buckets (uint32 arithmetic)."""
    c = (np.asarray(cells, dtype=np.int64) & 0xFFFFFFFF).astype(np.uint32)  # two's complement of the negative ones
    pr = np.asarray(PRIMES, dtype=np.uint32)
    with np.errstate(over="ignore"):
        h = (c[..., 0] * pr[0]) ^ (c[..., 1] * pr[1]) ^ (c[..., 2] * pr[2])
    assert h.dtype == np.uint32
    return (h & np.uint32(t - 1)).astype(np.int64)


# ---- points --------------------------------------------------------------------------------------------------------
TRANSLATION = (-37.5, 81.25, 100.0)  # metres


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def room(n, seed=3, small=False):
    """n points of a synthetic room scan (scene.make_scene: points on surfaces), in random order.  small: a 1.6 m room
    with one box, so that a few thousand points already have the density of a scan."""
    from geoformer_amd import scene

    kw = dict(room=(1.6, 1.6, 0.6), n_boxes=1) if small else {}
    p = scene.make_scene(n + n // 16 + 64, seed, **kw)["xyz"]
    assert p.shape[0] >= n
    return np.ascontiguousarray(p[_rng(n, seed, 0).permutation(p.shape[0])[:n]], dtype=np.float32)


def small_cube(n, seed=3):
    return _rng(n, seed, 1).uniform(0.0, 0.3, (n, 3)).astype(np.float32)


def signed(n, seed=3):
    return _rng(n, seed, 2).uniform(-0.2, 0.2, (n, 3)).astype(np.float32)


def lattice(n=None, seed=3, half=4):
    """The points LATTICE_STEP * (i, j, k), -half <= i, j, k <= half, in random order (the first n of them): with
    radius = LATTICE_STEP every interior point has exactly six neighbours at distance exactly the radius."""
    ax = np.arange(-half, half + 1, dtype=np.float32) * np.float32(LATTICE_STEP)
    p = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    p = p[_rng(p.shape[0], seed, 3).permutation(p.shape[0])]
    assert n is None or n <= p.shape[0]
    return np.ascontiguousarray(p[:n], dtype=np.float32)


def lattice_half(n):
    """The smallest lattice of at least n points."""
    half = 4
    while (2 * half + 1) ** 3 < n:
        half += 1
    return half


def translated(n, seed=3):
    """A (small) room moved far from the origin (fp32 sums: what the kernels and the brute force both see)."""
    return (room(n, seed, small=True) + np.asarray(TRANSLATION, dtype=np.float32)).astype(np.float32)


CLUSTER_EDGE = 0.02  # cube of a clump: all its points within 0.02 * sqrt(3) = 0.035 m of each other
CLUSTER_CLEAR = 0.12  # no background point closer than this to a clump's centre (per axis)


def clusters(n, sizes, seed=3):
    """(points [n,3], label [n]: the clump a point belongs to or -1, centres [len(sizes),3]): clumps of the given sizes
    inside cubes of CLUSTER_EDGE, 0.5 m apart, on a sparse uniform background in [-1,1]^3, in random order."""
    rng = _rng(n, seed, 4, *sizes)
    nb = n - sum(sizes)
    assert nb >= 0 and len(sizes) <= 27
    slots = np.stack(np.meshgrid(*[np.array([-0.5, 0.0, 0.5])] * 3, indexing="ij"), -1).reshape(-1, 3)
    centres = slots[rng.permutation(27)[:len(sizes)]] + rng.uniform(-0.05, 0.05, (len(sizes), 3))
    bg = np.zeros((0, 3))
    while bg.shape[0] < nb:
        c = rng.uniform(-1.0, 1.0, (2 * nb + 16, 3))
        far = np.ones(c.shape[0], bool)
        for ctr in centres:
            far &= np.abs(c - ctr).max(1) > CLUSTER_CLEAR
        bg = np.concatenate([bg, c[far]])
    parts, labels = [bg[:nb]], [np.full(nb, -1)]
    for i, s in enumerate(sizes):
        parts.append(centres[i] + rng.uniform(-CLUSTER_EDGE / 2, CLUSTER_EDGE / 2, (s, 3)))
        labels.append(np.full(s, i))
    perm = rng.permutation(n)
    p = np.concatenate(parts).astype(np.float32)[perm]
    return np.ascontiguousarray(p), np.concatenate(labels)[perm], centres.astype(np.float32)


def copies(n, count, seed=3):
    """small_cube with `count` exact copies of one point at random indices."""
    p = small_cube(n, seed)
    where = _rng(n, seed, 5).permutation(n)[:count]
    p[where] = p[where[0]]
    return p, np.sort(where)


KINDS = {"room": room, "small_cube": small_cube, "signed": signed, "translated": translated}


def points(kind, n, seed=3):
    if kind == "lattice":
        return lattice(n, seed, lattice_half(n))
    return KINDS[kind](n, seed)


def radius_of(kind, ball=False):
    """The radius a kind is used with (ball: by the ball query, whose rooms take the set abstraction's 0.2 m)."""
    if kind == "lattice":
        return LATTICE_STEP
    return 0.2 if ball and kind in ("room", "translated") else RADIUS


# ---- regime facts --------------------------------------------------------------------------------------------------
class Facts(NamedTuple):
    T: int
    scan_blocks: int
    nin: np.ndarray  # in-radius points per row (itself included), None where not counted
    shared_queries: int  # queries with two of their 27 cells in one bucket, at least one of the two occupied
    crowded_buckets: int  # buckets that hold more than one occupied cell


def in_radius_counts(xyz, radius):
    """Per point, the number of points with sqrt(d2) <= radius (fp32, the oracle's d2), itself included."""
    from oracle import oracle as orc

    n = xyz.shape[0]
    kk = min(n, KNN_CAP + 2)
    D2, _ = orc.knn(xyz, xyz, kk)
    nin = (np.sqrt(D2) <= np.float32(radius)).sum(1)
    assert kk == n or nin.max() < kk  # (otherwise a row may hold more than was looked at)
    return nin


def facts(xyz, radius, count_nin=True):
    n = xyz.shape[0]
    T = table_size(n)
    cells = cell_of(xyz, radius)
    occupied = np.unique(cells, axis=0)
    _, per_bucket = np.unique(bucket_of(occupied, T), return_counts=True)
    crowded = int((per_bucket > 1).sum())
    offs = np.stack(np.meshgrid(*[np.arange(-1, 2)] * 3, indexing="ij"), -1).reshape(27, 3)
    nb_cells = cells[:, None, :] + offs[None, :, :]  # [n,27,3]
    b = bucket_of(nb_cells, T)

    def key(c):
        c = c + (1 << 20)
        assert (c >= 0).all() and (c < (1 << 21)).all()
        return (c[..., 0] << 42) | (c[..., 1] << 21) | c[..., 2]

    occ = np.isin(key(nb_cells), key(occupied))  # [n,27]
    shared = 0
    for lo in range(0, n, 4096):
        bb, oo = b[lo:lo + 4096], occ[lo:lo + 4096]
        same = np.triu(bb[:, :, None] == bb[:, None, :], 1) & (oo[:, :, None] | oo[:, None, :])
        shared += int(same.any((1, 2)).sum())
    return Facts(T, scan_blocks(T), in_radius_counts(xyz, radius) if count_nin else None, shared, crowded)


# ---- the cases of the GPU tests ------------------------------------------------------------------------------------
KNN_K = (1, 2, 16, 63, 64)
SMALL_N = (1, 2, 3, 5, 200, 255, 256, 257)
SMALL_KINDS = ("small_cube", "signed")
COLLISION = (("small_cube", 200), ("signed", 255), ("lattice", 729))  # T = 1024: collisions are common

CLUSTER_N = 2200  # points of every cluster case (the same n: the overflow case and the call after it share a block)
CLUSTER_SIZES = (65, 300, 1024)
CLUSTER_K = (4, 64)
OVERFLOW_SIZE = KNN_CAP + 1
LATTICE_K = (4, 7, 64)
COPIES = (700, 200)  # n, copies

SHIFT_N = 6000  # translated / signed
LARGE_N = 70_000
LARGE_ROWS = 4096

BALL_N = (5, 255, 900, 6000)
BALL_M = (1, 3, 37, 256)
BALL_NSAMPLE = (1, 16, 64, 100)
BALL_KINDS = ("signed", "translated", "lattice")
BALL_CAP_NSAMPLE = (64, 100)

SA_N, SA_PICKS, SA_NSAMPLE, SA_RADIUS = 6000, 77, 16, 0.2
SA_SMALL_N = 900


def cluster_case(size):
    """A clump of `size` points (and one of 40) on a background."""
    return clusters(CLUSTER_N, (size, 40))


def ball_centres(xyz, m, seed=5):
    """m centres [m,3] for the point set: points of the set, points of the set moved by a fraction of a step (no point of
    the set), uniform ones in the bounding box; from m = 3 on centre 1 lies 50 m outside (no hit: its row is zeros)."""
    n = xyz.shape[0]
    rng = _rng(n, m, seed, 6)
    lo, hi = xyz.min(0), xyz.max(0)
    c = xyz[rng.integers(0, n, m)].copy()
    kind = np.arange(m) % 3
    c[kind == 1] += np.float32(LATTICE_STEP / 2) * rng.choice([-1.0, 1.0], ((kind == 1).sum(), 3)).astype(np.float32)
    c[kind == 2] = rng.uniform(lo, hi + 1e-6, ((kind == 2).sum(), 3)).astype(np.float32)
    if m >= 3:
        c[1] = hi + np.float32(50.0)
    return np.ascontiguousarray(c, dtype=np.float32)
