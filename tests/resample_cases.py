"""Cases shared by tests/test_resample_host.py (CPU: each case reaches the regime it is named for) and
tests/test_gpu_resample.py (GPU: csrc/resample.hip against the statements, bit for bit)."""
import functools

import numpy as np

from geoformer_amd import scene

MODES = ("first", "center")
CELLS = (0.002, 0.1, 0.25)
# (points asked for, seed) -> {cell: (cells M, most points in a cell)} with origin = the minimum corner
SCENES = {(4000, 1): {0.001: (4094, 1), 0.002: (4094, 1), 0.1: (3944, 3), 0.25: (1230, 12)},
          (20000, 3): {0.001: (19950, 1), 0.002: (19950, 1), 0.1: (6574, 12), 0.25: (955, 68)}}
SCENE_POINTS = {(4000, 1): 4094, (20000, 3): 19950}


@functools.lru_cache(maxsize=None)
def _raw(n, seed):
    r = scene.make_raw_scene(n, seed=seed)
    r.setflags(write=False)
    return r


def raw_scene(n, seed):
    return _raw(n, seed)


def room(n, seed):
    """float32 [N, 3] of make_raw_scene(n, seed)."""
    return np.ascontiguousarray(_raw(n, seed)[:, :3], dtype=np.float32)


def prefix(N):
    """The first N points of the larger scene."""
    return room(20000, 3)[:N].copy()


def one_cell(N=3000, seed=5):
    """N points inside one cell of 1.0 (all contention on one slot)."""
    rng = np.random.default_rng(seed)
    return (rng.random((N, 3)) * 0.9 + 0.05).astype(np.float32)


def carry(N=70000, seed=6):
    """More than 65 536 points, so the rank's scan of 256 block sums carries; about a third of the points open a cell."""
    rng = np.random.default_rng(seed)
    return (rng.random((N, 3)) * np.array([6.0, 5.0, 2.5])).astype(np.float32)


def shuffled(seed=7):
    """The smaller scene in a random order: the order of first occurrence is not the order of the keys."""
    x = room(4000, 1)
    return x[np.random.default_rng(seed).permutation(x.shape[0])].copy()


def faces(seed=8):
    """(xyz, origin): points exactly on the faces of cells of 0.125: origin + k * 0.125, exact in float32."""
    rng = np.random.default_rng(seed)
    origin = np.array([-2.0, 1.5, 0.25], np.float32)
    k = rng.integers(0, 12, (2000, 3)).astype(np.float32)
    x = origin + k * np.float32(0.125)
    assert np.array_equal((x - origin) / np.float32(0.125), k)
    return x.astype(np.float32), origin


def copies(K=200, seed=9):
    """The smaller scene's first 500 points with K exact copies of point 17 spread among them: ties in center mode."""
    rng = np.random.default_rng(seed)
    x = room(4000, 1)[:500]
    x = np.concatenate([x, np.repeat(x[17:18], K, 0)])
    perm = rng.permutation(x.shape[0])
    return x[perm].copy(), np.sort(np.nonzero((x[perm] == x[17]).all(1))[0])


def translated(offset=100.0):
    return room(4000, 1) + np.float32(offset)


def keys_of(xyz, cell, origin=None):
    """int64 cell keys as the statement forms them."""
    origin = xyz.min(0) if origin is None else origin
    c = np.floor((xyz - origin) / np.float32(cell)).astype(np.int64)
    return c[:, 0] | c[:, 1] << 21 | c[:, 2] << 42


def unique_formulation(xyz, cell, origin=None):
    """(first int32 [M], cell_of int32 [N], count int32 [M]) another way: np.unique on the keys, re-ordered by first
    index."""
    _, first, inv, cnt = np.unique(keys_of(xyz, cell, origin), return_index=True, return_inverse=True, return_counts=True)
    order = np.argsort(first)
    number = np.empty_like(order)
    number[order] = np.arange(order.shape[0])
    return first[order].astype(np.int32), number[inv.reshape(-1)].astype(np.int32), cnt[order].astype(np.int32)


def center_loop(xyz, cell, cell_of, M, origin=None):
    """rep of center mode by a loop over the cells, float32 scalar by scalar."""
    origin = xyz.min(0) if origin is None else origin
    cell = np.float32(cell)
    c = np.floor((xyz - origin) / cell)
    rep = np.empty(M, np.int32)
    for m in range(M):
        best = None
        for i in np.nonzero(cell_of == m)[0]:
            d = [np.float32(xyz[i, a] - np.float32(origin[a] + np.float32(np.float32(c[i, a] + np.float32(0.5)) * cell)))
                 for a in range(3)]
            d2 = np.float32(np.float32(np.float32(d[0] * d[0]) + np.float32(d[1] * d[1])) + np.float32(d[2] * d[2]))
            if best is None or (d2, i) < best:
                best = (d2, i)
        rep[m] = best[1]
    return rep


# ---- nearest point ---------------------------------------------------------------------------------------------------
NP_SIZES = (1, 63, 65, 1000, 5000)


def cloud(n, seed=11):
    """The first n points of the larger scene, shuffled."""
    x = room(20000, 3)
    return x[np.random.default_rng(seed).permutation(x.shape[0])[:n]].copy()


def jittered(xyz, Q, scale, seed=12):
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, xyz.shape[0], Q)
    return (xyz[pick] + rng.normal(0, scale, (Q, 3)).astype(np.float32)).astype(np.float32)


def lattice(side=9):
    """A quarter-unit lattice, exact in float32: neighbours are exactly 0.25 apart (d2 == r2 at max_dist = 0.25)."""
    g = np.arange(side, dtype=np.float32) * np.float32(0.25)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)


def lattice_with_holes(side=9, seed=13):
    """(queries, points): the lattice's points as queries against the lattice without a third of them: a query whose own
    point is gone has only candidates at exactly max_dist."""
    x = lattice(side)
    keep = np.random.default_rng(seed).random(x.shape[0]) > 1 / 3
    return x, x[keep].copy()


def lattice_midpoints(side=9):
    """Midpoints of the lattice's x edges: two lattice points at exactly 0.125, the index decides."""
    x = lattice(side)
    return (x[x[:, 0] < (side - 1) * 0.25] + np.array([0.125, 0, 0], np.float32)).astype(np.float32)


def straddling(max_dist=0.05, n=400, seed=14):
    """(queries, points, partner): pairs on both sides of a face of the grid's cells (cell = max_dist * 1.001 from the
    points' minimum corner), a little less than max_dist apart along the axis that crosses the face."""
    rng = np.random.default_rng(seed)
    cell = np.float64(np.float32(max_dist)) * 1.001
    lo = np.zeros(3)
    k = rng.integers(1, 40, (n, 3))
    axis = rng.integers(0, 3, n)
    p = (k + rng.random((n, 3)) * 0.9 + 0.05) * cell      # somewhere inside cell k
    q = p.copy()
    gap = max_dist * (1 - rng.random(n) * 1e-3 - 1e-5)    # just under max_dist
    for i in range(n):
        a = axis[i]
        face = (k[i, a] + 1) * cell
        p[i, a] = face - gap[i] * 0.5
        q[i, a] = face + gap[i] * 0.5
    pts = np.concatenate([lo[None], p]).astype(np.float32)  # (the corner fixes the grid's origin)
    return q.astype(np.float32), pts, np.arange(1, n + 1)
