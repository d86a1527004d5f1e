"""Inputs of the mask-splitting statement (postprocess.mask_components_host), shared by the host tests and the GPU
tests: hand-made cases with the ids the statement gives by its text, synthetic graphs under several masks, and the
lattice clouds on which the statement is sklearn's DBSCAN."""
import numpy as np

from tests.oversegment_cases import _rows


def _case(lists, masks, pick, min_samples, min_points, comp, tab, deg=None):
    I, d = _rows(lists)
    if deg is not None:
        d = np.asarray(deg, np.int32)
    return dict(masks=np.asarray(masks, np.int32), pick=np.asarray(pick, np.int64), I=I, deg=d, min_samples=min_samples,
                min_points=min_points, comp=np.asarray(comp, np.int32), tab=np.asarray(tab, np.int32))


def _clique(members, extra=()):
    """Row lists of a clique: every member lists itself, then the others (and `extra`)."""
    return {i: [i] + [j for j in members if j != i] + list(extra) for i in members}


def path():
    """The path 0..99 (each point lists itself and its successor) under mask A (all points) and mask B (all but point
    50): A is one cluster, B falls into the clusters 0 (50 points) and 51 (49 points)."""
    lists = [[i, i + 1] for i in range(99)] + [[99]]
    a = np.ones(100, np.int32)
    b = a.copy()
    b[50] = 0
    comp_b = np.r_[np.zeros(50), -1, np.full(49, 51)]
    return _case(lists, [a, b], [0, 1], 1, 1, [np.zeros(100), comp_b], [[100, 1, 100, 0, 100], [99, 2, 99, 0, 50]])


def picks():
    """The path's masks with a pick past the last row, a negative pick and row 1 picked twice."""
    c = path()
    none = np.full(100, -1)
    return dict(c, pick=np.asarray([1, 7, -1, 1, 0], np.int64),
                comp=np.asarray([c["comp"][1], none, none, c["comp"][1], c["comp"][0]], np.int32),
                tab=np.asarray([c["tab"][1], [0, 0, 0, -1, 0], [0, 0, 0, -1, 0], c["tab"][1], c["tab"][0]], np.int32))


def core_threshold():
    """min_samples = 3.  Point 0 lists two members (cnt 3: core), point 1 lists one (cnt 2 = min_samples - 1: a border
    point of 0's cluster, through its own row), point 2 lists nobody (0 lists it, it does not list 0 back: noise),
    point 3 lists 0 and 1 (cnt 3: core, joined to 0 by its own row alone)."""
    lists = [[0, 1, 2], [1, 0], [2], [3, 0, 1]]
    return _case(lists, [[1, 1, 1, 1]], [0], 3, 1, [[0, 0, -1, 0]], [[4, 1, 3, 0, 3]])


def contested_border():
    """min_samples = 4: the cliques {0..3} and {4..7} are two clusters; point 8 (cnt 3) lists a core of cluster 4 BEFORE a
    core of cluster 0 and goes to the lower id."""
    rows = _clique(range(4)) | _clique(range(4, 8)) | {8: [8, 5, 2]}
    return _case([rows[i] for i in range(9)], [[1] * 9], [0], 4, 1, [[0, 0, 0, 0, 4, 4, 4, 4, 0]], [[9, 2, 9, 0, 5]])


def one_way_border():
    """min_samples = 4: core 0 lists point 4, which does not list it back: 4 is noise."""
    rows = _clique(range(4)) | {4: [4]}
    rows[0] = rows[0] + [4]
    return _case([rows[i] for i in range(5)], [[1] * 5], [0], 4, 1, [[0, 0, 0, 0, -1]], [[5, 1, 4, 0, 4]])


def min_points_edge():
    """min_samples = 4, min_points = 6: the clique {0..3} with the border points 8, 9 has 6 points and stays; the clique
    {4..7} with the border point 10 has 5 and is dissolved, border point included."""
    rows = _clique(range(4)) | _clique(range(4, 8)) | {8: [8, 0], 9: [9, 1], 10: [10, 4]}
    comp = [0, 0, 0, 0, -1, -1, -1, -1, 0, 0, -1]
    return _case([rows[i] for i in range(11)], [[1] * 11], [0], 4, 6, [comp], [[11, 1, 6, 0, 6]])


def largest_tie():
    """min_samples = 4.  Mask 0: two cliques of 4, the tie goes to the smaller id.  Mask 1: the second clique has a border
    point more and is the largest."""
    rows = _clique(range(4)) | _clique(range(4, 8)) | {8: [8, 6]}
    m0 = [1] * 8 + [0]
    m1 = [1] * 9
    return _case([rows[i] for i in range(9)], [m0, m1], [0, 1], 4, 1,
                 [[0, 0, 0, 0, 4, 4, 4, 4, -1], [0, 0, 0, 0, 4, 4, 4, 4, 4]], [[8, 2, 8, 0, 4], [9, 2, 9, 4, 5]])


def odd_rows():
    """min_samples = 3.  Point 0 lists point 1 twice (each counts: cnt 3, core); point 1 has padding inside its row and
    an entry >= N (cnt 2: border of 0); point 2 lists only itself, four times (cnt 1: noise); point 3 lists nothing
    valid; point 4 lists point 0 three times behind a deg of 0, so only its column 0 is read (noise)."""
    lists = [[0, 1, 1, -1], [1, -1, 0, 9], [2, 2, 2, 2], [3, -1, -7, 2 ** 30], [4, 0, 0, 0]]
    return _case(lists, [[1] * 5], [0], 3, 1, [[0, 0, -1, -1, -1]], [[5, 1, 2, 0, 2]], deg=[3, 3, 3, 3, 0])


HAND_CASES = {"path": path, "picks": picks, "core_threshold": core_threshold, "contested_border": contested_border,
              "one_way_border": one_way_border, "min_points_edge": min_points_edge, "largest_tie": largest_tie,
              "odd_rows": odd_rows}


# ---- synthetic graphs, each under three masks at once ---------------------------------------------------------------------
def _graphs():
    """name -> (row lists, an articulation point): graphs whose components depend on which points a mask leaves out."""
    rng = np.random.default_rng(5)
    g = {}
    perm = rng.permutation(5000)
    rows = [None] * 5000
    for a, b in zip(perm[:-1], perm[1:]):
        rows[a] = [a, b]
    rows[perm[-1]] = [perm[-1]]
    g["path_shuffled"] = (rows, int(perm[2500]))  # long finds; without the middle point: two halves
    g["star"] = ([[0] + list(range(1, 64))] + [[i, 0] for i in range(1, 400)], 0)  # a 64-wide hub holds 399 leaves
    clique = [list(range(10)) for _ in range(10)] + [list(range(10, 20)) for _ in range(10)]
    clique[3] = clique[3] + [14]  # 3 lists 14, 14 does not list 3: the only link of the two cliques
    g["cliques_one_way"] = (clique, 3)
    g["padding_inside"] = ([[i, -1, (i + 1) % 40, -1, -1, (i + 7) % 40] for i in range(40)]
                           + [[i, -1, -1, -1, -1, -1] for i in range(40, 60)], 7)
    g["self_loops"] = ([[i, i, i, i + 1 if i % 10 != 9 else i] for i in range(50)], 4)
    n = 64
    g["out_of_range"] = ([[i, n + 5, (i + 1) % 32 if i < 32 else i, 2 ** 30, -7, n] for i in range(n)], 9)
    return g


GRAPHS = _graphs()


def graph_inputs(name):
    """(masks int32 [3, N]: all points / a random half / all but the articulation point, pick, I, deg) of a graph."""
    lists, cut = GRAPHS[name]
    I, deg = _rows(lists)
    n = len(lists)
    masks = np.ones((3, n), np.int32)
    masks[1] = np.random.default_rng(11).random(n) < 0.5
    masks[2, cut] = 0
    return masks, np.arange(3, dtype=np.int64), I, deg


def ring_inputs(n, p, density, seed=0):
    """A ring of n points (each lists itself, its successor and its predecessor) under p random masks."""
    i = np.arange(n)
    I = np.stack([i, (i + 1) % n, (i - 1) % n], 1).astype(np.int32)
    masks = (np.random.default_rng(seed).random((p, n)) < density).astype(np.int32)
    return masks, np.arange(p, dtype=np.int64), I, np.full(n, 2, np.int32)


# ---- lattice clouds: the statement is sklearn's DBSCAN ----------------------------------------------------------------------
LATTICE_EPS = 0.075  # between the lattice distances 0.0707 and 0.0866: no fp32 decision is near it
LATTICE_K = 32       # against a maximum degree of 19 (6 + 12 neighbours and the point itself)


def lattice_cloud(seed, keep=0.5):
    """(xyz fp32 [n, 3]: a random subset of a 14^3 lattice of spacing 0.05, member bool [n]: 2/3 of the points)."""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(*[np.arange(14) * 0.05] * 3, indexing="ij"), -1).reshape(-1, 3)
    xyz = g[rng.random(len(g)) < keep].astype(np.float32)
    return xyz, rng.random(len(xyz)) < 2 / 3


def brute_rows(xyz, eps=LATTICE_EPS, k=LATTICE_K):
    """Complete rows by brute force in float64: every point within eps, itself first, then by index."""
    x = xyz.astype(np.float64)
    d = np.linalg.norm(x[:, None] - x[None], axis=-1)
    lists = [[i] + [int(j) for j in np.nonzero(d[i] <= eps)[0] if j != i] for i in range(len(x))]
    assert max(len(r) for r in lists) < k  # no row is truncated
    I = np.full((len(x), k), -1, np.int32)
    for i, r in enumerate(lists):
        I[i, :len(r)] = r
    return I, np.asarray([len(r) - 1 for r in lists], np.int32)


def sklearn_ids(xyz, member, eps, min_samples):
    """int32 [n]: sklearn's DBSCAN of the member points, every cluster named by its smallest core index, -1 elsewhere."""
    from sklearn.cluster import DBSCAN

    idx = np.nonzero(member)[0]
    want = np.full(len(xyz), -1, np.int32)
    if len(idx) == 0:
        return want
    db = DBSCAN(eps=eps, min_samples=min_samples).fit(xyz[idx].astype(np.float64))
    core = np.zeros(len(idx), bool)
    core[db.core_sample_indices_] = True
    for c in range(db.labels_.max() + 1):
        want[idx[db.labels_ == c]] = idx[(db.labels_ == c) & core].min()
    return want
