"""Case builders of the tile stitch (postprocess.stitch_tiles_host, csrc/tile_stitch.hip), plain numpy, shared by
tests/test_tile_stitch_host.py and tests/test_gpu_tile_stitch.py: plans, random per-tile scores, hand-built tables, and
`brute_force`, the rule restated point by point and slot by slot, apart from postprocess.stitch_tiles_host."""
import numpy as np

from geoformer_amd import scene

MODES = ("core", "mean")


def uniform_plan(n=4000, extent=(9.0, 9.0), tile=3.0, halo=0.4, seed=5):
    """The plan of n uniform points in extent[0] x extent[1] m (n = 4000, 9 x 9 m, tile 3, halo 0.4: 3 x 3 tiles)."""
    rng = np.random.default_rng(seed)
    xyz = np.stack([rng.uniform(0, extent[0], n), rng.uniform(0, extent[1], n), rng.uniform(0, 1, n)], 1)
    return scene.tile_plan(xyz, tile, halo)


def gap_plan(n=600, seed=6):
    """9 x 1 m in three tiles of 3 m, no point with 2.5 < x < 6.5: the middle tile is empty."""
    rng = np.random.default_rng(seed)
    x = np.concatenate([[0.0, 9.0], rng.uniform(0, 2.5, n // 2), rng.uniform(6.5, 9, n - n // 2)])
    xyz = np.stack([x, rng.uniform(0, 1, x.size), np.zeros(x.size)], 1)
    plan = scene.tile_plan(xyz, 3.0, 0.4)
    assert plan.T == 3 and plan.offsets[1] == plan.offsets[2] and plan.offsets[1] > 0 and plan.offsets[3] > plan.offsets[2]
    return plan


def edge_plan(seed=7):
    """3 x 3 tiles of 3 m, halo 0.4, with points on the scan's closed upper edge, on tile borders and at the corners
    where four tiles meet; returns (plan, ids of the corner points)."""
    rng = np.random.default_rng(seed)
    fixed = np.array([[0, 0], [9, 9], [9, 0], [0, 9], [9, 4.5], [4.5, 9], [3, 3], [6, 6], [3, 6], [6, 3], [3.2, 5.9],
                      [2.7, 2.7], [3, 1], [1, 6], [2.6, 1], [3.4, 1]], np.float64)
    more = rng.uniform(0, 9, (300, 2))
    xy = np.concatenate([fixed, more])
    plan = scene.tile_plan(np.concatenate([xy, np.zeros((xy.shape[0], 1))], 1), 3.0, 0.4)
    assert plan.T == 9
    return plan, np.arange(6, 12)


def random_scores(plan, C, seed, empty="none"):
    """Per tile float32 [n_s, C] standard normal scores; an empty tile is None (empty="none") or [0, C] ("zero")."""
    rng = np.random.default_rng(seed)
    out = []
    for s in range(plan.T):
        n_s = int(plan.offsets[s + 1] - plan.offsets[s])
        x = rng.standard_normal((n_s, C)).astype(np.float32)
        out.append(None if n_s == 0 and empty == "none" else x)
    return out


def hand_plan():
    """A hand-built table over 3 tiles of 2, 3 and 2 points and 5 points of a scan: a point in three tiles (count 3), a
    point without any slot, a point whose core tile is its second slot, one whose core slot names no row (local index
    out of the tile), and one with a slot in front of the core's that names no tile."""
    tile_of = np.array([[0, 1, 2, -1], [-1, -1, -1, -1], [0, 2, -1, -1], [1, 2, -1, -1], [-1, 1, -1, -1]], np.int32)
    local_of = np.array([[1, 2, 0, 0], [0, 0, 0, 0], [0, 1, 0, 0], [3, 0, 0, 0], [0, 1, 0, 0]], np.int32)
    core_of = np.array([1, -1, 2, 1, 1], np.int32)
    # rows (1, 3) and (-1, 0) are deliberately no rows: the statement skips them; they are never given to the kernel
    return scene.TilePlan(tile_of, local_of, core_of, np.array([0, 2, 5, 7], np.int64), np.zeros(7, np.int64), 3, 1,
                          (1.0, 1.0))


def hand_plan_in_range():
    """hand_plan's first three points only: every slot names a row (what the GPU test launches)."""
    p = hand_plan()
    return p._replace(tile_of=p.tile_of[:3].copy(), local_of=p.local_of[:3].copy(), core_of=p.core_of[:3].copy())


def brute_force(plan, per_tile_scores, mode, C):
    """The rule, point by point: float32 [N, C]."""
    assert mode in MODES
    T = plan.T
    out = np.zeros((plan.N, C), np.float32)

    def row(s, l):
        if not 0 <= s < T or per_tile_scores[s] is None or not 0 <= l < per_tile_scores[s].shape[0]:
            return None
        return per_tile_scores[s][l]

    for g in range(plan.N):
        if mode == "core":
            for j in range(4):
                if plan.tile_of[g, j] == plan.core_of[g]:
                    v = row(int(plan.tile_of[g, j]), int(plan.local_of[g, j]))
                    if v is not None:
                        out[g] = v
                    break
            continue
        acc, count = None, 0
        for j in range(4):
            v = row(int(plan.tile_of[g, j]), int(plan.local_of[g, j]))
            if v is None:
                continue
            if acc is None:
                acc = v.astype(np.float32).copy()
            else:
                for c in range(C):
                    acc[c] = np.float32(acc[c]) + np.float32(v[c])
            count += 1
        if count:
            for c in range(C):
                out[g, c] = np.float32(acc[c]) / np.float32(count)
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def scan(rooms=4, n=6000):
    """`rooms` small rooms side by side along x, 1.7 m apart: one raw [rooms * n, 8] scan of about 6.7 x 1.6 m (the scan
    of tests/test_gpu_tile_merge.py, restated)."""
    parts = []
    for i in range(rooms):
        r = scene.make_raw_scene(n + 500 * i, 60 + i, n_boxes=1, room=(1.6, 1.6, 0.6))
        r[:, 0] += 1.7 * i
        r[:, 7] = np.where(r[:, 7] >= 0, r[:, 7] + 100 * i, r[:, 7])
        parts.append(r)
    return np.concatenate(parts)
