"""Case builders of the tile merge (scene.tile_plan, postprocess.merge_tiles_host, csrc/tile_merge.hip), plain numpy,
shared by tests/test_tile_merge_host.py and tests/test_gpu_tile_merge.py.  A case is a dict: plan (scene.TilePlan),
per_tile (per tile (cls int64 [n_rows], scores fp32 [n_rows], masks int32 [n_rows, n_s], pick int64 [p_s]), or
([], [], [], empty pick) for a tile without proposals), kw (iom / min_shared), and what the case expects where it is
built to an exact outcome."""
import numpy as np

from geoformer_amd import scene

NONE = ([], [], [], np.zeros(0, np.int64))


def strip(n, x0, x1, y0=0.0, y1=1.0, seed=0):
    """n points uniform in [x0, x1] x [y0, y1] x [0, 1] (float64)."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(x0, x1, n), rng.uniform(y0, y1, n), rng.uniform(0, 1, n)], 1)


def corners(x0, x1, y0=0.0, y1=1.0):
    """Two points that pin the extent of a scan."""
    return np.array([[x0, y0, 0.0], [x1, y1, 0.0]])


def build(xyz, tile, halo, rows, kw=None, decoys=1, reverse=True, **expect):
    """A case from rows = [(tile, ids of the scan's points, class, score), ...]: a row holds those of the ids that lie
    in its tile.  Every tile with rows gets `decoys` unpicked all-ones rows in front, and its picks are listed in
    reverse row order when `reverse` (pick is an indirection, not a range)."""
    plan = scene.tile_plan(xyz, tile, halo)
    N = plan.N
    per_tile = []
    for s in range(plan.T):
        mine = [r for r in rows if r[0] == s]
        n_s = int(plan.offsets[s + 1] - plan.offsets[s])
        if not mine:
            per_tile.append(NONE)
            continue
        member = np.zeros(N, bool)
        member[plan.points(s)] = True
        masks = np.ones((decoys + len(mine), n_s), np.int32)
        cls = np.full(decoys + len(mine), 3, np.int64)
        scores = np.full(decoys + len(mine), 0.99, np.float32)
        order = list(range(len(mine)))[::-1] if reverse else list(range(len(mine)))
        pick = np.zeros(len(mine), np.int64)
        for rank, (_, ids, c, sc) in enumerate(mine):
            at = decoys + order[rank]
            sel = np.zeros(N, bool)
            sel[np.asarray(ids, np.int64)] = True
            masks[at] = (sel & member)[plan.points(s)] * (1 + rank % 3)  # any nonzero is a member
            cls[at], scores[at], pick[rank] = c, sc, at
        per_tile.append((cls, scores, masks, pick))
    return dict(plan=plan, per_tile=per_tile, kw=dict(kw or {}), **expect)


def in_box(xyz, x0, x1, y0=-np.inf, y1=np.inf):
    return np.nonzero((xyz[:, 0] >= x0) & (xyz[:, 0] <= x1) & (xyz[:, 1] >= y0) & (xyz[:, 1] <= y1))[0]


def _two_tiles(n=3000, seed=1):
    """8 x 1 m, two tiles of 4 m, halo 0.5: the shared region is 3.5 <= x < 4.5."""
    return np.concatenate([corners(0, 8), strip(n, 0, 8, seed=seed)])


def hand_cases():
    """name -> case, each built to an outcome stated in `groups` (the rows of every instance) where it is exact."""
    out = {}
    xyz = np.concatenate([corners(0, 3), strip(1500, 0, 3, seed=2)])
    out["single_tile"] = build(xyz, 4.0, 0.5, [(0, in_box(xyz, 0, 1), 5, 0.3), (0, in_box(xyz, 0.5, 2), 5, 0.9),
                                               (0, in_box(xyz, 2, 3), 7, 0.9), (0, [], 7, 0.1)],
                               groups=[[0], [1], [2], [3]])
    xyz = _two_tiles()
    obj = in_box(xyz, 3.0, 5.0)
    out["halo_zero"] = build(xyz, 4.0, 0.0, [(0, obj, 5, 0.5), (1, obj, 5, 0.6)], groups=[[0], [1]])
    out["across_border"] = build(xyz, 4.0, 0.5, [(0, obj, 5, 0.5), (0, in_box(xyz, 0, 1), 5, 0.8), (1, obj, 5, 0.6)],
                                 groups=[[0, 2], [1]])
    out["other_class"] = build(xyz, 4.0, 0.5, [(0, obj, 5, 0.5), (1, obj, 6, 0.6)], groups=[[0], [1]])
    # the object ends 0.3 m behind the border: tile 0 holds all of it, tile 1 only the part from 3.5 m on.  Inside the
    # shared region both hold the same points, so the rows merge; IoU of the two masks (part / whole, about 0.35)
    # would not reach 0.5
    whole = in_box(xyz, 2.0, 4.3)
    out["truncated_part"] = build(xyz, 4.0, 0.5, [(0, whole, 5, 0.5), (1, whole, 5, 0.6)], groups=[[0, 1]],
                                  part=in_box(xyz, 3.5, 4.3), whole=whole)
    xyz3 = np.concatenate([corners(0, 12), strip(4000, 0, 12, seed=3)])
    long = in_box(xyz3, 1.0, 11.0, 0.2, 0.8)
    out["chain3"] = build(xyz3, 4.0, 0.5, [(0, long, 9, 0.2), (1, long, 9, 0.7), (2, long, 9, 0.4),
                                            (2, in_box(xyz3, 9, 12, 0.85, 1.0), 9, 0.95)], groups=[[0, 1, 2], [3]])
    out["tile_without_picks"] = build(xyz3, 4.0, 0.5, [(0, long, 9, 0.2), (2, long, 9, 0.4)], groups=[[0], [1]])
    gap = np.concatenate([corners(0, 12), strip(1500, 0, 3.4, seed=4), strip(1500, 8.6, 12, seed=5)])
    out["empty_tile"] = build(gap, 4.0, 0.5, [(0, in_box(gap, 1, 3.4), 4, 0.5), (2, in_box(gap, 8.6, 10), 4, 0.6)],
                              groups=[[0], [1]])
    # exact counts: the first k shared points in both rows
    zone = in_box(xyz, 3.5, 4.49)
    left, right = in_box(xyz, 1.0, 3.0), in_box(xyz, 5.0, 7.0)
    for k in (19, 20):
        out[f"min_shared_{k}"] = build(xyz, 4.0, 0.5, [(0, np.concatenate([left, zone[:k]]), 5, 0.5),
                                                        (1, np.concatenate([right, zone[:k]]), 5, 0.6)],
                                       kw=dict(min_shared=20, iom=0.5), groups=[[0, 1]] if k == 20 else [[0], [1]])
    # the ratio: row a has 40 shared points, row b 50, inter 20 (exactly iom * 40) or 19
    for k in (20, 19):
        a = np.concatenate([left, zone[:40]])
        b = np.concatenate([right, zone[40 - k:90 - k]])
        out[f"ratio_{k}_of_40"] = build(xyz, 4.0, 0.5, [(0, a, 5, 0.5), (1, b, 5, 0.6)], kw=dict(min_shared=1, iom=0.5),
                                        groups=[[0, 1]] if k == 20 else [[0], [1]], inter=k, small=40)
    return out


def random_case(seed, N, extent, tile, halo, picks, n_objects=12, kw=None):
    """A scan of N uniform points over extent = (ex, ey) with n_objects discs as objects; every tile picks the objects
    that reach into it (their points inside the tile, a few dropped) and fills up to picks(s) rows with random discs.
    picks: an int, or a list with one count per tile (cycled)."""
    rng = np.random.default_rng(seed)
    xyz = np.concatenate([corners(0, extent[0], 0, extent[1]),
                          np.stack([rng.uniform(0, extent[0], N - 2), rng.uniform(0, extent[1], N - 2),
                                    rng.uniform(0, 1, N - 2)], 1)])
    plan = scene.tile_plan(xyz, tile, halo)
    centres = np.stack([rng.uniform(0, extent[0], n_objects), rng.uniform(0, extent[1], n_objects)], 1)
    radii = rng.uniform(0.3, 1.5, n_objects)
    classes = rng.integers(4, 8, n_objects)
    rows = []
    for s in range(plan.T):
        want = picks if isinstance(picks, int) else picks[s % len(picks)]
        idx = plan.points(s)
        mine = []
        for o in range(n_objects):
            if len(mine) == want:
                break
            ids = idx[((xyz[idx, :2] - centres[o]) ** 2).sum(1) <= radii[o] ** 2]
            if ids.size:
                mine.append((s, ids[rng.random(ids.size) > 0.03], int(classes[o]), float(rng.uniform(0.1, 1.0))))
        while len(mine) < want and idx.size:
            c = xyz[rng.choice(idx), :2]
            ids = idx[((xyz[idx, :2] - c) ** 2).sum(1) <= rng.uniform(0.2, 0.8) ** 2]
            mine.append((s, ids, int(rng.integers(4, 8)), float(rng.uniform(0.1, 1.0))))
        rows += mine
    return build(xyz, tile, halo, rows, kw=kw or dict(min_shared=5, iom=0.5))


def wall_case(n_zone=30000):
    """Two tiles; n_zone points of the scan's ~n_zone + 2000 lie in the shared region and in the one mask of either
    tile: every wave of the overlap launch adds to the same three counters."""
    xyz = np.concatenate([corners(0, 8), strip(n_zone, 3.5, 4.49, seed=6), strip(2000, 0, 8, seed=7)])
    every = np.arange(xyz.shape[0])
    return build(xyz, 4.0, 0.5, [(0, every, 5, 0.5), (1, every, 5, 0.25)], groups=[[0, 1]], n_zone=n_zone)


def chain_case(links=150, per=24):
    """Two tiles with `links` rows each, joined into ONE chain of 2 * links rows through the shared region: its points,
    sorted by y, are cut into runs of `per`; row i of tile 0 holds runs 2i and 2i + 1, row i of tile 1 runs 2i + 1 and
    2i + 2.  The picks are listed in reverse, so neighbours in the chain are far apart as rows."""
    n_zone = per * (2 * links + 1)
    xyz = np.concatenate([corners(0, 8), strip(n_zone, 3.5, 4.49, seed=8), strip(500, 0, 3.4, seed=9),
                          strip(500, 4.6, 8, seed=10)])
    zone = in_box(xyz, 3.5, 4.49)
    zone = zone[np.argsort(xyz[zone, 1], kind="stable")]
    run = lambda k: zone[k * per:(k + 1) * per]  # noqa: E731
    rows = [(0, np.concatenate([run(2 * i), run(2 * i + 1)]), 5, 0.1 + 0.005 * i) for i in range(links)]
    rows += [(1, np.concatenate([run(2 * i + 1), run(2 * i + 2)]), 5, 0.9 - 0.005 * i) for i in range(links)]
    return build(xyz, 4.0, 0.5, rows, kw=dict(min_shared=20, iom=0.3), groups=[list(range(2 * links))])


def brute_merge(plan, per_tile, iom=0.5, min_shared=20):
    """merge_tiles_host restated from set operations: every picked row scattered to a dense boolean [P, N] array over
    the scan, the tiles as boolean [T, N]; components by repeated closure of the adjacency matrix."""
    T, N = plan.T, plan.N
    in_tile = np.zeros((T, N), bool)
    for s in range(T):
        in_tile[s, plan.points(s)] = True
    dense, row_tile, cls, scores = [], [], [], []
    for s, (c, sc, masks, pick) in enumerate(per_tile):
        for r in np.asarray(pick).tolist():
            d = np.zeros(N, bool)
            d[plan.points(s)[np.asarray(masks)[r] != 0]] = True
            dense.append(d), row_tile.append(s), cls.append(int(c[r])), scores.append(np.float32(sc[r]))
    P = len(dense)
    dense = np.array(dense).reshape(P, N)
    adj = np.eye(P, dtype=bool)
    inter = np.zeros((P, P), np.int64)
    shared = np.zeros((P, T), np.int64)
    for a in range(P):
        for t in range(T):
            if t != row_tile[a]:
                shared[a, t] = (dense[a] & in_tile[t]).sum()
        for b in range(P):
            if row_tile[a] != row_tile[b]:
                inter[a, b] = (dense[a] & dense[b]).sum()  # (a mask of tile s holds only points of s)
    for a in range(P):
        for b in range(P):
            s, t = row_tile[a], row_tile[b]
            if s != t and cls[a] == cls[b] and inter[a, b] >= min_shared and \
                    float(inter[a, b]) >= iom * float(min(shared[a, t], shared[b, s])):
                adj[a, b] = True
    while True:
        nxt = (adj.astype(np.int64) @ adj.astype(np.int64)) > 0
        if (nxt == adj).all():
            break
        adj = nxt
    rep = adj.argmax(1) if P else np.zeros(0, np.int64)  # the first True of a row: the component's smallest row
    reps = sorted(set(rep.tolist()))
    members = np.array([reps.index(r) for r in rep.tolist()], np.int32)
    groups = [[r for r in range(P) if rep[r] == g] for g in reps]
    out_cls = np.array([cls[g[0]] for g in groups], np.int64)
    out_scores = np.array([max(scores[r] for r in g) for g in groups], np.float32)
    masks = np.array([dense[g].any(0) for g in groups]).reshape(len(groups), N).astype(np.int32)
    pick = np.argsort(-out_scores, kind="stable").astype(np.int64)
    return (out_cls, out_scores, masks, pick, members), dict(inter=inter.astype(np.int32), shared=shared.astype(np.int32),
                                                             groups=groups, count=masks.sum(1).astype(np.int32))
