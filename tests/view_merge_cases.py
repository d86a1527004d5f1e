"""Builders and cases for the join of instances across the views of a scan (postprocess.merge_views_host and
csrc/view_merge.hip): hand cases with the expected ids, scores and masks written out, random cases built by perturbing
shared ground-truth sets, and the launch regimes of the kernels at the smallest shapes where they can go wrong."""
import numpy as np

F = np.float32


def view(N, rows, pick=None):
    """One view's (cls, scores, masks, pick) from rows of (points, class, score); pick: the picked rows (default all, in
    order).  No rows: a view without proposals."""
    if not rows:
        return ([], [], [], np.zeros(0, np.int64))
    masks = np.zeros((len(rows), N), np.int32)
    for r, (pts, _, _) in enumerate(rows):
        masks[r, np.asarray(list(pts), np.int64)] = 1
    return (np.asarray([c for _, c, _ in rows], np.int64), np.asarray([s for _, _, s in rows], F), masks,
            np.arange(len(rows), dtype=np.int64) if pick is None else np.asarray(pick, np.int64))


def case(N, views, expect=None, **kw):
    return dict(N=N, per_view=[v if isinstance(v, tuple) else view(N, v) for v in views], kw=kw, expect=expect)


def mean32(*ms):
    """The statement's score of the per-view maxima ms, in float32 arithmetic written out."""
    acc = F(ms[0])
    for m in ms[1:]:
        acc = F(acc + F(m))
    return F(acc / F(len(ms)))


R = lambda a, b: set(range(a, b))  # noqa: E731


def hand_cases():
    """name -> case; expect: members (row -> global id, -1 dropped), cls, scores, masks (point sets) of the instances."""
    out = {}
    # a chain through view 0, which holds two rows: a1 - b - c - a2 is one component of support 3
    out["chain_through_one_view"] = case(
        10, [[(R(0, 4), 3, 0.9), (R(6, 10), 3, 0.5)], [(R(0, 6), 3, 0.8)], [(R(2, 10), 3, 0.7)]],
        dict(members=[0, 0, 0, 0], cls=[3], scores=[mean32(0.9, 0.8, 0.7)], masks=[R(0, 10)], support=[3]), iou=0.4)
    two = [[({0}, 1, 0.5)], [({0, 1}, 1, 0.25)]]
    out["iou_exactly_at_the_threshold"] = case(
        2, two, dict(members=[0, 0], cls=[1], scores=[mean32(0.5, 0.25)], masks=[{0, 1}], support=[2]), iou=0.5)
    out["iou_just_under_the_threshold"] = case(
        2, two, dict(members=[0, 1], cls=[1, 1], scores=[mean32(0.5, 0.0), mean32(0.0, 0.25)], masks=[{0}, {0, 1}],
                     support=[1, 1]), iou=0.5000001)
    out["support_2_the_mask_is_the_union"] = case(
        8, [[(R(0, 5), 2, 0.6)], [(R(1, 7), 2, 0.9)]],
        dict(members=[0, 0], cls=[2], scores=[mean32(0.6, 0.9)], masks=[R(0, 7)], support=[2]))
    # two candidates of IoU 2/4 each: the smaller row wins, the other stays alone
    out["iou_tie_the_smaller_row_wins"] = case(
        4, [[(R(0, 4), 1, 0.9)], [(R(0, 2), 1, 0.8), (R(2, 4), 1, 0.7)]],
        dict(members=[0, 0, 1], cls=[1, 1], scores=[mean32(0.9, 0.8), mean32(0.0, 0.7)], masks=[R(0, 4), R(2, 4)],
             support=[2, 1]), min_views=1)
    # 2/4 (row 1) and 1/2 (row 2) are the same IoU: the smaller row wins
    out["equal_iou_as_different_fractions"] = case(
        7, [[({0, 1}, 1, 0.9)], [({0, 1, 5, 6}, 1, 0.8), ({0}, 1, 0.7)]],
        dict(members=[0, 0, 1], cls=[1, 1], scores=[mean32(0.9, 0.8), mean32(0.0, 0.7)], masks=[{0, 1, 5, 6}, {0}],
             support=[2, 1]), min_views=1)
    out["equal_iou_as_different_fractions_swapped"] = case(
        7, [[({0, 1}, 1, 0.9)], [({0}, 1, 0.7), ({0, 1, 5, 6}, 1, 0.8)]],
        dict(members=[0, 0, 1], cls=[1, 1], scores=[mean32(0.9, 0.7), mean32(0.0, 0.8)], masks=[{0, 1}, {0, 1, 5, 6}],
             support=[2, 1]), min_views=1)
    out["class_mismatch_with_iou_1"] = case(
        3, [[(R(0, 3), 3, 0.9)], [(R(0, 3), 4, 0.8)]],
        dict(members=[0, 1], cls=[3, 4], scores=[mean32(0.9, 0.0), mean32(0.0, 0.8)], masks=[R(0, 3), R(0, 3)],
             support=[1, 1]))
    # A one-sided best: a (row 0) prefers b (row 2) with IoU 1/9 >= 0.1, but b prefers c (row 1), so a joins nothing.
    # "Nothing joins at all" cannot be built with every pair over the threshold: between two views the same-class pair
    # of the largest IoU is always mutual (each of the two is the other's best), so wherever a one-sided preference
    # exists, the preferred row has a mutual partner of a larger IoU, which passes any threshold the one-sided pair
    # passes.  Hence two cases: a left alone while b joins c, and a threshold above every IoU, at which nothing joins.
    one_sided = [[(R(0, 4), 1, 0.9), (R(4, 9), 1, 0.8)], [(R(3, 9), 1, 0.7)]]
    out["one_sided_best"] = case(
        9, one_sided, dict(members=[0, 1, 1], cls=[1, 1], scores=[mean32(0.9, 0.0), mean32(0.8, 0.7)],
                           masks=[R(0, 4), R(3, 9)], support=[1, 2]), iou=0.1, min_views=1)
    out["one_sided_best_nothing_joins"] = case(
        9, one_sided, dict(members=[0, 1, 2], cls=[1, 1, 1], scores=[mean32(0.9, 0.0), mean32(0.8, 0.0), mean32(0.0, 0.7)],
                           masks=[R(0, 4), R(4, 9), R(3, 9)], support=[1, 1, 1]), iou=0.9, min_views=1)
    # V = 3, min_views = 2: X (points 0..3) is seen by one view and dropped, Y (10..15) by two and kept
    out["support_below_and_at_min_views"] = case(
        16, [[(R(0, 4), 1, 0.9), (R(10, 16), 1, 0.8)], [(R(10, 15), 1, 0.6)], []],
        dict(members=[-1, 0, 0], cls=[1], scores=[mean32(0.8, 0.6, 0.0)], masks=[R(10, 16)], support=[2]), min_views=2)
    out["support_below_and_at_min_views_3_of_4"] = case(
        16, [[(R(0, 4), 1, 0.9), (R(10, 16), 1, 0.8)], [(R(0, 4), 1, 0.5), (R(10, 15), 1, 0.6)], [(R(10, 16), 1, 0.4)], []],
        dict(members=[-1, 0, -1, 0, 0], cls=[1], scores=[mean32(0.8, 0.6, 0.4, 0.0)], masks=[R(10, 16)], support=[3]),
        min_views=3)
    # votes exactly at vote * support: point 10 has support - 1 votes, 11 one fewer, ...
    nested = lambda V: [[(R(0, 10) | R(10, 10 + V - 1 - v), 1, 0.5)] for v in range(V)]  # noqa: E731
    for V, vote, top in ((2, 0.5, 11), (2, 1.0, 10), (3, 1.0, 10), (4, 0.5, 12), (4, 0.75, 11), (4, 1.0, 10)):
        out[f"votes_at_the_threshold_support_{V}_vote_{vote}"] = case(
            14, nested(V), dict(members=[0] * V, cls=[1], scores=[mean32(*[0.5] * V)], masks=[R(0, top)], support=[V]),
            vote=vote, min_views=V)
    out["an_empty_row"] = case(
        6, [[(set(), 1, 0.9), (R(0, 3), 1, 0.8)], [(R(0, 3), 1, 0.7), (set(), 1, 0.95)]],
        dict(members=[-1, 0, 0, -1], cls=[1], scores=[mean32(0.8, 0.7)], masks=[R(0, 3)], support=[2]), min_views=1)
    out["a_view_with_no_picks"] = case(
        6, [[(R(0, 3), 1, 0.8)], [], [(R(0, 3), 1, 0.7)]],
        dict(members=[0, 0], cls=[1], scores=[mean32(0.8, 0.0, 0.7)], masks=[R(0, 3)], support=[2]))
    out["masks_and_no_picks"] = case(
        6, [[(R(0, 3), 1, 0.8)], view(6, [(R(0, 3), 1, 0.7)], pick=[])],
        dict(members=[0], cls=[1], scores=[mean32(0.8, 0.0)], masks=[R(0, 3)], support=[1]))
    out["all_views_empty"] = case(5, [[], [], []], dict(members=[], cls=[], scores=[], masks=[], support=[]))
    # picks 7 and -1 name no row of the masks: empty rows; row 0 is picked twice: the second copy finds its partner taken
    out["pick_out_of_range_and_listed_twice"] = case(
        6, [view(6, [(R(0, 4), 2, 0.8), (R(4, 6), 2, 0.3)], pick=[0, 7, 0, -1]), [(R(0, 4), 2, 0.6)]],
        dict(members=[0, -1, 1, -1, 0], cls=[2, 2], scores=[mean32(0.8, 0.6), mean32(0.8, 0.0)], masks=[R(0, 4), R(0, 4)],
             support=[2, 1]), min_views=1)
    # the sum of the views' maxima over V = 3 and 5 is not exact in float32
    out["score_sum_v3"] = case(
        4, [[(R(0, 4), 1, 0.7), (R(0, 3), 1, 0.1)], [(R(0, 4), 1, 0.2)], [(R(0, 4), 1, 0.9)]],
        dict(members=[0, 1, 0, 0], cls=[1, 1], scores=[F(F(F(F(0.7) + F(0.2)) + F(0.9)) / F(3)), F(F(F(F(0.1) + F(0)) + F(0)) / F(3))],
             masks=[R(0, 4), R(0, 3)], support=[3, 1]), min_views=1)
    s5 = [0.1, 0.7, 0.3, 0.9, 0.6]
    out["score_sum_v5"] = case(
        4, [[(R(0, 4), 1, s)] for s in s5],
        dict(members=[0] * 5, cls=[1], scores=[F(F(F(F(F(F(0.1) + F(0.7)) + F(0.3)) + F(0.9)) + F(0.6)) / F(5))],
             masks=[R(0, 4)], support=[5]))
    # two member rows of one view count once per point (the chain's view 0 above), and the larger of their scores counts
    out["one_view_alone"] = case(
        5, [[(R(0, 2), 1, 0.3), (set(), 1, 0.9), (R(1, 5), 2, 0.6)]],
        dict(members=[0, -1, 1], cls=[1, 2], scores=[F(0.3), F(0.6)], masks=[R(0, 2), R(1, 5)], support=[1, 1]))
    return out


def random_case(seed, N=None, V=None, picks=None, n_objects=None, classes=3):
    """Rows built by perturbing shared ground-truth sets: per view every object is seen with probability 0.8 as its set
    with some points dropped and some added; now and then a row is duplicated (an exact IoU tie), split in two halves or
    replaced by noise.  picks: the number of picked rows per view (rows are repeated or cut to reach it)."""
    rng = np.random.default_rng(seed)
    N = int(rng.integers(1, 201)) if N is None else N
    V = int(rng.integers(1, 7)) if V is None else V
    K = int(rng.integers(1, 7)) if n_objects is None else n_objects
    objs = []
    for _ in range(K):
        size = int(rng.integers(1, max(2, N // 3 + 1)))
        start = int(rng.integers(0, max(1, N - size + 1)))
        objs.append((np.arange(start, min(N, start + size)), int(rng.integers(1, classes + 1))))
    views = []
    for v in range(V):
        rows = []
        for pts, c in objs:
            if rng.random() > 0.8:
                continue
            keep = pts[rng.random(pts.size) > rng.choice([0.0, 0.1, 0.4])]
            extra = rng.integers(0, N, int(rng.integers(0, 3)))
            s = set(keep.tolist()) | set(extra.tolist()) if rng.random() < 0.7 else set(keep.tolist())
            score = float(F(rng.uniform(0.05, 1.0)))
            u = rng.random()
            if u < 0.12:
                rows += [(s, c, score), (s, c, float(F(rng.uniform(0.05, 1.0))))]  # a duplicate: an exact tie
            elif u < 0.22 and len(s) > 1:
                half = sorted(s)
                rows += [(set(half[:len(half) // 2]), c, score), (set(half[len(half) // 2:]), c, score)]
            elif u < 0.27:
                rows.append((set(rng.integers(0, N, 3).tolist()), int(rng.integers(1, classes + 1)), score))
            else:
                rows.append((s, c, score))
        order = rng.permutation(len(rows)).tolist()
        rows = [rows[i] for i in order]
        pick = None
        if picks is not None:
            p = picks[v] if not isinstance(picks, int) else picks
            if p and not rows:
                rows = [(set(objs[0][0].tolist()), objs[0][1], 0.5)]
            pick = [i % len(rows) for i in range(p)] if rows else []
        elif rows and rng.random() < 0.3:
            pick = rng.permutation(len(rows))[:int(rng.integers(0, len(rows) + 1))].tolist()
        views.append(view(N, rows, pick) if rows else view(N, []))
    kw = dict(iou=float(rng.choice([0.25, 0.5, 0.75])), vote=float(rng.choice([0.5, 0.75, 1.0])))
    if rng.random() < 0.6:
        kw["min_views"] = int(rng.integers(1, V + 1))
    return dict(N=N, per_view=views, kw=kw, expect=None)


def random_cases(n=48):
    return [random_case(1000 + i) for i in range(n)]


def chain_case(links=60, length=10, shift=3):
    """`links` rows in one chain over three views: row k lies in view k % 3 and holds [shift * k, shift * k + length);
    its best partner in each of the other two views is its neighbour in the chain (IoU 7 / 13), so the union-find hooks
    links - 1 edges."""
    N = shift * (links - 1) + length
    views = [[], [], []]
    for k in range(links):
        views[k % 3].append((R(shift * k, shift * k + length), 1, float(F(0.3 + 0.01 * k))))
    return case(N, views, iou=0.5)


def all_views_case(V=32, N=70):
    """One instance whose members span all V views: view v sees points 0 .. N-1 but point v."""
    return case(N, [[(R(0, N) - {v}, 1, float(F(0.5 + 0.01 * v)))] for v in range(V)], min_views=V, vote=1.0)


def wall_case(N=20000):
    """One instance that holds every point in both views: every wave of the pack and assemble launches counts into it."""
    return case(N, [[(R(0, N), 1, 0.5)], [(R(0, N), 1, 0.75)]])


def synthetic_rows(seed, N, V, picks, n_objects=60):
    """V views x picks rows over N points for the measurements: objects are intervals of the points, every view sees a
    random choice of them with jittered ends."""
    rng = np.random.default_rng(seed)
    size = N // n_objects
    views = []
    for v in range(V):
        masks = np.zeros((picks, N), np.int32)
        ids = rng.permutation(n_objects)[:picks] if picks <= n_objects else rng.integers(0, n_objects, picks)
        for r, o in enumerate(ids):
            a = max(0, int(o * size + rng.integers(-size // 10, size // 10 + 1)))
            b = min(N, int((o + 1) * size + rng.integers(-size // 10, size // 10 + 1)))
            masks[r, a:b] = 1
        views.append(((ids % 5 + 1).astype(np.int64), rng.uniform(0.1, 1.0, picks).astype(F), masks,
                      np.arange(picks, dtype=np.int64)))
    return dict(N=N, per_view=views, kw={}, expect=None)
