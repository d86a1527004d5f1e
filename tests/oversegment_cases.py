"""Hand-made inputs of the over-segmentation rule (postprocess.oversegment_host stages B-D), shared by the host tests
and the GPU tests: every case is (xyz fp32 [n, 3], normals4 fp32 [n, 4], I int32 [n, k], deg int32 [n], keywords, the
ids the statement gives by its text)."""
import numpy as np

UP = (0.0, 0.0, 1.0, 0.0)  # a flat point with normal +z


def _rows(lists, k=None):
    """(I, deg) from per-point lists of row entries (ANY rows: the lists are taken as they are)."""
    k = k or max(len(r) for r in lists)
    I = np.full((len(lists), k), -1, np.int32)
    for i, r in enumerate(lists):
        I[i, :len(r)] = r
    return I, np.full(len(lists), k - 1, np.int32)


def _chain_rows(members):
    """Row lists that link the points `members` into a path: each lists itself and its successor."""
    return {a: [a, b] for a, b in zip(members[:-1], members[1:])} | {members[-1]: [members[-1]]}


def _case(xyz, normals4, lists, want, **kw):
    I, deg = _rows(lists)
    return (np.asarray(xyz, np.float32), np.asarray(normals4, np.float32), I, deg, kw, np.asarray(want, np.int32))


def lattices(offset):
    """Two parallel 5 x 5 lattices (2 cm) 1 cm apart, every normal +z, rows = all points within 3 cm: one segment when
    the offset bound admits the 1 cm step, two when it does not."""
    g = np.stack(np.meshgrid(np.arange(5) * 0.02, np.arange(5) * 0.02, indexing="ij"), -1).reshape(-1, 2)
    xyz = np.concatenate([np.c_[g, np.zeros(25)], np.c_[g, np.full(25, 0.01)]])
    d = np.linalg.norm(xyz[:, None] - xyz[None], axis=-1)
    lists = [list(np.argsort(d[i], kind="stable")[:int((d[i] <= 0.03).sum())]) for i in range(50)]
    want = np.zeros(50) if offset > 0.01 else np.repeat([0, 25], 25)
    return _case(xyz, [UP] * 50, lists, want, offset=offset, normal_deg=15.0, flatness=0.01, min_points=8)


def crease(angle_deg):
    """Two 5 x 5 lattices (2 cm) that meet along a line at `angle_deg`; rows = the lattice neighbours at distance
    <= 2 cm.  One segment below the 15 degree bound, two above."""
    th = np.radians(angle_deg)
    u, y = [a.reshape(-1) for a in np.meshgrid(np.arange(5) * 0.02, np.arange(5) * 0.02, indexing="ij")]
    a = np.c_[-0.02 - u, y, np.zeros(25)]
    b = np.c_[u * np.cos(th), y, u * np.sin(th)]
    xyz = np.concatenate([a, b])
    nb = (np.sin(th), 0.0, -np.cos(th), 0.0)  # the tilted plane's normal under the sign rule (first component positive)
    d = np.linalg.norm(xyz[:, None] - xyz[None], axis=-1)
    lists = [list(np.nonzero(d[i] <= 0.0201)[0]) for i in range(50)]
    want = np.zeros(50) if angle_deg < 15 else np.repeat([0, 25], 25)
    return _case(xyz, [UP] * 25 + [nb] * 25, lists, want, offset=0.012, normal_deg=15.0, flatness=0.01, min_points=8)


def bridge(sigma):
    """A path of 17 points on a line (1 cm steps); the middle one (index 8) carries `sigma`.  Flat, it joins the two
    halves into one segment; not flat, the halves are two segments of 8 and it is attached to the first qualifying
    entry of its row, which lists the RIGHT half first."""
    xyz = np.c_[np.arange(17) * 0.01, np.zeros(17), np.zeros(17)]
    n4 = np.tile(np.asarray(UP), (17, 1))
    n4[8, 3] = sigma
    rows = _chain_rows(list(range(17)))
    rows[8] = [8, 9, 7]
    flat = 0 <= sigma <= np.float32(0.01)
    want = np.zeros(17) if flat else np.r_[np.zeros(8), 9, np.full(8, 9)]
    return _case(xyz, n4, [rows[i] for i in range(17)], want, offset=0.012, normal_deg=15.0, flatness=0.01, min_points=8)


def attach(offset):
    """Segment A: points 0..7 on z = 0; segment B: points 8..15 on z = 5 mm; the non-flat point 16 at z = 4 mm lists a
    point of A before a point of B.  4.5 mm: both planes qualify and the FIRST entry (A, the farther plane) wins; 2 mm:
    only B qualifies; 0.5 mm: none."""
    xyz = np.concatenate([np.c_[np.arange(8) * 0.01, np.zeros(8), np.zeros(8)],
                          np.c_[np.arange(8) * 0.01, np.full(8, 1.0), np.full(8, 0.005)],
                          [[0.03, 0.5, 0.004]]])
    n4 = np.tile(np.asarray(UP), (17, 1))
    n4[16] = (1.0, 0.0, 0.0, 0.5)  # not flat; its own normal plays no part in the attach test
    rows = _chain_rows(list(range(8))) | _chain_rows(list(range(8, 16)))
    rows[16] = [16, 3, 11]
    last = 0 if offset >= 0.004 else 8 if offset >= 0.001 else -1
    want = np.r_[np.zeros(8), np.full(8, 8), last]
    return _case(xyz, n4, [rows[i] for i in range(17)], want, offset=offset, normal_deg=15.0, flatness=0.01, min_points=8)


def sizes(min_points):
    """A path of 8 points (indices 0..7) beside a path of 7 (8..14) and a non-flat point (15) that lists the short path
    first: min_points = 8 keeps the first and dissolves the second (its points and nothing attached to it), 7 keeps
    both."""
    xyz = np.c_[np.arange(16) * 0.01, np.zeros(16), np.zeros(16)]
    n4 = np.tile(np.asarray(UP), (16, 1))
    n4[15, 3] = -1.0
    rows = _chain_rows(list(range(8))) | _chain_rows(list(range(8, 15)))
    rows[15] = [15, 10, 2]
    want = np.r_[np.zeros(8), np.full(7, 8), 8] if min_points <= 7 else np.r_[np.zeros(8), np.full(7, -1), 0]
    return _case(xyz, n4, [rows[i] for i in range(16)], want, offset=0.012, normal_deg=15.0, flatness=0.01,
                 min_points=min_points)


RULE_CASES = {
    "lattices_offset_11mm": lambda: lattices(0.011), "lattices_offset_9mm": lambda: lattices(0.009),
    "crease_14deg": lambda: crease(14.0), "crease_16deg": lambda: crease(16.0),
    "sigma_below": lambda: bridge(0.0099), "sigma_above": lambda: bridge(0.0101),
    "attach_first": lambda: attach(0.0045), "attach_second": lambda: attach(0.002), "attach_none": lambda: attach(0.0005),
    "min_points_met": lambda: sizes(7), "min_points_missed": lambda: sizes(8),
}
