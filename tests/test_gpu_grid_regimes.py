"""The hash grid of csrc/geodesic.hip (count -> scan -> fill) and the two kernels that walk it, k_knn_radius and
k_ball_query_grid, bit for bit against brute force in every regime: the smallest table and its hash collisions, partial
workgroups, padded rows for every k, the rank cut and its ties, neighbours at exactly the radius, negative and translated
coordinates, the candidate lists' capacity on both sides of its boundary (the kNN kernel's error flag, the ball query's
linear scan), a table whose scan loops with a carry, and a grid built ahead on another stream and handed over.
Points and cases: tests/grid_cases.py (tests/test_grid_cases_host.py proves that the cases reach the regimes).
No tolerance anywhere: the kNN reference is oracle.knn followed by the sqrt(D) <= float32(radius) filter, the ball-query
reference is oracle.ball_query."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import grid_cases as gc

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()  # (a copy: the shared cases are read-only)


def _assert_plan(hip, n, T, blocks=None):
    out = [ctypes.c_int(-1) for _ in range(4)]
    assert hip.gf_dev_point_grid_plan(n, *[ctypes.byref(o) for o in out]) == 0
    assert out[0].value == T == gc.table_size(n) and (out[2].value, out[3].value) == (gc.KNN_CAP, gc.BQG_CAP)
    assert blocks is None or out[1].value == blocks


@functools.lru_cache(maxsize=None)
def _points(kind, n):
    p = gc.points(kind, n)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def _cluster(size):
    xyz, label, centres = gc.cluster_case(size)
    for a in (xyz, label, centres):
        a.setflags(write=False)
    return xyz, label, centres


def _ref_rows(oracle, xyz, k, radius, rows=None):
    """(d2, I, in-radius mask) of the brute force, [rows, k]."""
    D2, I = oracle.knn(xyz, xyz if rows is None else xyz[rows], k)
    return D2, I, np.sqrt(D2) <= np.float32(radius)


def _knn(xyz, k, radius, sqrt_out, **kw):
    from geoformer_amd import pointops

    kw.setdefault("check_overflow", True)
    return tuple(t.cpu().numpy() for t in pointops.knn_radius(_dev(xyz), k, radius, sqrt_out=sqrt_out, **kw))


def _assert_rows(got, ref, sqrt_out, rows=None, what=""):
    gd, gi, deg = (g if rows is None else g[rows] for g in got[:3])
    D2, I, inr = ref
    bad = np.flatnonzero((np.where(inr, I, -1) != gi).any(1))
    assert not len(bad), f"{what}: {len(bad)} index rows differ, first {bad[0]}: {gi[bad[0]]} != {np.where(inr, I, -1)[bad[0]]}"
    D = np.sqrt(D2) if sqrt_out else D2
    assert (np.where(inr, D, np.inf) == gd).all(), what  # (bitwise for finite values and for inf)
    assert (deg == inr.sum(1) - 1).all(), what  # min(nin, k) - 1


def _check_knn(oracle, xyz, radius, ks=gc.KNN_K, sqrt_outs=(True, False), what=""):
    for k in ks:
        ref = _ref_rows(oracle, xyz, k, radius)
        for sqrt_out in sqrt_outs:
            _assert_rows(_knn(xyz, k, radius, sqrt_out), ref, sqrt_out, what=f"{what} k={k} sqrt_out={sqrt_out}")
    return ref


# ---- kNN -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", gc.SMALL_N)
@pytest.mark.parametrize("kind", gc.SMALL_KINDS)
def test_knn_small_tables(hip, oracle, kind, n):
    """T = 1024 (and its first step at n = 257): collisions, partial last workgroups, the padding loop for every k."""
    _assert_plan(hip, n, 2048 if n > 256 else 1024, 2 if n > 256 else 1)
    _check_knn(oracle, _points(kind, n), gc.RADIUS, what=f"{kind} n={n}")


@pytest.mark.parametrize("size", gc.CLUSTER_SIZES)
def test_knn_rank_cut_in_clusters(hip, oracle, size):
    """Rows of k < nin <= 1024 candidates; size 1024 fills the list exactly: no flag (check_overflow would raise)."""
    xyz, label, _ = _cluster(size)
    ref = _check_knn(oracle, xyz, gc.RADIUS, ks=gc.CLUSTER_K, what=f"cluster of {size}")
    full = ref[2].all(1)  # (k = 64)
    assert (full == (label == 0)).all() and full.sum() == size
    flag = _knn(xyz, 64, gc.RADIUS, True, check_overflow=False, return_flag=True)[3]
    assert flag.tolist() == [0]


def test_knn_lattice_ties_and_exact_radius(hip, oracle):
    """Six neighbours at exactly the radius (kept: sqrt(d2) <= radius), all at one distance: k = 4 cuts through them by
    index, k = 7 fits exactly, k = 64 pads."""
    xyz = _points("lattice", 729)
    _assert_plan(hip, 729, 4096)
    ref = _check_knn(oracle, xyz, gc.LATTICE_STEP, ks=gc.LATTICE_K, what="lattice")
    D2, I, inr = ref  # k = 64
    interior = np.flatnonzero(inr.sum(1) == 7)
    assert len(interior) == 343
    assert (D2[interior, 1:7] == np.float32(gc.LATTICE_STEP) ** 2).all() and (D2[interior, 0] == 0).all()
    assert (np.diff(I[interior, 1:7], axis=1) > 0).all()  # equal distances: ascending index
    gd, gi, deg = _knn(xyz, 64, gc.LATTICE_STEP, True)
    assert (gd[interior, 1:7] == np.float32(gc.LATTICE_STEP)).all() and (deg[interior] == 6).all()


def test_knn_exact_copies(hip, oracle):
    n, count = gc.COPIES
    xyz, where = gc.copies(n, count)
    ref = _check_knn(oracle, xyz, gc.RADIUS, ks=(4, 64), what="copies")
    assert (ref[1][where, :64] == where[:64]).all() and (ref[0][where] == 0).all()  # the 64 lowest copies, every row


@pytest.mark.parametrize("kind", ["translated", "signed"])
def test_knn_translated_and_negative_coordinates(hip, oracle, kind):
    xyz = _points(kind, gc.SHIFT_N)
    _assert_plan(hip, gc.SHIFT_N, 32768)
    _check_knn(oracle, xyz, gc.RADIUS, ks=(16, 64), what=kind)


@functools.lru_cache(maxsize=None)
def _overflow_run():
    """One run of the 1025-point clump (flag 1) followed by a run of the same n without it, on the same stream: the
    allocator hands the second call the first one's scratch block, so its flag is clear only if the call clears it."""
    from geoformer_amd import pointops

    xyz, label, _ = _cluster(gc.OVERFLOW_SIZE)
    calm = _cluster(gc.CLUSTER_SIZES[0])[0]
    x, c = _dev(xyz), _dev(calm)
    torch.cuda.synchronize()
    D, I, deg, flag = pointops.knn_radius(x, 64, gc.RADIUS, sqrt_out=False, return_flag=True)
    first = tuple(t.cpu().numpy() for t in (D, I, deg, flag))
    at = flag.data_ptr()
    del D, I, deg, flag
    D, I, deg, flag = pointops.knn_radius(c, 64, gc.RADIUS, sqrt_out=False, return_flag=True)
    second = tuple(t.cpu().numpy() for t in (D, I, deg, flag))
    return first, second, at == flag.data_ptr()


def test_knn_capacity_overflow_sets_the_flag(hip, oracle):
    from geoformer_amd import _lib, pointops

    xyz, label, _ = _cluster(gc.OVERFLOW_SIZE)
    (gd, gi, deg, flag), _, _ = _overflow_run()
    assert flag.tolist() == [1]
    with pytest.raises(_lib.GeoFormerHipError, match="more in-radius neighbours"):
        pointops.knn_radius(_dev(xyz), 64, gc.RADIUS, check_overflow=True)
    # rows of the points with nin <= 1024: exact
    calm = np.flatnonzero(label != 0)
    _assert_rows((gd, gi, deg), _ref_rows(oracle, xyz, 64, gc.RADIUS, calm), False, calm, "rows beside the overflow")
    # rows of the overflowing points: k of their true in-radius neighbours, unique, ascending by (d2, index)
    over = np.flatnonzero(label == 0)
    D2, I, inr = _ref_rows(oracle, xyz, gc.OVERFLOW_SIZE + 1, gc.RADIUS, over)
    assert (inr.sum(1) == gc.OVERFLOW_SIZE).all()
    assert (deg[over] == 63).all() and (gi[over] >= 0).all()
    for j, i in enumerate(over):
        at = {int(v): p for p, v in enumerate(I[j, :gc.OVERFLOW_SIZE])}  # position in the full (d2, index) order
        pos = np.array([at.get(int(v), -1) for v in gi[i]])
        assert (pos >= 0).all(), f"row {i}: an entry is no in-radius neighbour"
        assert (np.diff(pos) > 0).all(), f"row {i}: not unique and ascending by (d2, index)"
        assert (gd[i] == D2[j, pos]).all(), f"row {i}: distances"


def test_knn_flag_is_clear_on_the_next_call(hip, oracle):
    first, (gd, gi, deg, flag), same_block = _overflow_run()
    assert first[3].tolist() == [1] and flag.tolist() == [0]
    assert same_block  # (the same flag word: it is the call's own memset that cleared it)
    calm = _cluster(gc.CLUSTER_SIZES[0])[0]
    _assert_rows((gd, gi, deg), _ref_rows(oracle, calm, 64, gc.RADIUS), False, what="the call after the overflow")


def test_knn_large_table_scan_with_carry(hip, oracle):
    """512 scan workgroups: the top level of the scan takes two passes.  4096 random rows and the rows at both ends of
    every 1024 against brute force over all points."""
    n = gc.LARGE_N
    _assert_plan(hip, n, 1 << 19, 512)
    xyz = _points("room", n)
    i = np.arange(n)
    rows = np.union1d(np.random.default_rng(11).permutation(n)[:gc.LARGE_ROWS], i[(i % 1024 == 0) | (i % 1024 == 1023)])
    assert len(rows) >= gc.LARGE_ROWS
    ref = _ref_rows(oracle, xyz, 64, gc.RADIUS, rows)
    assert ref[2].sum(1).max() > 16 and not ref[2].all(1).any()
    for sqrt_out in (True, False):
        _assert_rows(_knn(xyz, 64, gc.RADIUS, sqrt_out), ref, sqrt_out, rows, f"large sqrt_out={sqrt_out}")


# ---- ball query ----------------------------------------------------------------------------------------------------
def _ball(centres, xyz, radius, nsample, grid):
    from geoformer_amd import pointops

    return pointops.ball_query(_dev(centres[None]), _dev(xyz[None]), radius, nsample, grid=grid)[0].cpu().numpy()


def _assert_ball(got, ref, what):
    bad = np.flatnonzero((got != ref).any(1))
    assert not len(bad), f"{what}: {len(bad)} rows differ, first {bad[0]}: {got[bad[0]]} != {ref[bad[0]]}"


@pytest.mark.parametrize("n", gc.BALL_N)
@pytest.mark.parametrize("kind", gc.BALL_KINDS)
def test_ball_query_grid(hip, oracle, kind, n):
    """Centres on and off the point set and one far away (a row of zeros), m that leave a partial workgroup, rows cut at
    nsample and padded; on the lattice the points at exactly the radius are no hits.  Oracle == grid == brute force."""
    xyz = _points(kind, n)
    radius = gc.radius_of(kind, ball=True)
    _assert_plan(hip, n, gc.table_size(n))
    for m in gc.BALL_M:
        centres = gc.ball_centres(xyz, m)
        for nsample in gc.BALL_NSAMPLE:
            ref = oracle.ball_query(centres[None], xyz[None], radius, nsample)[0]
            what = f"{kind} n={n} m={m} nsample={nsample}"
            _assert_ball(_ball(centres, xyz, radius, nsample, True), ref, what + " grid")
            _assert_ball(_ball(centres, xyz, radius, nsample, False), ref, what + " scan")
            if m >= 3:
                assert (ref[1] == 0).all()  # the far centre
    if kind == "lattice" and n >= 900:
        on = xyz[:64]  # points of the set as centres: the six points at exactly the radius are not in the ball
        ref = oracle.ball_query(on[None], xyz[None], radius, 16)[0]
        assert (ref == np.arange(64)[:, None]).all()
        _assert_ball(_ball(on, xyz, radius, 16, True), ref, "lattice points as centres")


@pytest.mark.parametrize("size", [gc.BQG_CAP, gc.BQG_CAP + 1])
def test_ball_query_capacity(hip, oracle, size):
    """A centre with exactly 1024 hits (the list is full) and with 1025 (the linear scan inside the kernel)."""
    xyz, label, cl_centres = _cluster(size)
    member = np.flatnonzero(label == 0)
    centres = np.stack([cl_centres[0], xyz[member[0]], xyz[np.flatnonzero(label == -1)[0]], cl_centres[1],
                        xyz[member[-1]]]).astype(np.float32)
    for nsample in gc.BALL_CAP_NSAMPLE + (2000,):
        ref = oracle.ball_query(centres[None], xyz[None], gc.RADIUS, nsample)[0]
        if nsample == 2000:
            assert [len(np.unique(r)) for r in ref] == [size, size, 1, 40, size]
        else:
            assert (ref[0] == member[:nsample]).all()  # the first hits in index order
        _assert_ball(_ball(centres, xyz, gc.RADIUS, nsample, True), ref, f"cluster of {size} nsample={nsample} grid")
        _assert_ball(_ball(centres, xyz, gc.RADIUS, nsample, False), ref, f"cluster of {size} nsample={nsample} scan")


# ---- the grid handed over ------------------------------------------------------------------------------------------
def _sa_module(C):
    from geoformer_amd.model.set_abstraction import PointnetSAModuleVotesSeparate

    torch.manual_seed(gc.SA_N)
    sa = PointnetSAModuleVotesSeparate(radius=gc.SA_RADIUS, nsample=gc.SA_NSAMPLE, npoint=gc.SA_PICKS, mlp=[C, 32, 32, 48],
                                       normalize_xyz=True)
    for m in sa.modules():
        if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
            m.running_mean.normal_(); m.running_var.uniform_(0.5, 2); m.weight.data.normal_(1, 0.2); m.bias.data.normal_()
    return sa.eval().cuda()


def test_grid_built_on_a_side_stream_and_handed_over(hip, oracle):
    """point_grid_build on another stream, ordered by events the way the eval forward does it, then sa_group_mlp_max
    with that grid (grid_ready = 1) and with a grid of its own: the same groups, and the oracle's."""
    from geoformer_amd import pointops

    n, C = gc.SA_N, 16
    xyz_h = _points("room", n)
    g = torch.Generator().manual_seed(n)
    inds_h = torch.randperm(n, generator=g)[:gc.SA_PICKS].int()
    feats = torch.randn(1, C, n, generator=g).cuda()
    ref = oracle.ball_query(xyz_h[inds_h.numpy()][None], xyz_h[None], gc.SA_RADIUS, gc.SA_NSAMPLE)
    assert len(np.unique(ref)) > gc.SA_PICKS * 4 and (np.diff(ref, axis=2) != 0).any(2).all()  # real groups
    sa = _sa_module(C)
    with torch.no_grad():
        chain = sa._fused_chain()
        main, aux = torch.cuda.current_stream(), torch.cuda.Stream()
        xyz, inds = _dev(xyz_h[None]), inds_h[None].cuda()
        xyz_ready = torch.cuda.Event()
        xyz_ready.record(main)
        aux.wait_event(xyz_ready)
        with torch.cuda.stream(aux):
            xyz.record_stream(aux)
            grid = pointops.point_grid_build(xyz, gc.SA_RADIUS)
            grid.record_stream(main)
            grid_done = torch.cuda.Event()
            grid_done.record(aux)
        main.wait_event(grid_done)
        handed = pointops.sa_group_mlp_max(xyz, feats, inds, gc.SA_RADIUS, gc.SA_NSAMPLE, True, True, chain, grid=grid)
        own = pointops.sa_group_mlp_max(xyz, feats, inds, gc.SA_RADIUS, gc.SA_NSAMPLE, True, True, chain, grid=None)
    for name, a, b in zip(("new_xyz", "idx", "pooled"), handed, own):
        assert torch.equal(a, b), name
    assert (handed[1].cpu().numpy() == ref).all() and (own[1].cpu().numpy() == ref).all()
    assert (handed[0].cpu().numpy()[0] == xyz_h[inds_h.numpy()]).all()
    assert torch.isfinite(handed[2]).all() and handed[2].abs().max().item() > 0


def test_sa_stage_below_the_grid_threshold(hip, oracle):
    """n = 900 < 4096: the set-abstraction call takes the scan kernel; the same groups as the oracle's (and as the grid
    kernel's, asked for directly)."""
    from geoformer_amd import pointops

    n, C = gc.SA_SMALL_N, 16
    xyz_h = _points("translated", n)
    g = torch.Generator().manual_seed(n)
    inds_h = torch.randperm(n, generator=g)[:gc.SA_PICKS].int()
    feats = torch.randn(1, C, n, generator=g).cuda()
    centres = xyz_h[inds_h.numpy()]
    ref = oracle.ball_query(centres[None], xyz_h[None], gc.SA_RADIUS, gc.SA_NSAMPLE)
    sa = _sa_module(C)
    with torch.no_grad():
        new_xyz, idx, pooled = pointops.sa_group_mlp_max(_dev(xyz_h[None]), feats, inds_h[None].cuda(), gc.SA_RADIUS,
                                                         gc.SA_NSAMPLE, True, True, sa._fused_chain(), grid=None)
    assert (idx.cpu().numpy() == ref).all() and (new_xyz.cpu().numpy()[0] == centres).all()
    _assert_ball(_ball(centres, xyz_h, gc.SA_RADIUS, gc.SA_NSAMPLE, True), ref[0], "grid kernel at n = 900")
    assert torch.isfinite(pooled).all()
