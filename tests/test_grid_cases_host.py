"""The hash grid's sizes (gf_dev_point_grid_plan, csrc/geodesic.hip) against the numpy restatement of tests/grid_cases.py,
and the coverage the GPU tests of tests/test_gpu_grid_regimes.py rest on: every case list reaches the regime it is named
for -- hash collisions, the rank cut, padded rows, neighbours at exactly the radius, the candidate lists' capacity on both
sides of its boundary, a scan with a carry.  A change of the table rule, the hash or a capacity that moves a case into
another regime fails here.  No GPU: the plan launches nothing, the facts are counted on the CPU."""
import ctypes
import functools

import numpy as np
import pytest

from tests import grid_cases as gc
from tests.test_host_logic import lib  # noqa: F401  (the library, built for gfx950 if missing)

OK, INVALID = 0, -1


def _lib_plan(lib, n):
    out = [ctypes.c_int(-7) for _ in range(4)]
    st = lib.gf_dev_point_grid_plan(int(n), *[ctypes.byref(o) for o in out])
    return st, tuple(o.value for o in out)  # table_size, scan_blocks, knn_cap, bq_cap


def _plan_sizes():
    edges = [v for j in range(1, 23) for v in ((1 << j) - 1, 1 << j, (1 << j) + 1)]
    return sorted(set(range(1, 5001)) | {v for v in edges if 1 <= v <= (1 << 22)})


def test_plan_equals_the_restatement(lib):
    ns = _plan_sizes()
    assert ns[0] == 1 and ns[-1] == 1 << 22 and (1 << 22) - 1 in ns and 65537 in ns
    seen = set()
    for n in ns:
        st, got = _lib_plan(lib, n)
        T = gc.table_size(n)
        assert st == OK, (n, lib.gf_last_error())
        assert got == (T, gc.scan_blocks(T), gc.KNN_CAP, gc.BQG_CAP), n
        seen.add(T)
    assert seen == {1 << j for j in range(10, 25)}  # every step from the smallest table to that of 2^22 points
    assert gc.KNN_CAP == gc.BQG_CAP == 1024


def test_table_rule():
    for n in _plan_sizes():
        T = gc.table_size(n)
        assert T & (T - 1) == 0 and T >= gc.T_MIN and T >= 4 * n and (T == gc.T_MIN or T // 2 < 4 * n)
        assert (gc.scan_blocks(T) - 1) * gc.SCAN_ITEMS < T <= gc.scan_blocks(T) * gc.SCAN_ITEMS
    assert gc.table_size(256) == 1024 and gc.table_size(257) == 2048  # the first step
    assert gc.table_size(1 << 24) == gc.table_size(1 << 30) == gc.T_MAX == 1 << 26  # the cap
    # the scan's top level loops (with a carry) from n = 65 537 on
    assert gc.scan_blocks(gc.table_size(65536)) == gc.SCAN_TOP and gc.scan_blocks(gc.table_size(65537)) == 2 * gc.SCAN_TOP


def test_plan_refuses_bad_arguments(lib):
    for n in (0, -5):
        st, got = _lib_plan(lib, n)
        assert st == INVALID and got == (-7,) * 4 and b"gf_dev_point_grid_plan" in lib.gf_last_error()
    one = ctypes.c_int(-7)
    assert lib.gf_dev_point_grid_plan(100, ctypes.byref(one), None, ctypes.byref(one), ctypes.byref(one)) == INVALID
    assert one.value == -7


def test_cells_and_buckets():
    """The restatement on values worked out by hand."""
    r = np.float32(0.05)
    inv = gc.inv_cell(r)
    assert inv.dtype == np.float32 and inv == np.float32(1.0) / np.float32(np.float32(0.05) * np.float32(1.001))
    p = np.array([[0.0, 0.05, 0.0501], [-0.0001, -0.05, -0.0501], [0.3, -0.2, 100.0]], dtype=np.float32)
    c = gc.cell_of(p, r)
    assert c.tolist() == [[0, 0, 1], [-1, -1, -2], [5, -4, 1998]]  # 0.3 / 0.05005 = 5.99, 100 / 0.05005 = 1998.002
    assert gc.bucket_of(np.array([0, 0, 0]), 1024) == 0
    assert gc.bucket_of(np.array([1, 0, 0]), 1 << 26) == 73856093 % (1 << 26)
    assert gc.bucket_of(np.array([1, 1, 1]), 1 << 20) == (73856093 ^ 19349663 ^ 83492791) % (1 << 20)
    m1 = (((-1 * 73856093) % (1 << 32)) ^ ((2 * 19349663) % (1 << 32)) ^ ((-3 * 83492791) % (1 << 32))) % 4096
    assert gc.bucket_of(np.array([-1, 2, -3]), 4096) == m1
    many = gc.bucket_of(np.random.default_rng(0).integers(-3000, 3000, (4000, 3)), 2048)
    assert many.min() >= 0 and many.max() < 2048 and len(np.unique(many)) > 1500


@functools.lru_cache(maxsize=None)
def _facts(kind, n):
    return gc.facts(gc.points(kind, n), gc.radius_of(kind))


@pytest.mark.parametrize("kind,n", gc.COLLISION)
def test_collision_cases_collide(oracle, kind, n):
    f = _facts(kind, n)
    assert f.T == (4096 if n == 729 else 1024)
    assert f.shared_queries >= 5 and f.crowded_buckets >= 5, f


def test_small_cases_step_the_table_and_pad():
    assert gc.SMALL_N == (1, 2, 3, 5, 200, 255, 256, 257) and gc.KNN_K == (1, 2, 16, 63, 64)
    assert [gc.table_size(n) for n in gc.SMALL_N] == [1024] * 7 + [2048]
    assert {n % 4 for n in gc.SMALL_N} == {0, 1, 2, 3}  # four rows per workgroup: every fill of the last one
    assert {(kind, n) for kind, n in gc.COLLISION[:2]} <= {(kind, n) for kind in gc.SMALL_KINDS for n in gc.SMALL_N}


def test_padding_and_lattice_rows(oracle):
    for kind, n in gc.COLLISION[:2]:
        nin = _facts(kind, n).nin
        assert nin.min() >= 1 and nin.max() < 16  # rows of k = 16, 63, 64 are padded; k = 1, 2 cut some
        assert (nin > 2).any() and (nin <= 2).any()
    nin = _facts("lattice", 729).nin
    assert nin.max() == 7 and (nin == 7).sum() == 7 ** 3 and nin.min() == 4  # interior / the eight corners
    assert set(gc.LATTICE_K) == {4, 7, 64}  # a cut through the six equal distances, the exact fit, padding
    p = gc.lattice()
    assert p.shape == (729, 3) and (p / np.float32(gc.LATTICE_STEP) == np.round(p / np.float32(gc.LATTICE_STEP))).all()
    assert np.abs(p).max() == 4 * gc.LATTICE_STEP and len(np.unique(p, axis=0)) == 729


@pytest.mark.parametrize("size", gc.CLUSTER_SIZES + (gc.OVERFLOW_SIZE,))
def test_cluster_cases(oracle, size):
    """The clump's rows hold exactly `size` points (the rank cut for k < size <= 1024, the boundary at 1024 / 1025),
    everything else stays far below any k > 4; a ball of the same radius about the clump's centre holds exactly the clump."""
    xyz, label, centres = gc.cluster_case(size)
    assert xyz.shape == (gc.CLUSTER_N, 3) and (label == 0).sum() == size and (label == 1).sum() == 40
    nin = gc.in_radius_counts(xyz, gc.RADIUS)
    assert (nin[label == 0] == size).all() and nin.max() == size
    assert (nin[label == 1] == 40).all() and nin[label == -1].max() < 16
    assert (nin[label == -1] < 4).any()  # padded rows at k = 4 too
    if size <= gc.KNN_CAP:
        assert all(k < size <= gc.KNN_CAP for k in gc.CLUSTER_K)
    else:
        assert size == gc.KNN_CAP + 1 == 1025
    where = np.flatnonzero(label == 0)  # spread over the index range: not one workgroup's rows
    assert where.min() < gc.CLUSTER_N // 8 and where.max() > gc.CLUSTER_N - gc.CLUSTER_N // 8
    d = np.sqrt(((xyz.astype(np.float64) - centres[0].astype(np.float64)) ** 2).sum(1))
    assert (d < gc.RADIUS).sum() == size and np.abs(d - gc.RADIUS).min() > 0.01  # (far from the rim: fp32 agrees)
    assert ((d < gc.RADIUS) == (label == 0)).all()


def test_cluster_sizes_sit_on_the_capacity():
    assert gc.CLUSTER_SIZES[-1] == gc.KNN_CAP == gc.BQG_CAP and gc.OVERFLOW_SIZE == gc.KNN_CAP + 1
    assert gc.CLUSTER_SIZES[0] == 65 > max(gc.CLUSTER_K) and min(gc.CLUSTER_K) == 4


def test_copies_case(oracle):
    n, count = gc.COPIES
    xyz, where = gc.copies(n, count)
    assert len(where) == count == 200 and (xyz[where] == xyz[where[0]]).all()
    nin = gc.in_radius_counts(xyz, gc.RADIUS)
    assert (nin[where] >= count).all() and nin[where].max() <= gc.KNN_CAP  # 200 zero distances: the index alone decides


@pytest.mark.parametrize("kind", ["translated", "signed"])
def test_shifted_cases(oracle, kind):
    xyz = gc.points(kind, gc.SHIFT_N)
    f = gc.facts(xyz, gc.RADIUS)
    assert xyz.shape == (gc.SHIFT_N, 3) and f.T == 32768
    assert f.nin.max() > 8 and np.median(f.nin) >= 4  # a graph, not isolated points
    cells = np.abs(gc.cell_of(xyz, gc.RADIUS)).max()
    if kind == "translated":
        # the 27-cell walk is complete below ~8380 cells from the origin: the case sits at a quarter of that
        assert (np.abs(xyz).max(0) > np.abs(np.asarray(gc.TRANSLATION)) - 1.0).all()
        assert 1900 < cells < 8380 // 4
    else:
        assert (xyz < 0).any(0).all() and (xyz > 0).any(0).all() and (gc.cell_of(xyz, gc.RADIUS) < 0).any()


def test_large_case_scans_with_a_carry():
    xyz = gc.room(gc.LARGE_N)
    assert xyz.shape == (gc.LARGE_N, 3) and gc.LARGE_N > 65536
    T = gc.table_size(gc.LARGE_N)
    assert gc.scan_blocks(T) == 512 > gc.SCAN_TOP
    f = gc.facts(xyz, gc.RADIUS, count_nin=False)
    assert f.shared_queries >= 5 and f.crowded_buckets >= 5
    # points fall into buckets on both sides of the first pass of the scan's top level
    b = gc.bucket_of(gc.cell_of(xyz, gc.RADIUS), T)
    assert (b < gc.SCAN_TOP * gc.SCAN_ITEMS).sum() > 10_000 and (b >= gc.SCAN_TOP * gc.SCAN_ITEMS).sum() > 10_000


@pytest.mark.parametrize("kind", gc.BALL_KINDS)
def test_ball_cases(oracle, kind):
    assert gc.BALL_N == (5, 255, 900, 6000) and gc.BALL_M == (1, 3, 37, 256) and gc.BALL_NSAMPLE == (1, 16, 64, 100)
    assert {m % 4 for m in gc.BALL_M} == {0, 1, 3}  # four centres per workgroup
    assert [gc.table_size(n) for n in gc.BALL_N] == [1024, 1024, 4096, 32768]
    r = gc.radius_of(kind, ball=True)
    most = 0
    for n in gc.BALL_N:
        xyz = gc.points(kind, n)
        assert xyz.shape == (n, 3)
        c = gc.ball_centres(xyz, max(gc.BALL_M))
        for m in gc.BALL_M:  # the centres of a smaller m: not the same ones
            cm = gc.ball_centres(xyz, m)
            assert cm.shape == (m, 3) and (m < 3 or (cm[1] > xyz.max(0) + 40).all())
        d2 = ((c[:, None, :].astype(np.float64) - xyz[None].astype(np.float64)) ** 2).sum(2)
        hits = (d2 < np.float64(np.float32(r)) ** 2).sum(1)
        assert hits[1] == 0  # the far centre
        on_set = (d2.min(1) == 0)
        assert on_set.sum() >= 80 and (~on_set).sum() >= 160  # centres that are points of the set, and that are not
        most = max(most, hits.max())
        if n == 6000:
            assert (hits == 0).sum() >= 1 and (hits > 1).sum() > 100
    if kind == "lattice":
        # the neighbours at exactly the radius are no hits: a lattice point's ball holds the point alone
        xyz = gc.points(kind, 900)
        d2 = ((xyz[:50, None, :].astype(np.float64) - xyz[None].astype(np.float64)) ** 2).sum(2)
        assert ((d2 < gc.LATTICE_STEP ** 2).sum(1) == 1).all() and ((d2 <= gc.LATTICE_STEP ** 2).sum(1) > 1).all()
    else:
        assert most > 64  # rows cut at nsample = 1, 16, 64 and padded at 100
