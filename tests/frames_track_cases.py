"""Inputs shared by test_frames_track_host.py and test_gpu_frames_track.py: sequences of tracker updates whose owners are
integer functions of the cell number (no model needed), the frames of tests/frames_stream_cases.py with block labels, and
the comparisons.  Every case is built once per process and must not be modified."""
import functools
from fractions import Fraction

import numpy as np
import torch

from geoformer_amd import frames
from tests import frames_cases as fc
from tests import frames_lift_cases as lc
from tests import frames_stream_cases as sc

# Sizes, each next to the constant it straddles (csrc/frames_track.hip):
WAVE = lc.WAVE                   # lanes of a wave: a run of equal (row, track) pairs ends at a wave's last lane at the latest
NARROW_POINTS = lc.NARROW_PIXELS  # 1005 points: 15 waves + 45 lanes, a partial last wave (and 3 blocks of FT_THREADS + 237)
WAVES_POINTS = lc.FRAME_PIXELS   # 4800 points: 75 whole waves
RUN = lc.RUN                     # 3: a run length that does not divide WAVE, so runs cross the wave boundaries
MAX_ROWS = 4096                  # FT_MAX_ROWS = frames.TRACK_MAX_ROWS: FT_MATCH_THREADS = 1024 threads scan 4 rows each
MAX_PROBES = 128                 # FT_MAX_PROBES = frames.TRACK_MAX_PROBES: a thread's probes in a table below 2 m slots
MIN_SLOTS = 64                   # FT_MIN_SLOTS: the smallest pair table
CROSS = 32                       # 32 rows x 32 tracks with all 1024 pairs present: the default table of 8 (32 + 32) = 512
#                                  slots cannot hold them (pigeonhole), the proven one of 2 m = 2048 can; a given table of
#                                  MIN_SLOTS cannot either: 1024 > MIN_SLOTS + MAX_PROBES
FIRST_MAP, FIRST_TABLE = 1024, 64   # frames._TRACK_MIN_MAP / _TRACK_MIN_TABLE: the first capacities of a Tracker's map
#                                  and table; NARROW_POINTS cells stay within the first map, WAVES_POINTS grow it
WIDE_ROW = 300000                # points of the wide row: its cross-products n * union exceed 2^32 (see wide())
SPLITS = {k: v for k, v in sc.SPLITS.items() if k != "4"}   # 1+3, 2+2, 4x1

assert MAX_ROWS == frames.TRACK_MAX_ROWS and MAX_PROBES == frames.TRACK_MAX_PROBES and MIN_SLOTS == frames.TRACK_MIN_SLOTS
assert (FIRST_MAP, FIRST_TABLE) == (frames._TRACK_MIN_MAP, frames._TRACK_MIN_TABLE)
assert NARROW_POINTS % WAVE and NARROW_POINTS < FIRST_MAP < WAVES_POINTS and WAVES_POINTS % WAVE == 0 and WAVE % RUN
assert CROSS * CROSS > frames.tracker_slots(CROSS, CROSS, CROSS * CROSS)[0] and CROSS * CROSS > MIN_SLOTS + MAX_PROBES
assert frames.tracker_slots(CROSS, CROSS, CROSS * CROSS) == (512, 2048)


class Update:
    """One update's arguments, frozen."""

    def __init__(self, cells, owner, cls, score, keep=None):
        self.cells, self.owner = np.ascontiguousarray(cells, np.int32), np.ascontiguousarray(owner, np.int32)
        self.cls, self.score = np.ascontiguousarray(cls, np.int32), np.ascontiguousarray(score, np.float32)
        self.keep = None if keep is None else np.ascontiguousarray(keep, bool)
        for a in (self.cells, self.owner, self.cls, self.score) + (() if keep is None else (self.keep,)):
            a.setflags(write=False)

    def args(self, device=None):
        out = (self.cells, self.owner, self.cls, self.score, self.keep)
        if device is None:
            return out
        return tuple(None if a is None else torch.from_numpy(a.copy()).to(device) for a in out)


def rows(p, seed=0):
    """(cls [p], score [p]) of p rows: classes 1 .. 5 and distinct scores in (0.5, 1)."""
    rng = np.random.default_rng(seed)
    return (np.arange(p) * 7 + seed) % 5 + 1, (0.5 + 0.5 * rng.permutation(p + 1)[:p] / (p + 1)).astype(np.float32)


def by_blocks(m, block, first=0, step=1, seed=0, shift=0):
    """An update over the cells first, first + step, ..: the owner of cell c is (c + shift) // block, numbered from 0."""
    cells = first + step * np.arange(m, dtype=np.int64)
    owner = (cells + shift) // block
    owner -= owner.min() if m else 0
    return Update(cells, owner, *rows(int(owner.max()) + 1 if m else 0, seed))


@functools.lru_cache(maxsize=None)
def sequences():
    """{name: [Update]}: the regimes of the device test, each a sequence from a fresh tracker."""
    out = {}
    none = Update(np.zeros(0), np.zeros(0), np.zeros(0), np.zeros(0))
    one = Update([5], [0], [3], [0.75])
    out["empty_and_tiny"] = [none, one, none, one, Update([5], [-1], [3], [0.5])]
    # a partial last wave; blocks of 97 cells that slide by 20 cells per update (IoU 77 / 117 > 0.3: every id is kept)
    out["partial_wave"] = [by_blocks(NARROW_POINTS, 97, shift=20 * k, seed=k) for k in range(3)]
    # whole waves, and a map that grows past FIRST_MAP: first 600 cells, then 4800, then every second cell up to 12000
    out["whole_waves"] = [by_blocks(600, 100), by_blocks(WAVES_POINTS, 100, seed=1), by_blocks(6000, 100, step=2, seed=2),
                          by_blocks(WAVES_POINTS, 150, seed=3)]
    # one row on one track: every wave one run, every add on one slot
    out["one_pair"] = [by_blocks(WAVES_POINTS, WAVES_POINTS, seed=k) for k in range(3)]
    # MAX_ROWS rows alone on MAX_ROWS tracks (no two adjacent lanes share a pair), then the rows permuted
    alone = by_blocks(MAX_ROWS, 1)
    perm = np.random.default_rng(5).permutation(MAX_ROWS)
    inv = np.argsort(perm)
    out["alone"] = [alone, Update(alone.cells, perm[alone.owner], alone.cls[inv], alone.score[inv])]
    # runs of RUN points that cross the wave boundaries: blocks of 3 cells, then the same blocks shifted by one cell
    out["runs"] = [by_blocks(NARROW_POINTS, RUN), by_blocks(NARROW_POINTS, RUN, shift=1, seed=1), by_blocks(NARROW_POINTS, RUN, seed=2)]
    # every pair of CROSS rows and CROSS tracks present once: cell c is track c % CROSS, then row c // CROSS
    c = np.arange(CROSS * CROSS)
    out["cross"] = [Update(c, c % CROSS, *rows(CROSS)), Update(c, c // CROSS, *rows(CROSS, 1)), by_blocks(CROSS * CROSS, CROSS, seed=2)]
    out["wide"] = wide()
    out["hold_and_retire"] = hold_and_retire()
    # rows that are not kept and rows below min_points are used with their own parameters in the tests
    return out


@functools.lru_cache(maxsize=None)
def wide():
    """Two updates.  The first makes track 0 of B0 cells and track 1 of B1 cells.  In the second, row 0 (WIDE_ROW points)
    covers N0 cells of track 0 and N1 of track 1; a second row covers the rest of both.  Row 0's two candidates have IoU
    cross-products above 2^32 whose order an int32 product gets wrong: the counts are searched here so that Fraction
    decides for track 1 while the wrapped products decide for track 0."""
    def wrap(v):
        return (v + 2 ** 31) % 2 ** 32 - 2 ** 31

    a = WIDE_ROW
    for N0 in range(100000, 100200):
        for N1 in range(140000, 140200, 7):
            B0, B1 = N0 + 1000, N1 + 65000
            u0, u1 = a + B0 - N0, a + B1 - N1
            l, r = N0 * u1, N1 * u0   # IoU0 > IoU1  <=>  l > r
            if Fraction(N1, u1) > Fraction(N0, u0) and wrap(l) > wrap(r) and min(l, r) > 2 ** 32 and Fraction(N1, u1) > Fraction(3, 10):
                break
        else:
            continue
        break
    else:
        raise AssertionError("no counts found")
    assert Fraction(N1, u1) > Fraction(N0, u0) and wrap(l) > wrap(r)
    m = a + (B0 - N0) + (B1 - N1)
    cells = np.arange(m)
    first = np.where(cells < B0, 0, np.where(cells < B0 + B1, 1, -1))
    # row 0: N0 cells of track 0, N1 cells of track 1 and the a - N0 - N1 cells without a track; row 1: the rest
    second = np.ones(m, np.int64)
    second[:N0] = 0
    second[B0:B0 + N1] = 0
    second[B0 + B1:] = 0
    assert (second == 0).sum() == a and (first == -1).sum() == a - N0 - N1
    return [Update(cells, first, [1, 2], [0.5, 0.5]), Update(cells, second, [1, 2], [0.5, 0.5])]


@functools.lru_cache(maxsize=None)
def hold_and_retire():
    """For max_misses = 1.  Cells 0 .. 299 in three blocks of 100.  Block 1 is missed once and seen again (its id is kept),
    block 2 is missed twice (retired: its cells read -1) and then seen again (a new id, never the old one)."""
    cells = np.arange(300)
    blocks = cells // 100
    cls, score = rows(3)

    def seen(*which):
        lut = np.full(3, -1)
        lut[list(which)] = np.arange(len(which))
        return Update(cells, lut[blocks], cls[list(which)], score[list(which)])

    return [seen(0, 1, 2), seen(0, 2), seen(0, 1), seen(0, 1), seen(0, 1, 2)]


def random_sequence(seed, updates=5, points=600, max_rows=12):
    """Updates over growing cell sets: random cells; the owners are blocks between cuts that move a little from update to
    update (so that most blocks match, some split and some are new), renumbered at random, with noise; some rows are not
    kept and some change their class."""
    rng = np.random.default_rng(seed)
    out, top = [], 700
    cuts = np.sort(rng.choice(top, size=max_rows - 1, replace=False))
    for u in range(updates):
        top += int(rng.integers(20, 200))
        cells = np.sort(rng.choice(top, size=min(points, top - 20), replace=False))
        p = int(rng.integers(max_rows // 2, max_rows + 1))
        mine = np.sort(rng.choice(cuts, size=p - 1, replace=False) + rng.integers(-15, 16, p - 1))
        owner = np.searchsorted(mine, cells, side="right")
        order = rng.permutation(p)
        owner = order[owner]
        noise = rng.random(cells.shape[0])
        owner = np.where(noise < 0.1, -1, np.where(noise < 0.2, rng.integers(0, p, cells.shape[0]), owner))
        cls = np.empty(p, np.int64)
        cls[order] = np.where(rng.random(p) < 0.8, 1, rng.integers(1, 4, p))
        out.append(Update(cells, owner, cls, rng.integers(0, 8, p).astype(np.float32) / 8, rng.random(p) < 0.85))
    return out


@functools.lru_cache(maxsize=None)
def dense4_block_images():
    """frames_lift_cases.block_images' rule on the four frames of frames_stream_cases.dense4."""
    case = fc.dense(fc.DENSE_FRAMES_TOP)
    idx = np.maximum(case.index, 0).astype(np.int64)
    fg = case.index >= 0
    sem = np.where(fg, np.where(idx % 7 == 0, 6, (idx // 500) % 5 + 1), lc.IGNORE).astype(np.int32)
    ins = np.where(fg & (idx % 3 != 0), idx // 500 + 1, lc.IGNORE).astype(np.int32)
    for a in (sem, ins):
        a.setflags(write=False)
    return sem, ins


def same_tracked(got, want):
    """Every field of two Tracked equal as bits (shapes and dtypes included)."""
    return all(x.dtype == y.dtype and tuple(x.shape) == tuple(y.shape) and torch.equal(x.cpu(), y.cpu()) for x, y in zip(got, want))


def same_state(got, want):
    """state() of two trackers equal: the map, and every column of the table as bits."""
    (ma, ta), (mb, tb) = got, want
    cols = all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(ta, tb))
    return ma.dtype == mb.dtype == np.int32 and ma.shape == mb.shape and (ma == mb).all() and cols


def counters(t):
    return t.tracks, t.live, t.cells, t.updates
