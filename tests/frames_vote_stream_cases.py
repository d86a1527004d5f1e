"""Inputs shared by test_frames_vote_stream_host.py and test_gpu_frames_vote_stream.py: the frames of
tests/frames_stream_cases.py, the label images and vote inputs of tests/frames_lift_cases.py, cut into chunks, and the
sequences of adds that every test feeds to a voter.  Every case is built once per process and must not be modified."""
import functools

import numpy as np
import torch

from geoformer_amd import frames
from tests import frames_lift_cases as lc
from tests import frames_stream_cases as sc

# Sizes, each next to the constant it straddles (csrc/frames_vote_stream.hip):
WAVE = lc.WAVE                   # lanes of a wave: a run of equal pairs ends at a wave's last lane at the latest
MAX_PROBES = 128                 # VS_MAX_PROBES = frames.VOTER_MAX_PROBES: a thread's probes in a table below 2 (P + T) slots
MIN_SLOTS = 64                   # VS_MIN_SLOTS: the smallest table
ONE_GROUP_CUTS = (1000, 2500)    # lc.FRAME_PIXELS = 4800 elements cut 1000 + 1500 + 2300: no cut is a multiple of WAVE (a
#                                  wave's run is split between adds) nor of lc.RUN = 3 (a run of "runs" is split too)
NARROW_CUTS = (1, 2)             # narrow3's 3 frames of 335 pixels as 1 + 1 + 1: 1005 elements, a partial last wave
FIRST_VALUES = 40                # a first add of 40 distinct values, each twice: 64 slots < 2 T = 160, so probes are bounded,
#                                  and it cannot fail: 40 keys leave 24 slots free, one of them within 64 < MAX_PROBES probes
MANY_VALUES = lc.MANY_VALUES     # 1000 more: above MIN_SLOTS + MAX_PROBES, so 64 slots must overflow (pigeonhole)
MANY_SLOTS = 4096                # >= 2 * (FIRST_VALUES + MANY_VALUES + FIRST_VALUES): the unbounded regime at every add
THIRD_VALUES, THIRD_SLOTS, THIRD_ELEMENTS = lc.THIRD_VALUES, lc.THIRD_SLOTS, lc.THIRD_ELEMENTS  # a third full, bounded
CROWDED_SLOTS = 256              # a given table that three successful adds of CROWDED_VALUES new values each fill above
CROWDED_VALUES = 50              # half (150 of 256; every add bounded: 256 < 2 T = 300)
DENSE4_PAIRS_10CM = 1358         # semantic pairs of dense4 at 10 cm, ignore 0 (the statement's, checked in the host test)
SPLITS = sc.SPLITS
IGNORE = lc.IGNORE

assert MAX_PROBES == frames.VOTER_MAX_PROBES and MIN_SLOTS == frames.VOTER_MIN_SLOTS
assert all(c % WAVE and c % lc.RUN for c in ONE_GROUP_CUTS) and ONE_GROUP_CUTS[-1] < lc.FRAME_PIXELS
assert FIRST_VALUES < MIN_SLOTS < 2 * FIRST_VALUES and MANY_VALUES > MIN_SLOTS + MAX_PROBES
assert MANY_SLOTS >= 2 * (2 * FIRST_VALUES + MANY_VALUES)
assert 3 * CROWDED_VALUES > CROWDED_SLOTS // 2 and CROWDED_SLOTS < 2 * 3 * CROWDED_VALUES  # bounded from the first add on
assert CROWDED_SLOTS - 3 * CROWDED_VALUES < MANY_VALUES  # the failing add cannot fit by pigeonhole


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def dense4_cells(cell, stride=1):
    """(cells int32 [4, Hs, Ws] of FuserHost fed dense4 frame by frame -- the numbers do not depend on the split --,
    the FuserHost)."""
    fz = frames.FuserHost(cell, stride)
    cells = torch.cat([fz.add(p) for p in sc.chunks(sc.dense4(), (1, 1, 1, 1))])
    return cells, fz


@functools.lru_cache(maxsize=None)
def narrow3_cells(stride=1):
    fz = frames.FuserHost(0.05, stride)
    cells = torch.cat([fz.add(p) for p in sc.chunks(sc.narrow3(), (1, 1, 1))])
    return cells, fz


def frame_adds(cells, image, sizes):
    """[(group, value)] per chunk of `sizes` frames: the cells and the (full-resolution) images of those frames."""
    at = np.cumsum((0,) + tuple(sizes))
    assert at[-1] == cells.shape[0] == image.shape[0]
    return [(cells[a:b].contiguous(), np.ascontiguousarray(image[a:b])) for a, b in zip(at[:-1], at[1:])]


def cut(group, value, cuts):
    """[(group, value)] of one-dimensional arrays cut at the element counts `cuts`."""
    at = (0,) + tuple(cuts) + (group.shape[0],)
    return [(np.ascontiguousarray(group[a:b]), np.ascontiguousarray(value[a:b])) for a, b in zip(at[:-1], at[1:])]


@functools.lru_cache(maxsize=None)
def changing_winner():
    """Three adds to group 0: value 2 three times (2 wins), value 1 four times (1 wins), value 2 once more (4 : 4, a tie:
    the smaller value, 1)."""
    i32 = lambda *v: np.array(v, np.int32)  # noqa: E731
    return [_freeze(i32(0, 0, 0), i32(2, 2, 2)), _freeze(i32(0, 0, 0, 0), i32(1, 1, 1, 1)), _freeze(i32(0), i32(2))]


@functools.lru_cache(maxsize=None)
def many_values():
    """(first, many, later): (group, value) int32 on group 0 -- FIRST_VALUES distinct values, each twice; MANY_VALUES
    other distinct values in a random order; and the first half of `many` again with some of `first`: values that hash
    among whatever a failed add of `many` left behind."""
    rng = np.random.default_rng(2)
    fv = np.repeat(np.arange(FIRST_VALUES, dtype=np.int32) * 3 + 2000, 2)
    mv = rng.permutation(MANY_VALUES).astype(np.int32) + 5
    lv = np.concatenate([mv[:FIRST_VALUES // 2], fv[:FIRST_VALUES]])
    return tuple(_freeze(np.zeros_like(v), v) for v in (fv, mv, lv))


@functools.lru_cache(maxsize=None)
def third_full():
    value = (np.arange(THIRD_ELEMENTS, dtype=np.int32) % THIRD_VALUES) * 17 + 1
    return _freeze(np.zeros_like(value), value)


@functools.lru_cache(maxsize=None)
def crowded():
    """Four adds of CROWDED_VALUES new values each on groups 0 .. 4 (each value three times, so runs of 3)."""
    out = []
    for k in range(4):
        v = np.repeat(np.arange(CROWDED_VALUES, dtype=np.int32) + 100 * k, 3)
        out.append(_freeze((v % 5).astype(np.int32), v))
    return out


def same_lifted(a, b):
    """Every field of two Lifted equal as bits (shapes and dtypes included)."""
    return all(x.dtype == y.dtype == torch.int32 and tuple(x.shape) == tuple(y.shape) and torch.equal(x.cpu(), y.cpu())
               for x, y in zip(a, b))


def same_state(a, b):
    """VoterHost.state() / Voter.state() of two voters equal."""
    return all(x.dtype == y.dtype and x.shape == y.shape and (x == y).all() for x, y in zip(a.state(), b.state()))


def sampled(value, stride):
    s = 1 if stride is None else stride
    return np.ascontiguousarray(value[:, ::s, ::s]) if s != 1 else value
