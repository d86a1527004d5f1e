"""Inputs shared by test_frames_stream_host.py and test_gpu_frames_stream.py: tests/frames_cases.py's synthetic frames, cut
into chunks.  Every case is built once per process and must not be modified."""
import functools

import numpy as np
import torch

from geoformer_amd import frames
from tests import frames_cases as fc

# Sizes, each next to the constant it straddles (csrc/frames_stream.hip):
MAX_PROBES = 128             # FM_MAX_PROBES = frames.STREAM_MAX_PROBES: a thread's probes in a table below 2 (M + n) slots
MIN_SLOTS = 64               # FM_MIN_SLOTS: the smallest table; dense(4)'s first frame brings far more than 64 cells, so
#                              a table of 64 slots fills up and a thread runs out of probes: the overflow word
UNBOUNDED_SLOTS = 1 << 16    # >= 2 (M + n) at every add of dense(4) at 2 cm (M + n <= 7242 + 4800): probing unbounded
CROWDED_SLOTS = 8192         # a given table that dense(4)'s first three frames fill above half (5432 cells at 2 cm from an
#                              origin 1 m below the points) with no run of occupied slots longer than 46, far below
#                              MAX_PROBES, so those adds cannot overflow; 20000 more cells cannot fit: the overflow
SMALL_CAPACITY = 16          # rows of count / sums: below the cells of any first frame, so the rows grow at once
COARSE = 0.1                 # metres: the cell at which these frames put 3 and more pixels into a cell (min_obs = 3)
ONE_CELL = 100.0             # metres: every point of the scene in one cell: full contention, every wave one run
DENSE4_CELLS = 7242          # cells of dense(4), uint16, stride 1, at 2 cm with the origin at the points' minimum
DENSE4_PIXELS = 7323         # valid pixels of dense(4), uint16, stride 1
SPLITS = {"1+3": (1, 3), "2+2": (2, 2), "4x1": (1, 1, 1, 1), "4": (4,)}
REACH = 4096.0               # FM_REACH = frames.STREAM_REACH
CELL_POINTS = fc.CELL_POINTS  # 20000 points alone in their cells, as 2 x 10000: 157 SMALL_CHUNKs each (< TOP) but 313 in
#                               all; at chunk 64 the second add numbers cells above the first's 10000

assert MAX_PROBES == frames.STREAM_MAX_PROBES and REACH == frames.STREAM_REACH
assert UNBOUNDED_SLOTS >= 2 * (DENSE4_CELLS + fc.DENSE[0] * fc.DENSE[1])


def sub(fr, a, b):
    """Frames a .. b - 1 of a Frames."""
    return frames.Frames(fr.depth[a:b].contiguous(), None if fr.color is None else fr.color[a:b].contiguous(),
                         np.ascontiguousarray(fr.table[a:b]), fr.depth_shift)


def chunks(fr, sizes):
    """fr cut into consecutive chunks of the given numbers of frames."""
    assert sum(sizes) == fr.depth.shape[0]
    at = np.cumsum((0,) + tuple(sizes))
    return [sub(fr, int(a), int(b)) for a, b in zip(at[:-1], at[1:])]


@functools.lru_cache(maxsize=None)
def dense4(kind="u16", color=True):
    """frames_cases.dense(4) as Frames."""
    return fc.make(fc.dense(fc.DENSE_FRAMES_TOP), kind, color)


@functools.lru_cache(maxsize=None)
def gaps3():
    """frames_cases.gaps(3) as float32 Frames: the middle frame has no valid pixel, the last keeps every pixel."""
    return fc.make(fc.dense(3), "f32", True, depth=fc.gaps(3))


@functools.lru_cache(maxsize=None)
def nasty3():
    """frames_cases.nasty() as float32 Frames: NaN, inf, 0 and negative depths over a fifth of the pixels."""
    return fc.make(fc.dense(3), "f32", True, depth=fc.nasty())


@functools.lru_cache(maxsize=None)
def narrow3(kind="u16"):
    return fc.make(fc.narrow(), kind, True)


def moved(fr, offset):
    """fr with every pose translated by `offset` metres (three numbers): the same frames seen from elsewhere."""
    F = fr.depth.shape[0]
    pose = np.zeros((F, 4, 4))
    pose[:, :3, :] = fr.table[:, 4:].astype(np.float64).reshape(F, 3, 4)
    pose[:, 3, 3] = 1
    pose[:, :3, 3] += np.asarray(offset, np.float64)
    return frames.make(fr.depth, fr.table[0, :4].astype(np.float64), pose, fr.color, fr.depth_shift)


def same_fused(a, b):
    """Every field of two Fused equal as bits (shapes and dtypes included)."""
    for x, y in zip(a, b):
        x, y = x.detach().cpu(), y.detach().cpu()
        if x.dtype != y.dtype or tuple(x.shape) != tuple(y.shape):
            return False
        xv = x.view(torch.int32) if x.dtype == torch.float32 else x
        yv = y.view(torch.int32) if y.dtype == torch.float32 else y
        if not bool((xv == yv).all()):
            return False
    return True


def same_state(a, b):
    """FuserHost.state() / Fuser.state() of two maps equal."""
    return all(x.shape == y.shape and (x == y).all() for x, y in zip(a.state(), b.state()))
