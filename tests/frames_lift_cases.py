"""Per-pixel labels and vote inputs shared by test_frames_lift_host.py and test_gpu_frames_lift.py, on top of the rendered
frames of tests/frames_cases.py.  Every case is built once per process and must not be modified."""
import functools

import numpy as np

from geoformer_amd import frames, scene
from tests import frames_cases as fc

# Sizes, each next to the constant it straddles (csrc/frames_vote.hip):
WAVE = 64                    # lanes of a wave: a run of equal pairs ends at a wave's last lane at the latest
MAX_PROBES = 128             # FV_MAX_PROBES = frames.VOTE_MAX_PROBES: the probes of a thread in a table below 2 T slots
MIN_SLOTS = 64               # the smallest table
NARROW_PIXELS = 1005         # 3 frames of fc.NARROW: 15 waves + 45 lanes, a partial last wave
FRAME_PIXELS = 4800          # one frame of fc.DENSE = 75 waves: the elements of the one-group cases
RUN = 3                      # a run length that does not divide WAVE: runs cross the wave boundaries
MANY_VALUES = 1000           # distinct values on one group: more than MIN_SLOTS + MAX_PROBES, so 64 slots must overflow
MANY_SLOTS = 2048            # >= 2 * MANY_VALUES: the unbounded regime
THIRD_VALUES = 300           # distinct values in THIRD_SLOTS = 1024 slots: a third full, below 2 T, bounded probes
THIRD_SLOTS = 1024
IGNORE = 0                   # "unannotated" in the label images, as in ScanNet's label-filt / instance-filt

assert MAX_PROBES == frames.VOTE_MAX_PROBES and MIN_SLOTS == frames.VOTE_MIN_SLOTS
assert fc.NARROW[0] * fc.NARROW[1] * 3 == NARROW_PIXELS and NARROW_PIXELS % WAVE
assert fc.DENSE[0] * fc.DENSE[1] == FRAME_PIXELS and WAVE % RUN and MANY_VALUES > MIN_SLOTS + MAX_PROBES
THIRD_ELEMENTS = 900         # three elements per value: 2 T = 1800 > THIRD_SLOTS
assert MANY_SLOTS >= 2 * MANY_VALUES and 3 * THIRD_VALUES == THIRD_ELEMENTS and THIRD_SLOTS < 2 * THIRD_ELEMENTS


@functools.lru_cache(maxsize=None)
def point_labels():
    """(semantic int64 [N], instance int64 [N]) of scene.make_small_scene(8192, 7): classes 0, 1 and 4, one instance
    (id 0) and -100 elsewhere."""
    sc = scene.make_small_scene(8192, 7)
    return sc["label"], sc["instance"]


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def images(case_name, n=3):
    """(semantic uint8 [F, H, W], instance uint16 [F, H, W]) of a rendered case ("narrow", "dense", "round_trip"): the
    scene's class + 1 and instance id + 1 of the source point of every pixel (case.index), IGNORE on the background and
    where the point has no instance."""
    case = getattr(fc, case_name)() if case_name != "dense" else fc.dense(n)
    lab, inst = point_labels()
    idx = np.maximum(case.index, 0)
    sem = np.where(case.index >= 0, lab[idx] + 1, IGNORE).astype(np.uint8)
    ins = np.where((case.index >= 0) & (inst[idx] >= 0), inst[idx] + 1, IGNORE).astype(np.uint16)
    return _freeze(sem, ins)


@functools.lru_cache(maxsize=None)
def block_images(case_name):
    """(semantic int32 [F, H, W], instance int32 [F, H, W]) made from the source point's number, so that a case has many
    instances of several classes, each with some points of a wrong class: instance = index // 500 + 1 on two points in
    three (IGNORE on the others), class = (index // 500) % 5 + 1 except on every 7th point, which says class 6."""
    case = getattr(fc, case_name)()
    idx = np.maximum(case.index, 0).astype(np.int64)
    fg = case.index >= 0
    sem = np.where(fg, np.where(idx % 7 == 0, 6, (idx // 500) % 5 + 1), IGNORE).astype(np.int32)
    ins = np.where(fg & (idx % 3 != 0), idx // 500 + 1, IGNORE).astype(np.int32)
    return _freeze(sem, ins)


@functools.lru_cache(maxsize=None)
def random_votes(T=600, n=37, values=5, seed=11):
    """(group int32 [T], value int32 [T]): groups in [-3, n) and values in [-2, values): negative ones sown in."""
    rng = np.random.default_rng(seed)
    return _freeze(rng.integers(-3, n, T).astype(np.int32), rng.integers(-2, values, T).astype(np.int32))


def one_group(kind):
    """(group int32 [FRAME_PIXELS], value int32 [FRAME_PIXELS], n) of the one-dimensional regimes:
    "same": one group, one value -- every wave one run, full contention on one slot;
    "alternate": one group, values 1, 2, 1, 2, ... lane by lane -- no run longer than 1;
    "runs": groups in runs of RUN elements (group t // RUN), value 7 -- runs that cross the wave boundaries;
    "alone": every element its own group."""
    t = np.arange(FRAME_PIXELS, dtype=np.int32)
    if kind == "same":
        return np.zeros_like(t), np.full_like(t, 5), 1
    if kind == "alternate":
        return np.zeros_like(t), 1 + (t & 1), 1
    if kind == "runs":
        return t // RUN, np.full_like(t, 7), FRAME_PIXELS // RUN
    assert kind == "alone"
    return t, t % 11, FRAME_PIXELS


def counter_vote(group, value, n, ignore=None, fill=-100):
    """vote_host's rule as a plain Python loop over a dict of Counters: (label, votes, total, pairs)."""
    from collections import Counter

    per = {}
    for g, v in zip(np.asarray(group).reshape(-1).tolist(), np.asarray(value).reshape(-1).tolist()):
        assert g < n
        if g >= 0 and v >= 0 and (ignore is None or v != ignore):
            per.setdefault(g, Counter())[v] += 1
    label, votes, total = [fill] * n, [0] * n, [0] * n
    for g, c in per.items():
        top = max(c.values())
        label[g], votes[g], total[g] = min(v for v, k in c.items() if k == top), top, sum(c.values())
    return (np.array(label, np.int32), np.array(votes, np.int32), np.array(total, np.int32),
            sum(len(c) for c in per.values()))
