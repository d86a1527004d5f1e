"""csrc/frames_track.hip on the GPU: frames.Tracker bit for bit against frames.TrackerHost after EVERY update -- Tracked's
fields, state() and the counters -- each sequence from a fresh Tracker twice with the lane-run aggregation and once
without it.  The inputs and what each size straddles are named in tests/frames_track_cases.py."""
import numpy as np
import pytest
import torch

from geoformer_amd import frames
from tests import frames_cases as fc
from tests import frames_stream_cases as sc
from tests import frames_track_cases as tc

pytestmark = pytest.mark.gpu


def _check(updates, on_device=True, host_kw=None, **dev_kw):
    """The three device runs of a sequence of updates against the statement, after every update; returns (the
    TrackerHost, the three Trackers).  on_device: the arguments are handed over as CUDA tensors (what Fuser.kept and
    label_batches return), else as numpy arrays, which the host checks and sizes the map from."""
    host_kw = host_kw or {}
    th, want = frames.TrackerHost(**host_kw), []
    for up in updates:
        tracked = th.update(*up.args())
        want.append((tracked, th.state(), tc.counters(th)))
    trackers = []
    for aggregate in (True, None, False):
        t = frames.Tracker(aggregate=aggregate, **host_kw, **dev_kw)
        for up, (tracked_w, state_w, counters_w) in zip(updates, want):
            got = t.update(*up.args("cuda" if on_device else None))
            assert all(x.is_cuda for x in got) and tc.same_tracked(got, tracked_w)
            assert tc.same_state(t.state(), state_w) and tc.counters(t) == counters_w
        trackers.append(t)
    return th, trackers


def test_limits_are_the_modules(hip):
    from geoformer_amd import _lib

    lib = _lib.load()
    assert frames.tracker_limits() == (tc.MAX_ROWS, tc.MAX_PROBES, 1 << 30) == \
        (frames.TRACK_MAX_ROWS, frames.TRACK_MAX_PROBES, frames.TRACK_MAX_TRACKS)
    for p, live in ((0, 0), (1, 0), (50, 50), (32, 32), (4096, 0), (4096, 1 << 20), (7, 1), (8, 0), (4096, 1 << 30)):
        assert lib.gf_frames_track_default_slots(p, live) == frames.tracker_slots(p, live, 0)[0], (p, live)
    assert lib.gf_frames_track_default_slots(4097, 0) == 0 and lib.gf_frames_track_default_slots(0, -1) == 0
    assert lib.gf_frames_track_scratch_bytes(1000, 10, 5, 64) >= 4 * 1000 + 12 * 64 + 8 * 10 + 16 * 5
    for bad in ((-1, 0, 0, 64), ((1 << 29) + 1, 0, 0, 64), (0, 4097, 0, 64), (0, 0, -1, 64), (0, 0, 0, 63), (0, 0, 0, 32),
                (0, 0, 0, 1 << 31)):
        assert lib.gf_frames_track_scratch_bytes(*bad) == 0, bad
    assert lib.gf_frames_track_columns() == len(frames.TrackTable._fields) == 8


@pytest.mark.parametrize("on_device", [True, False])
@pytest.mark.parametrize("name", ["empty_and_tiny", "partial_wave", "whole_waves", "one_pair", "runs"])
def test_a_sequence_equals_the_statement(hip, name, on_device):
    th, trackers = _check(tc.sequences()[name], on_device)
    assert all(t.retries == 0 for t in trackers)
    if name == "whole_waves":   # the map grew past its first capacity: with the cells on the device, by the count pass's word
        assert th.cells == 12000 - 1 > tc.FIRST_MAP and all(t.map_growths >= 1 for t in trackers)
    if name == "partial_wave":
        assert th.tracks == 11 and all(t.map_growths == 0 and 11 < t.pairs <= 22 for t in trackers)   # each block on two tracks
    if name == "one_pair":
        assert th.tracks == 1 and th.table().hits.tolist() == [3] and all(t.pairs == 1 for t in trackers)


def test_rows_at_the_limit_alone_on_their_tracks(hip):
    """No run at all: MAX_ROWS rows of one point each, then the rows permuted; the table grows past its first capacity."""
    th, trackers = _check(tc.sequences()["alone"])
    assert th.tracks == th.live == tc.MAX_ROWS > tc.FIRST_TABLE and th.table().hits.tolist() == [2] * tc.MAX_ROWS
    assert all(t.row_growths >= 1 and t.pairs == tc.MAX_ROWS for t in trackers)


def test_a_row_too_many_is_refused_before_any_launch(hip):
    t = frames.Tracker()
    up = tc.sequences()["alone"][0]
    t.update(*up.args("cuda"))
    before, counters = t.state(), tc.counters(t)
    p = tc.MAX_ROWS + 1
    with pytest.raises(ValueError, match="rows in one update"):
        t.update(up.cells, up.owner, np.zeros(p, np.int32), np.zeros(p, np.float32))
    assert tc.same_state(t.state(), before) and tc.counters(t) == counters


def test_the_default_table_overflows_once_and_the_result_is_equal(hip):
    th, trackers = _check(tc.sequences()["cross"])
    assert all(t.retries == 1 and t.pairs == tc.CROSS for t in trackers)   # (pairs: the last update's, CROSS blocks on CROSS tracks)
    t = frames.Tracker()
    first, second, _ = tc.sequences()["cross"]
    t.update(*first.args("cuda"))
    t.update(*second.args("cuda"))
    assert t.retries == 1 and t.pairs == tc.CROSS * tc.CROSS


def test_a_given_table_that_overflows_changes_nothing(hip):
    first, second, _ = tc.sequences()["cross"]
    third = tc.Update(first.cells, first.owner, *tc.rows(tc.CROSS, 3))     # the first update's rows again: CROSS pairs, which fit
    th = frames.TrackerHost()
    th.update(*first.args())
    for aggregate in (True, False):
        t = frames.Tracker(slots=tc.MIN_SLOTS, aggregate=aggregate)
        t.update(*first.args("cuda"))          # (no track yet, so no pair: 64 slots are plenty)
        before, counters = t.state(), tc.counters(t)
        assert tc.same_state(before, th.state())
        with pytest.raises(ValueError, match="2048 slots are always enough"):
            t.update(*second.args("cuda"))
        assert tc.same_state(t.state(), before) and tc.counters(t) == counters and t.retries == 0
        want = frames.TrackerHost()
        want.update(*first.args())
        assert tc.same_tracked(t.update(*third.args("cuda")), want.update(*third.args()))
        assert tc.same_state(t.state(), want.state()) and tc.counters(t) == tc.counters(want)
    with pytest.raises(ValueError, match="slots"):
        frames.Tracker(slots=100)


def test_cross_products_beyond_32_bits(hip):
    """The wide row's better track is decided by products above 2^32 that an int32 product orders the other way."""
    th, trackers = _check(tc.sequences()["wide"])
    assert th.tracks == 3 and th.table().hits.tolist() == [1, 2, 1]     # row 0 continued track 1; row 1 is new


def test_hold_and_retire(hip):
    th, trackers = _check(tc.sequences()["hold_and_retire"], host_kw=dict(max_misses=1))
    assert th.table().alive.tolist() == [True, True, False, True] and all(t.live == 3 for t in trackers)
    ids = trackers[0].labels(torch.arange(300, dtype=torch.int32, device="cuda"))
    assert ids.is_cuda and torch.equal(ids.cpu(), th.labels(np.arange(300, dtype=np.int32)))


@pytest.mark.parametrize("same_class", [False, True])
def test_random_sequences_with_keep_and_min_points(hip, same_class):
    for seed in (1, 2):
        kw = dict(iou=0.3 if seed % 2 else 0.15, max_misses=seed % 3, min_points=1 + 3 * (seed % 2), same_class=same_class)
        th, trackers = _check(tc.random_sequence(seed), host_kw=kw)
        assert th.tracks > th.live > 0


def test_device_flags_leave_the_state_as_it_was(hip):
    up = tc.by_blocks(tc.NARROW_POINTS, 97)
    th = frames.TrackerHost()
    th.update(*up.args())
    for aggregate in (True, False):
        t = frames.Tracker(aggregate=aggregate)
        t.update(*up.args("cuda"))
        before, counters = t.state(), tc.counters(t)
        cells, owner, cls, score, _ = up.args("cuda")
        swapped = cells.clone()
        swapped[[500, 501]] = swapped[[501, 500]]
        equal = cells.clone()
        equal[700] = equal[699]
        negative = cells.clone()
        negative[0] = -1
        high, low = owner.clone(), owner.clone()
        high[1004], low[3] = cls.shape[0], -2
        far = cells.clone()
        far[-1] = 2 ** 31 - 1           # ascending, and beyond any map
        for c, o, what in ((swapped, owner, "ascending"), (equal, owner, "ascending"), (negative, owner, "ascending"),
                           (cells, high, "owner"), (cells, low, "owner"), (far, owner, "cells")):
            with pytest.raises(ValueError, match=what):
                t.update(c, o, cls, score)
            assert tc.same_state(t.state(), before) and tc.counters(t) == counters
        want = frames.TrackerHost()
        want.update(*up.args())
        nxt = tc.by_blocks(tc.NARROW_POINTS, 97, shift=20, seed=1)
        assert tc.same_tracked(t.update(*nxt.args("cuda")), want.update(*nxt.args()))
        assert tc.same_state(t.state(), want.state())


# ---- through the model --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(hip):
    from geoformer_amd.model import GeoFormer, load_config
    from tests.util import synthetic_state_dict

    m = GeoFormer(load_config("test_geoformer_scannet.yaml"))
    m.load_state_dict(synthetic_state_dict(m.state_dict(), 0))
    m.cuda()
    m.eval()
    return m


def test_a_stream_through_the_model_is_tracked_as_the_statement_tracks_it(model):
    from geoformer_amd import batch_eval

    fu = frames.Fuser(0.02)
    tracker, th = frames.Tracker(), frames.TrackerHost()
    cells = []
    for part in sc.chunks(sc.dense4(), tc.SPLITS["2+2"]):
        cells.append(fu.add(part))
        fused = fu.snapshot(1, torch.cat(cells))
        raw, shift = fused.raw_scene()
        np.random.seed(0)
        (name, labels), = batch_eval.label_batches(model, [("frames", raw)], 1)
        got = frames.track_scene(tracker, fu, labels)
        host = labels.to_host()
        want = th.update(fu.kept(1).cpu().numpy(), host.owner, host.table.label_id, host.table.score, host.table.kept)
        assert tc.same_tracked(got, want) and tc.same_state(tracker.state(), th.state()) and tc.counters(tracker) == tc.counters(th)
        image = frames.gather(fused, got.ids)
        assert tuple(image.shape) == tuple(fused.point_of.shape) == (len(cells) * 2, fc.DENSE[1], fc.DENSE[0])
        assert bool(((image >= 0) == (fused.point_of >= 0) & (got.ids[fused.point_of.clamp(min=0).long()] >= 0)).all())
    assert th.updates == 2 and th.cells == fu.cells
