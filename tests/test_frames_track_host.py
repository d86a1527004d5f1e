"""frames.TrackerHost, the statement of the tracker (no GPU): against a dense restatement in plain Python loops with
fractions.Fraction for the IoU order, its properties, and a streamed run through FuserHost and two VoterHosts.  The
inputs are named in tests/frames_track_cases.py."""
from fractions import Fraction

import numpy as np
import pytest
import torch

from geoformer_amd import frames
from tests import frames_stream_cases as sc
from tests import frames_track_cases as tc


def U(cells, owner, cls, score, keep=None):
    """Arguments of an update from plain sequences."""
    return tc.Update(cells, owner, cls, score, keep).args()


class Dense:
    """The rule of frames.TrackerHost once more, as loops over a [p, T] matrix."""

    def __init__(self, iou=0.3, max_misses=2, min_points=1, same_class=False):
        self.iou, self.max_misses, self.min_points, self.same_class = iou, max_misses, min_points, same_class
        self.map, self.tracks, self.u = {}, [], 0   # cell -> track; [dict per track]

    def update(self, cells, owner, cls, score, keep=None):
        p, T, u = len(cls), len(self.tracks), self.u
        keep = [True] * p if keep is None else list(keep)
        alive = [t["alive"] for t in self.tracks]
        r = [o if o >= 0 and keep[o] else -1 for o in owner.tolist()]
        t = []
        for c in cells.tolist():
            q = self.map.get(c, -1)
            t.append(q if q >= 0 and alive[q] else -1)
        a, b, n = [0] * p, [0] * T, [[0] * T for _ in range(p)]
        for ri, ti in zip(r, t):
            if ri >= 0:
                a[ri] += 1
            if ti >= 0:
                b[ti] += 1
            if ri >= 0 and ti >= 0:
                n[ri][ti] += 1

        def key(ri, ti, index):  # the larger IoU first, then the smaller index
            return (-Fraction(n[ri][ti], a[ri] + b[ti] - n[ri][ti]), index)

        def ok(ri, ti):
            return n[ri][ti] > 0 and (not self.same_class or int(cls[ri]) == self.tracks[ti]["cls"])

        best_row = [min((ti for ti in range(T) if ok(ri, ti)), key=lambda ti: key(ri, ti, ti), default=-1) for ri in range(p)]
        best_track = [min((ri for ri in range(p) if ok(ri, ti)), key=lambda ri: key(ri, ti, ri), default=-1) for ti in range(T)]
        track, row_of = [-1] * p, [-1] * T
        for ri in range(p):
            ti = best_row[ri]
            if ti >= 0 and best_track[ti] == ri and \
                    np.float64(n[ri][ti]) >= np.float64(self.iou) * np.float64(a[ri] + b[ti] - n[ri][ti]):
                track[ri], row_of[ti] = ti, ri
        new = []
        for ri in range(p):
            if track[ri] < 0 and keep[ri] and a[ri] >= self.min_points:
                track[ri] = T + len(new)
                new.append(track[ri])
                self.tracks.append(dict(cls=int(cls[ri]), score=np.float32(score[ri]), born=u, seen=u, hits=1, misses=0, size=0,
                                        alive=True))
        gone = set()
        for ti in range(T):
            tr = self.tracks[ti]
            if row_of[ti] >= 0:
                ri = row_of[ti]
                tr.update(hits=tr["hits"] + 1, misses=0, seen=u)
                if np.float32(score[ri]) >= tr["score"]:
                    tr.update(score=np.float32(score[ri]), cls=int(cls[ri]))
            elif tr["alive"] and b[ti] > 0:
                tr["misses"] += 1
                if tr["misses"] > self.max_misses:
                    tr.update(alive=False, size=0)
                    gone.add(ti)
        ids = []
        for c, ri, ti in zip(cells.tolist(), r, t):
            tid = track[ri] if ri >= 0 else -1
            if tid >= 0:
                now = tid
            elif ti >= 0 and (row_of[ti] >= 0 or ti in gone):
                now = -1
            else:
                now = ti
            if now != ti or tid >= 0:
                self.map[c] = now
            ids.append(now)
        for ti, tr in enumerate(self.tracks):  # size, counted afresh from the map
            if tr["alive"]:
                tr["size"] = sum(1 for q in self.map.values() if q == ti)
                if tr["size"] == 0:
                    tr["alive"] = False
                    gone.add(ti)
        self.u += 1
        return ids, track, [0 <= q < T for q in track], new, sorted(gone)

    def state(self, M):
        shown = [q if q >= 0 and self.tracks[q]["alive"] else -1 for q in (self.map.get(c, -1) for c in range(M))]
        return shown, {f: [tr[f] for tr in self.tracks] for f in frames.TrackTable._fields}


def _equals_dense(tracked, th, dense_out, dense):
    ids, track, matched, new, gone = dense_out
    got = [x.numpy().tolist() for x in tracked]
    assert got == [ids, track, matched, new, gone]
    shown, table = th.state()
    want_map, want = dense.state(th.cells)
    assert shown.tolist() == want_map
    for f, col in zip(frames.TrackTable._fields, table):
        assert col.tolist() == [float(v) if f == "score" else v for v in want[f]], f


@pytest.mark.parametrize("same_class", [False, True])
@pytest.mark.parametrize("seed", range(6))
def test_the_statement_equals_the_dense_restatement(seed, same_class):
    kw = dict(iou=0.3 if seed % 2 else 0.15, max_misses=seed % 3, min_points=1 + 3 * (seed % 2), same_class=same_class)
    th, dense = frames.TrackerHost(**kw), Dense(**kw)
    matches = 0
    for up in tc.random_sequence(seed):
        tracked = th.update(*up.args())
        _equals_dense(tracked, th, dense.update(*up.args()), dense)
        matches += int(tracked.matched.sum())
    assert matches > 0 and th.updates == 5 and th.tracks > th.live > 0


@pytest.mark.parametrize("name", ["partial_wave", "runs", "cross", "hold_and_retire", "empty_and_tiny"])
def test_the_device_sequences_equal_the_dense_restatement(name):
    kw = dict(max_misses=1) if name == "hold_and_retire" else {}
    th, dense = frames.TrackerHost(**kw), Dense(**kw)
    for up in tc.sequences()[name]:
        _equals_dense(th.update(*up.args()), th, dense.update(*up.args()), dense)


def test_the_same_labels_twice_and_permuted_rows_keep_every_id():
    th = frames.TrackerHost()
    up = tc.by_blocks(1005, 97)
    first = th.update(*up.args())
    assert first.new.tolist() == list(range(11)) and not first.matched.any() and first.track.tolist() == list(range(11))
    again = th.update(*up.args())
    assert again.matched.all() and again.new.numel() == 0 and torch.equal(again.ids, first.ids) and again.retired.numel() == 0
    perm = np.random.default_rng(1).permutation(11)
    inv = np.argsort(perm)
    third = th.update(up.cells, perm[up.owner].astype(np.int32), up.cls[inv], up.score[inv])
    assert torch.equal(third.ids, first.ids) and third.track.tolist() == inv.tolist() and third.matched.all()
    table = th.table()
    assert table.hits.tolist() == [3] * 11 and table.seen.tolist() == [2] * 11 and table.born.tolist() == [0] * 11
    assert table.size.tolist() == np.bincount(up.owner).tolist() and th.tracks == th.live == 11 and th.cells == 1005
    assert torch.equal(th.labels(up.cells), first.ids) and th.labels(np.array([[-1, 0]], np.int32)).tolist() == [[-1, 0]]


def test_a_scene_that_grows_keeps_ids_and_numbers_new_objects_next():
    th = frames.TrackerHost()
    th.update(*tc.by_blocks(200, 100).args())                     # objects 0 and 1
    grown = th.update(*tc.by_blocks(350, 100, seed=1).args())     # the same, a third, and the start of a fourth
    assert grown.track.tolist() == [0, 1, 2, 3] and grown.matched.tolist() == [True, True, False, False]
    assert grown.new.tolist() == [2, 3] and th.cells == 350
    # object 1 extended over new cells 200 .. 299 in place of object 2: the track's boundary is redrawn
    cells = np.arange(350)
    wider = th.update(*U(cells, np.where(cells < 100, 0, np.where(cells < 300, 1, 2)), *tc.rows(3)))
    assert wider.track.tolist() == [0, 1, 3] and wider.ids[250] == 1 and th.table().size.tolist() == [100, 200, 0, 50]
    assert wider.retired.tolist() == [2] and not th.table().alive[2] and th.live == 3


def test_a_split_keeps_the_id_on_exactly_one_side_and_ties_go_to_the_smaller_index():
    th = frames.TrackerHost()
    cells = np.arange(100)
    th.update(*U(cells, np.zeros(100), [1], [0.5]))
    halves = th.update(*U(cells, cells >= 50, [1, 1], [0.5, 0.5]))   # IoU 1/2 both: the smaller row
    assert halves.track.tolist() == [0, 1] and halves.matched.tolist() == [True, False] and halves.new.tolist() == [1]
    assert th.table().size.tolist() == [50, 50]
    # and in the other direction: one row over two tracks of equal IoU takes the smaller track; the other is missed and,
    # with every cell taken over, retires
    joined = th.update(*U(cells, np.zeros(100), [1], [0.5]))
    assert joined.track.tolist() == [0] and joined.retired.tolist() == [1] and (joined.ids == 0).all()
    uneven = frames.TrackerHost()
    uneven.update(*U(cells, np.zeros(100), [1], [0.5]))
    parts = uneven.update(*U(cells, cells >= 30, [1, 1], [0.5, 0.5]))
    assert parts.track.tolist() == [1, 0]   # the larger part (IoU 0.7) keeps the id


def test_hold_and_retire():
    th = frames.TrackerHost(max_misses=1)
    ups, out = tc.hold_and_retire(), []
    step = lambda: out.append(th.update(*ups[len(out)].args()))  # noqa: E731
    step()
    assert out[0].new.tolist() == [0, 1, 2]
    step()
    assert out[1].track.tolist() == [0, 2] and (out[1].ids[100:200] == 1).all()       # block 1 missed once: it holds its cells
    step()
    assert out[2].track.tolist() == [0, 1] and out[2].retired.tolist() == []         # ... and is seen again; block 2 missed once
    assert (out[2].ids[200:] == 2).all() and th.table().misses.tolist() == [0, 0, 1]
    step()
    assert out[3].retired.tolist() == [2] and (out[3].ids[200:] == -1).all()         # missed twice: retired, its cells read -1
    assert (th.labels(np.arange(200, 300, dtype=np.int32)) == -1).all() and th.table().size[2] == 0 and th.live == 2
    step()
    assert out[4].track.tolist() == [0, 1, 3] and out[4].new.tolist() == [3] and (out[4].ids[200:] == 3).all()   # never id 2 again
    assert th.tracks == 4 and th.table().alive.tolist() == [True, True, False, True]


def test_a_partial_update_leaves_the_rest_alone():
    th = frames.TrackerHost(max_misses=0)
    th.update(*tc.by_blocks(300, 100).args())
    before = th.state()
    part = th.update(np.arange(100, dtype=np.int32), np.full(100, -1, np.int32), np.zeros(0, np.int64), np.zeros(0, np.float32))
    assert part.retired.tolist() == [0] and (part.ids == -1).all()       # the region saw track 0 and nothing of it: retired at once
    shown, table = th.state()
    assert (shown[100:] == before[0][100:]).all() and (shown[:100] == -1).all()
    for f in ("hits", "misses", "seen", "size", "alive"):
        assert getattr(table, f)[1:].tolist() == getattr(before[1], f)[1:].tolist(), f


def test_min_points_and_keep():
    th = frames.TrackerHost(min_points=60)
    cells = np.arange(300)
    owner = np.where(cells < 100, 0, np.where(cells < 150, 1, 2)).astype(np.int32)     # 100, 50 and 150 points
    got = th.update(*U(cells, owner, [1, 2, 3], [0.9, 0.9, 0.9], [True, True, False]))
    assert got.track.tolist() == [0, -1, -1] and (got.ids[100:] == -1).all() and th.tracks == 1
    # the row that is not kept neither matches nor hides track 0's cells: its points count as unowned
    got = th.update(*U(cells, np.zeros(300), [1], [0.5], [False]))
    assert got.track.tolist() == [-1] and (got.ids[:100] == 0).all() and th.table().misses.tolist() == [1]


def test_score_and_class_follow_the_best_sighting():
    th = frames.TrackerHost()
    cells = np.arange(50, dtype=np.int32)
    for cls, score in ((1, 0.5), (2, 0.75), (3, 0.25), (4, 0.75)):
        th.update(*U(cells, np.zeros(50), [cls], [score]))
    assert th.table().cls.tolist() == [4] and th.table().score.tolist() == [0.75] and th.table().hits.tolist() == [4]
    same = frames.TrackerHost(same_class=True)
    same.update(*U(cells, np.zeros(50), [1], [0.5]))
    assert same.update(*U(cells, np.zeros(50), [2], [0.5])).new.tolist() == [1]   # another class: no match


def test_every_error_leaves_the_state_as_it_was():
    th = frames.TrackerHost()
    up = tc.by_blocks(300, 100)
    th.update(*up.args())
    before, counters = th.state(), tc.counters(th)
    i32, f32 = np.int32, np.float32
    bad = [
        (up.cells[::-1].copy(), up.owner, up.cls, up.score),                      # descending
        (np.array([3, 3], i32), np.zeros(2, i32), np.ones(1, i32), f32([1])),                 # not strictly ascending
        (np.array([-1, 3], i32), np.zeros(2, i32), np.ones(1, i32), f32([1])),                # negative
        (up.cells, np.full(300, 3, i32), up.cls, up.score),                       # owner == p
        (up.cells, np.full(300, -2, i32), up.cls, up.score),                      # owner < -1
        (up.cells, up.owner[:-1], up.cls, up.score),                              # lengths
        (up.cells.astype(np.int64), up.owner, up.cls, up.score),                  # dtypes
        (up.cells, up.owner, up.cls.astype(np.float32), up.score),
        (up.cells, up.owner, up.cls, up.score.astype(np.float64)),
        (up.cells, up.owner, up.cls, up.score[:-1]),
        (up.cells, up.owner, up.cls, up.score, np.ones(3, np.uint8)),             # keep must be bool
        (up.cells, up.owner, np.zeros(tc.MAX_ROWS + 1, i32), np.zeros(tc.MAX_ROWS + 1, f32)),
        (up.cells, up.owner, np.array([2 ** 40, 0, 0]), up.score),
    ]
    for args in bad:
        with pytest.raises(ValueError):
            th.update(*args)
        assert tc.same_state(th.state(), before) and tc.counters(th) == counters
    with pytest.raises(ValueError):
        th.labels(np.array([300], np.int32))
    for kw in (dict(iou=1.5), dict(iou=-0.1), dict(max_misses=-1), dict(min_points=0), dict(max_misses=0.5)):
        with pytest.raises(ValueError):
            frames.TrackerHost(**kw)
    assert tc.same_tracked(frames.TrackerHost().update(*up.args()), frames.Tracker(device="cpu").update(*up.args()))


def test_cpu_tracker_is_the_statement_and_slots():
    t = frames.Tracker(device="cpu", iou=0.5, max_misses=1)
    assert isinstance(t._host, frames.TrackerHost) and t.updates == 0 and t.tracks == 0 and t.cells == 0 and t.live == 0
    assert frames.tracker_slots(0, 0, 0) == (64, 64) and frames.tracker_slots(50, 50, 113000) == (1024, 262144)
    assert frames.tracker_slots(4096, 0, 4096) == (32768, 8192)
    assert frames.TRACK_AGGREGATE in (True, False)


@pytest.mark.parametrize("split", sorted(tc.SPLITS))
def test_a_streamed_run_keeps_the_ids_of_the_blocks(split):
    """lift_scene_stream renumbers its instances densely per snapshot; the track ids must not change.  The tracker runs at
    iou = 0: between two snapshots of this input an object grows by any factor (a block of 3 cells after the first frame has
    62 after the fourth), its IoU with itself is at most 1 / that factor, so no positive threshold is safe here; at 0 the
    rule is the mutual best alone, which is what carries the identity."""
    fz = frames.FuserHost(0.05)
    sem_v, ins_v = frames.VoterHost(0), frames.VoterHost(0)
    sem_img, ins_img = tc.dense4_block_images()
    th = frames.TrackerHost(iou=0.0)
    at, seen, raw_ids = 0, None, []
    for part in sc.chunks(sc.dense4(), tc.SPLITS[split]):
        F = part.depth.shape[0]
        cells = fz.add(part)
        sem_v.add(cells, sem_img[at:at + F])
        ins_v.add(cells, ins_img[at:at + F])
        at += F
        kept = fz.kept(1)
        sem, inst = (x.numpy() for x in frames.lift_scene_stream(fz, sem_v, ins_v))
        block = ins_v.snapshot(fz.cells, rows=kept)[0].label.numpy()     # the block of every cell, as voted
        p = int(inst.max()) + 1
        first = np.array([np.nonzero(inst == r)[0][0] for r in range(p)])
        assert (block[inst < 0] < 0).all() and len(set(block[first].tolist())) == p     # one row per block
        turn = (np.arange(p) + len(raw_ids)) % p                        # ... and the rows are rotated by the snapshot's number
        inst, first = np.where(inst >= 0, turn[np.maximum(inst, 0)], -1), first[np.argsort(turn)]
        got = th.update(kept, inst.astype(np.int32), sem[first], np.ones(p, np.float32))
        ids = got.ids.numpy()
        raw_ids.append(dict(zip(block[first].tolist(), range(p))))
        now = dict(zip(kept.numpy().tolist(), zip(block.tolist(), ids.tolist())))
        if seen is not None:
            both = [c for c in now if c in seen and seen[c][0] == now[c][0] and now[c][0] >= 0]
            assert len(both) > 500 and all(seen[c][1] == now[c][1] for c in both)
        seen = now
    pairs = {(b, t) for b, t in seen.values() if b >= 0}
    assert len({b for b, _ in pairs}) == len({t for _, t in pairs}) == len(pairs) > 5      # one to one at the end
    if len(raw_ids) > 1:   # (the raw numbers did change: the check above is not empty)
        assert any(raw_ids[0][b] != raw_ids[-1][b] for b in raw_ids[0] if b in raw_ids[-1])
