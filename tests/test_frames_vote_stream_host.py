"""frames.VoterHost, the numpy statement of the persistent vote: against vote_host of the concatenation (contract A),
against a plain Python loop, and with FuserHost against lift / lift_scene_host of the whole input (contract B).  The
inputs and what each size straddles are named in tests/frames_vote_stream_cases.py."""
import numpy as np
import pytest
import torch

from geoformer_amd import frames
from tests import frames_lift_cases as lc
from tests import frames_stream_cases as sc
from tests import frames_vote_stream_cases as vc


def _feed(adds, ignore=None, stride=None, make=frames.VoterHost):
    v = make(ignore)
    for g, x in adds:
        v.add(g, x, stride)
    return v


def _contract_a(adds, n, ignore=None, fill=-100, stride=None):
    """snapshot == vote_host of the concatenation, in every field and in pairs; the voter is returned."""
    v = _feed(adds, ignore, stride)
    group = np.concatenate([np.asarray(g).reshape(-1) for g, _ in adds])
    value = np.concatenate([vc.sampled(x, stride).reshape(-1).astype(np.int32) if np.asarray(x).ndim == 3
                            else np.asarray(x).reshape(-1).astype(np.int32) for _, x in adds])
    want, want_pairs = frames.vote_host(group, value, n, ignore, fill)
    got, pairs = v.snapshot(n, fill)
    assert vc.same_lifted(got, want) and pairs == want_pairs == v.pairs
    assert v.elements == group.size
    return v, group, value, want


@pytest.mark.parametrize("which", ["semantic", "instance"])
@pytest.mark.parametrize("ignore", [None, vc.IGNORE])
@pytest.mark.parametrize("split", sorted(vc.SPLITS))
@pytest.mark.parametrize("cell", [0.1, 0.02])
def test_dense_frames_equal_the_vote_of_the_concatenation(cell, split, ignore, which):
    cells, fz = vc.dense4_cells(cell)
    image = lc.images("dense", 4)[which == "instance"]
    assert image.dtype == (np.uint16 if which == "instance" else np.uint8)
    v, group, value, want = _contract_a(vc.frame_adds(cells, image, vc.SPLITS[split]), fz.cells, ignore)
    label, votes, total, pairs = lc.counter_vote(group, value, fz.cells, ignore)
    assert pairs == v.pairs and all(np.array_equal(a.numpy(), b) for a, b in zip(want, (label, votes, total)))
    keys, count = v.state()
    assert keys.dtype == count.dtype == np.int64 and (np.diff(keys) > 0).all() and count.sum() == want.total.sum()


def test_the_coarse_case_makes_a_second_add_meet_its_own_keys():
    cells, fz = vc.dense4_cells(0.1)
    sem = lc.images("dense", 4)[0]
    adds = vc.frame_adds(cells, sem, vc.SPLITS["4x1"])
    per_chunk = np.concatenate([_feed([a], vc.IGNORE).state()[0] for a in adds])
    _, times = np.unique(per_chunk, return_counts=True)
    v = _feed(adds, vc.IGNORE)
    _, heard = np.unique(v.state()[0] >> 32, return_counts=True)
    kept = fz.kept(3)
    # (on the statement: 464 of the 1358 pairs occur in more than one chunk, 25 cells hear more than one class, and
    # min_obs = 3 keeps 1027 of 1333 cells)
    assert v.pairs == vc.DENSE4_PAIRS_10CM and (times > 1).sum() > 100
    assert (heard > 1).sum() >= 1
    assert 0 < kept.numel() < fz.cells
    assert kept.dtype == torch.int32 and torch.equal(kept, torch.nonzero(torch.from_numpy(fz.state()[1]) >= 3).reshape(-1).int())
    with pytest.raises(ValueError, match="min_obs"):
        fz.kept(0)


@pytest.mark.parametrize("min_obs", [1, 3])
def test_with_a_fuser_equals_lift_of_the_whole_input(min_obs):
    cells, fz = vc.dense4_cells(0.1)
    sem, ins = lc.images("dense", 4)
    fused = fz.snapshot(min_obs, cells)
    for image, ignore, fill in ((sem, vc.IGNORE, -100), (ins, vc.IGNORE, -7), (sem, None, -100)):
        v = _feed(vc.frame_adds(cells, image, vc.SPLITS["1+3"]), ignore)
        got = v.snapshot(fz.cells, fill, rows=fz.kept(min_obs))[0]
        assert vc.same_lifted(got, frames.lift(fused, image, ignore, fill))
        assert got.label.shape[0] == fused.xyz.shape[0]


@pytest.mark.parametrize("kw", [{}, {"min_votes": 3, "min_share": 0.9}, {"min_obs": 3}])
def test_lift_scene_stream_equals_lift_scene_host(kw):
    cells, fz = vc.dense4_cells(0.1)
    pair = lc.images("dense", 4)
    voters = [_feed(vc.frame_adds(cells, image, vc.SPLITS["2+2"]), vc.IGNORE) for image in pair]
    got = frames.lift_scene_stream(fz, *voters, **kw)
    scene_kw = {k: v for k, v in kw.items() if k != "min_obs"}
    want = frames.lift_scene_host(fz.snapshot(kw.get("min_obs", 1), cells), *pair, ignore=vc.IGNORE, **scene_kw)
    for x, w in zip(got, want):
        assert x.dtype == torch.int32 and torch.equal(x, w)
    assert int(want[1].max()) >= 0 and bool((want[1] == -100).any())
    # scene_labels is that tail, on any two Lifted of one shape
    fused = fz.snapshot(kw.get("min_obs", 1), cells)
    sem, ins = (frames.lift(fused, image, vc.IGNORE) for image in pair)
    again = frames.scene_labels(sem, ins, host=True, **scene_kw)
    assert all(torch.equal(x, w) for x, w in zip(again, want))
    with pytest.raises(ValueError, match="differ in shape"):
        frames.scene_labels(sem, frames.Lifted(*(t[:-1] for t in ins)))


@pytest.mark.parametrize("stride", [2, 3])
def test_full_resolution_images_at_a_stride(stride):
    cells, fz = vc.dense4_cells(0.1, stride)
    sem, ins = lc.images("dense", 4)
    assert cells.shape[1:] == (-(-sem.shape[1] // stride), -(-sem.shape[2] // stride))
    for image in (sem, ins):
        v, _, _, want = _contract_a(vc.frame_adds(cells, image, vc.SPLITS["1+3"]), fz.cells, vc.IGNORE, stride=stride)
        assert (want.total.numpy() > 0).sum() > 50
        assert vc.same_lifted(v.snapshot(fz.cells, rows=fz.kept(1))[0], frames.lift(fz.snapshot(1, cells), image, vc.IGNORE,
                                                                                   stride=stride))
    # narrow: 67 x 5 is no multiple of either stride
    cells, fz = vc.narrow3_cells(stride)
    _contract_a(vc.frame_adds(cells, lc.images("narrow")[0], (1, 1, 1)), fz.cells, None, stride=stride)
    with pytest.raises(ValueError, match="does not sample"):
        frames.VoterHost().add(cells, lc.images("narrow")[0], stride + 2)


def test_a_winner_that_changes_between_snapshots():
    v = frames.VoterHost()
    seen = []
    for g, x in vc.changing_winner():
        v.add(g, x)
        got, pairs = v.snapshot(1)
        seen.append((got.label.tolist(), got.votes.tolist(), got.total.tolist(), pairs))
    assert seen == [([2], [3], [3], 1), ([1], [4], [7], 2), ([1], [4], [8], 2)]  # the last: 4 : 4, the smaller value


def test_rows_select_and_order_the_groups():
    group, value = lc.random_votes()
    v = _feed(vc.cut(group, value, (100, 350)))
    full, pairs = v.snapshot(37, -9)
    state = v.state()
    perm = np.random.default_rng(0).permutation(37).astype(np.int32)[:20]
    got, p = v.snapshot(37, -9, rows=perm)
    assert p == pairs and all(torch.equal(a, b[perm.astype(np.int64)]) for a, b in zip(got, full))
    got, _ = v.snapshot(37, rows=np.zeros(0, np.int32))
    assert all(a.shape == (0,) and a.dtype == torch.int32 for a in got)
    got, _ = v.snapshot(37, -9, rows=torch.tensor([5, 5, 5], dtype=torch.int32))
    assert got.label.tolist() == [int(full.label[5])] * 3
    for bad in ([0, 37], [-1], [2 ** 31 - 1]):
        with pytest.raises(ValueError, match="rows holds"):
            v.snapshot(37, rows=np.array(bad, np.int32))
    for bad in (np.zeros(3, np.int64), np.zeros((2, 2), np.int32)):
        with pytest.raises(ValueError, match="rows: expected int32"):
            v.snapshot(37, rows=bad)
    assert all(np.array_equal(a, b) for a, b in zip(v.state(), state))  # a snapshot changes nothing


def test_a_stored_group_beyond_n_is_a_value_error():
    group, value = lc.random_votes()
    v = _feed([(group, value)])
    top = int(np.asarray(group)[np.asarray(value) >= 0].max())
    v.snapshot(top + 1)
    with pytest.raises(ValueError, match=f"outside the {top} groups"):
        v.snapshot(top)
    with pytest.raises(ValueError, match="outside the 0 groups"):
        v.snapshot(0)
    assert frames.VoterHost().snapshot(0)[0].label.shape == (0,)
    big = frames.VoterHost()
    big.add(np.array([2 ** 31 - 2], np.int32), np.array([2 ** 31 - 1], np.int32))  # no upper bound at add
    assert big.state()[0].tolist() == [((2 ** 31 - 2) << 32) | (2 ** 31 - 1)]
    with pytest.raises(ValueError, match="groups"):
        big.snapshot(2 ** 31)


def test_the_element_budget_and_other_failed_adds_leave_no_trace(monkeypatch):
    group, value = lc.random_votes()
    v = _feed(vc.cut(group, value, (300,))[:1])
    state, elements = v.state(), v.elements
    assert elements == 300
    monkeypatch.setattr(frames, "VOTER_MAX_ELEMENTS", 500)
    with pytest.raises(ValueError, match="at most 500"):
        v.add(group[:201], value[:201])  # counted as offered, not as voting
    v.add(group[:200], value[:200])
    assert v.elements == 500
    monkeypatch.undo()
    v = _feed(vc.cut(group, value, (300,))[:1])
    monkeypatch.setattr(frames, "MAX_POINTS", 100)
    with pytest.raises(ValueError, match="in one add"):
        v.add(group[:101], value[:101])
    monkeypatch.undo()
    for g, x, s, match in ((group[:5], value[:4], None, "differ in shape"), (group[:5].astype(np.int64), value[:5], None, "int32"),
                           (group[:5], value[:5].astype(np.int64), None, "uint8, uint16 or int32"),
                           (group[:5], value[:5], 0, "stride"), (group[:6], value[:6], 2, "does not sample"),
                           ([0], [1], None, "numpy arrays or torch tensors")):
        with pytest.raises(ValueError, match=match):
            v.add(g, x, s)
    assert v.elements == elements and all(np.array_equal(a, b) for a, b in zip(v.state(), state))
    with pytest.raises(ValueError, match="ignore"):
        frames.VoterHost(0.5)


def test_mixed_dtypes_nothing_votes_and_an_empty_add():
    group, value = (np.array(a) for a in lc.random_votes())
    parts = vc.cut(group, np.where(value < 0, 3, value).astype(np.int32), (150, 400))
    mixed = [(parts[0][0], parts[0][1].astype(np.uint8)), (parts[1][0], parts[1][1].astype(np.uint16)), parts[2]]
    a, b = _feed(mixed, 1), _feed(parts, 1)
    assert vc.same_state(a, b) and a.pairs > 50
    _contract_a(parts, 37, 1)
    # nothing votes: every value ignored, no valid group
    v, _, _, want = _contract_a([(group, np.full_like(value, 4))], 37, ignore=4, fill=-9)
    assert v.pairs == 0 and v.elements == group.size and (want.label.numpy() == -9).all()
    v, _, _, _ = _contract_a([(np.full_like(group, -1), value)], 37)
    assert v.pairs == 0
    # an empty add, in both forms
    e = np.zeros(0, np.int32)
    v = _feed([parts[0], (e, e), (np.zeros((0, 3, 4), np.int32), np.zeros((0, 6, 8), np.uint8))][:2], 1)
    v.add(np.zeros((0, 3, 4), np.int32), np.zeros((0, 6, 8), np.uint8), 2)
    assert vc.same_state(v, _feed(parts[:1], 1)) and v.elements == 150
    got, pairs = frames.VoterHost().snapshot(5)
    assert got.label.tolist() == [-100] * 5 and got.votes.tolist() == [0] * 5 and got.total.tolist() == [0] * 5 and pairs == 0


def test_the_cpu_device_is_the_statement():
    v = frames.Voter(ignore=1, device="cpu")
    group, value = lc.random_votes()
    v.add(group, value)
    assert v.slots is None and v.rehashes == 0 and v.retries == 0
    assert vc.same_state(v, _feed([(group, value)], 1)) and v.pairs == v.snapshot(37)[1] and v.elements == 600
    assert frames.voter_slots(0, 0) == (64, 64) and frames.voter_slots(100, 4800) == (1024, 16384)
    assert frames.voter_slots(0, vc.MANY_VALUES) == (128, 2048) and frames.voter_slots(1 << 30, 0)[0] == frames.VOTER_MAX_SLOTS
    fz = frames.Fuser(0.1, device="cpu")
    fz.add(sc.sub(sc.dense4(), 0, 1))
    assert torch.equal(fz.kept(2), fz._host.kept(2)) and 0 < fz.kept(2).numel() < fz.cells
