"""frames.vote_host / lift / lift_scene_host without a GPU: the numpy statement of csrc/frames_vote.hip against a plain
Python Counter loop, its order-freedom, the full-resolution form, the round trip through fuse_host, and the dataset-style
labels of lift_scene_host."""
import numpy as np
import pytest
import torch

from geoformer_amd import evaluation, frames
from tests import frames_cases as fc
from tests import frames_lift_cases as lc


def _np(lifted):
    return tuple(a.numpy() for a in lifted)


def _same(lifted, want):
    for x, w in zip(_np(lifted), want):
        assert x.dtype == np.int32 and np.array_equal(x, w)


def test_vote_host_against_a_counter_loop():
    group, value = lc.random_votes()
    n = 37
    assert (group < 0).any() and (value < 0).any() and group.max() == n - 1
    for ignore in (None, 2):
        got, pairs = frames.vote_host(group, value, n, ignore)
        *want, want_pairs = lc.counter_vote(group, value, n, ignore)
        _same(got, want)
        assert pairs == want_pairs and 0 < pairs <= n * 5
    assert (got.total.numpy() > got.votes.numpy()).any()  # (some group does hold several values)
    # any shape, tensors or arrays
    again, _ = frames.vote_host(torch.from_numpy(np.array(group)).reshape(20, 30), np.array(value).reshape(20, 30), n, 2)
    _same(again, want)


def test_ties_go_to_the_smallest_value():
    group = np.array([0, 0, 0, 0, 1, 1, 1, 2], np.int32)
    value = np.array([9, 3, 9, 3, 7, 2, 2, 2 ** 31 - 1], np.int32)
    got, pairs = frames.vote_host(group, value, 4)
    assert got.label.tolist() == [3, 2, 2 ** 31 - 1, -100] and got.votes.tolist() == [2, 2, 1, 0]
    assert got.total.tolist() == [4, 3, 1, 0] and pairs == 5
    assert frames.vote_host(group, value, 4, fill=-7)[0].label.tolist()[3] == -7


def test_bit_identical_under_a_permutation():
    group, value = lc.random_votes()
    a, pa = frames.vote_host(group, value, 37, 1)
    perm = np.random.default_rng(0).permutation(group.size)
    b, pb = frames.vote_host(group[perm], value[perm], 37, 1)
    _same(a, _np(b))
    assert pa == pb


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.int32])
def test_ignore_for_each_dtype(dtype):
    group = np.array([0, 0, 0, 1, 1, 2], np.int32)
    value = np.array([0, 0, 4, 0, 0, 3], dtype)
    off, _ = frames.vote_host(group, value, 3)
    assert off.label.tolist() == [0, 0, 3] and off.total.tolist() == [3, 2, 1]
    on, pairs = frames.vote_host(group, value, 3, ignore=0)
    assert on.label.tolist() == [4, -100, 3] and on.votes.tolist() == [1, 0, 1] and on.total.tolist() == [1, 0, 1]
    assert pairs == 2
    # all votes ignored: fill, 0, 0
    none, pairs = frames.vote_host(group, np.zeros(6, dtype), 3, ignore=0, fill=-1)
    assert none.label.tolist() == [-1] * 3 and not none.votes.any() and not none.total.any() and pairs == 0
    # an ignore no value can hold changes nothing
    _same(frames.vote_host(group, value, 3, ignore=-5)[0], _np(off))


def test_empty_inputs_and_errors():
    e = np.zeros(0, np.int32)
    got, pairs = frames.vote_host(e, e, 5)
    assert got.label.tolist() == [-100] * 5 and got.votes.tolist() == [0] * 5 and pairs == 0
    got, pairs = frames.vote_host(e, e, 0)
    assert all(a.shape == (0,) and a.dtype == torch.int32 for a in got) and pairs == 0
    got, _ = frames.vote_host(np.array([-1, -1], np.int32), np.array([3, 3], np.int32), 0)  # no vote: no group needed
    assert got.label.shape == (0,)
    with pytest.raises(ValueError, match="outside"):
        frames.vote_host(np.array([0, 5], np.int32), np.array([1, 1], np.int32), 5)
    with pytest.raises(ValueError):
        frames.vote_host(np.array([0], np.int32), np.array([1], np.int32), 0)
    with pytest.raises(ValueError):
        frames.vote_host(np.array([0], np.int64), np.array([1], np.int32), 1)   # group dtype
    with pytest.raises(ValueError):
        frames.vote_host(np.array([0], np.int32), np.array([1], np.int64), 1)   # value dtype
    with pytest.raises(ValueError):
        frames.vote_host(np.array([0, 0], np.int32), np.array([1], np.int32), 1)  # shapes
    with pytest.raises(ValueError):
        frames.vote_host(np.array([0], np.int32), np.array([1], np.int32), 1, ignore=0.5)
    # CPU tensors through the wrapper run the statement
    group, value = lc.random_votes()
    a, pa = frames.vote(torch.from_numpy(np.array(group)), torch.from_numpy(np.array(value)), 37)
    _same(a, _np(frames.vote_host(group, value, 37)[0]))
    assert frames.vote_slots(1000, 1) == (64, 2048) and frames.vote_slots(19660800, 113305) == (1 << 21, 1 << 26)
    assert frames.vote_slots(0, 0) == (64, 64) and frames.vote_slots(33, 1000) == (128, 128)


@pytest.fixture(scope="module")
def fused_full():
    return frames.fuse_host(fc.make(fc.dense(), "u16"), 0.05)


@pytest.mark.parametrize("stride", [2, 3])
def test_full_resolution_form_equals_slicing_first(stride):
    fr = fc.make(fc.dense(), "u16")
    fused = frames.fuse_host(fr, 0.05, stride)
    sem, ins = lc.images("dense")
    for img in (sem, ins, np.array(ins).astype(np.int32)):
        full = frames.lift(fused, img, ignore=lc.IGNORE, stride=stride)
        sliced = frames.lift(fused, np.ascontiguousarray(img[:, ::stride, ::stride]), ignore=lc.IGNORE)
        want, _ = frames.vote_host(fused.point_of, np.ascontiguousarray(img[:, ::stride, ::stride]), fused.xyz.shape[0], lc.IGNORE)
        _same(full, _np(sliced))
        _same(full, _np(want))
        assert (full.total.numpy() > 0).any()
    with pytest.raises(ValueError, match="sample"):
        frames.lift(fused, sem, stride=stride + 2)
    with pytest.raises(ValueError, match="sample"):
        frames.lift(fused, sem)  # full resolution without the stride
    with pytest.raises(ValueError):
        frames.lift(fused, sem, stride=0)


def test_round_trip_a_point_of_one_instance_carries_it():
    """fc.round_trip() is rendered at radius 0: a pixel holds exactly one source point, so its label is that point's."""
    case = fc.round_trip()
    fused = frames.fuse_host(fc.make(case, "f32"), 0.05)
    n = fused.xyz.shape[0]
    _, ins = lc.block_images("round_trip")
    lifted = frames.lift(fused, ins, ignore=lc.IGNORE)
    label, votes, total = _np(lifted)
    p = fused.point_of.numpy().reshape(-1)
    v = ins.reshape(-1)
    on = p >= 0
    lo = np.full(n, 2 ** 31 - 1, np.int64)
    hi = np.full(n, -1, np.int64)
    voting = on & (v != lc.IGNORE)
    np.minimum.at(lo, p[voting], v[voting])
    np.maximum.at(hi, p[voting], v[voting])
    one = lo == hi                       # every voting pixel of the point comes from one source instance
    assert one.sum() > 100 and (hi >= 0).sum() > one.sum()
    assert (label[one] == lo[one]).all() and (votes[one] == total[one]).all()
    assert (label[hi < 0] == -100).all() and (total[hi < 0] == 0).all()
    ignored = np.zeros(n, np.int64)
    np.add.at(ignored, p[on & ~voting], 1)
    clean = ignored == 0
    assert clean.any() and (~clean).any()
    assert (total[clean] == fused.count.numpy()[clean]).all()
    assert (total + ignored == fused.count.numpy()).all()


def test_lift_scene_host_gives_dataset_style_labels(fused_full):
    sem_img, ins_img = lc.block_images("dense")
    n = fused_full.xyz.shape[0]
    sem, inst = (a.numpy() for a in frames.lift_scene_host(fused_full, sem_img, ins_img, ignore=lc.IGNORE))
    assert sem.dtype == inst.dtype == np.int32 and sem.shape == inst.shape == (n,)
    own_sem = frames.lift(fused_full, sem_img, ignore=lc.IGNORE).label.numpy()
    own_ins = frames.lift(fused_full, ins_img, ignore=lc.IGNORE).where().numpy()
    on = inst >= 0
    I = int(inst.max()) + 1
    assert I > 5 and np.array_equal(np.unique(inst[on]), np.arange(I)) and (inst[~on] == -100).all()
    assert np.array_equal(on, own_ins >= 0)
    # ascending in the original id: the original id is a strictly increasing function of the new one
    orig = np.full(I, -1, np.int64)
    orig[inst[on]] = own_ins[on]
    assert (orig[inst[on]] == own_ins[on]).all() and (np.diff(orig) > 0).all()
    # every instance has one class, the mode of its members' lifted classes (ties to the smallest)
    mode, _, _, _ = lc.counter_vote(inst, own_sem, I)
    assert (sem[on] == mode[inst[on]]).all()
    assert (own_sem[on] != sem[on]).any()  # (some member did say another class)
    assert np.array_equal(sem[~on], own_sem[~on])
    # gt_ids_from_labels does not depend on which point comes first
    gt = evaluation.gt_ids_from_labels(sem, inst)
    perm = np.random.default_rng(1).permutation(n)
    assert np.array_equal(evaluation.gt_ids_from_labels(sem[perm], inst[perm]), gt[perm])
    assert len(np.unique(gt)) == I + 1
    # thresholds: stricter ones drop points, and the instances stay dense
    s2, i2 = (a.numpy() for a in frames.lift_scene_host(fused_full, sem_img, ins_img, ignore=lc.IGNORE, min_votes=3, min_share=0.9))
    keep = frames.lift(fused_full, ins_img, ignore=lc.IGNORE).where(3, 0.9).numpy() >= 0
    assert 0 < keep.sum() < on.sum() and np.array_equal(i2 >= 0, keep)
    assert np.array_equal(np.unique(i2[keep]), np.arange(int(i2.max()) + 1))
    # no instance at all
    s0, i0 = frames.lift_scene_host(fused_full, sem_img, np.zeros_like(ins_img), ignore=lc.IGNORE)
    assert (i0 == -100).all() and np.array_equal(s0.numpy(), own_sem)


def test_raw_scene_with_and_without_labels(fused_full):
    n = fused_full.xyz.shape[0]
    raw, shift = fused_full.raw_scene()
    assert raw.shape == (n, 8) and (raw[:, 6:] == -100).all()
    sem, inst = frames.lift_scene_host(fused_full, *lc.images("dense"), ignore=lc.IGNORE)
    lab, shift2 = fused_full.raw_scene(semantic=sem, instance=inst.numpy())
    assert np.array_equal(lab[:, :6], raw[:, :6]) and np.array_equal(shift, shift2)
    assert np.array_equal(lab[:, 6], sem.numpy()) and np.array_equal(lab[:, 7], inst.numpy())
    assert set(np.unique(lab[:, 7])) == {-100.0, 0.0} and {1.0, 2.0, 5.0} <= set(np.unique(lab[:, 6]))
    only, _ = fused_full.raw_scene(center=False, instance=inst)
    assert (only[:, 6] == -100).all() and np.array_equal(only[:, 7], inst.numpy())
    with pytest.raises(ValueError):
        fused_full.raw_scene(semantic=sem[:-1])
    with pytest.raises(ValueError):
        fused_full.raw_scene(semantic=sem.double())


def test_lifted_where_thresholds():
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)  # noqa: E731
    lifted = frames.Lifted(i32(4, 5, 6, -100, 7), i32(1, 2, 3, 0, 6), i32(1, 4, 4, 0, 10))
    assert lifted.where().tolist() == [4, 5, 6, -100, 7]
    assert lifted.where(min_votes=2).tolist() == [-100, 5, 6, -100, 7]
    assert lifted.where(min_share=0.5).tolist() == [4, 5, 6, -100, 7]      # 2 >= 0.5 * 4: kept
    assert lifted.where(min_share=0.6).tolist() == [4, -100, 6, -100, 7]   # 2 < 2.4, 3 >= 2.4, 6 >= 6.0
    assert lifted.where(min_votes=3, min_share=0.7, fill=-1).tolist() == [-1, -1, 6, -1, -1]
    assert lifted.where(min_votes=0).tolist() == [4, 5, 6, -100, 7] and lifted.where().dtype == torch.int32
