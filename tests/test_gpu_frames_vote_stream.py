"""csrc/frames_vote_stream.hip on the GPU: frames.Voter bit for bit against frames.VoterHost -- state() after EVERY add, a
snapshot's three fields and its pairs -- each sequence from a fresh Voter twice with the lane-run aggregation and once
without it.  The inputs and what each size straddles are named in tests/frames_vote_stream_cases.py."""
import numpy as np
import pytest
import torch

from geoformer_amd import frames
from tests import frames_cases as fc
from tests import frames_lift_cases as lc
from tests import frames_stream_cases as sc
from tests import frames_vote_stream_cases as vc

pytestmark = pytest.mark.gpu


def _same_state(got, want):
    return all(x.dtype == y.dtype and x.shape == y.shape and (x == y).all() for x, y in zip(got, want))


def _dev(a):
    return a.cuda() if torch.is_tensor(a) else a


def _check(adds, n, ignore=None, fill=-100, stride=None, rows=None, on_device=True, **dev_kw):
    """The three device runs of a sequence of adds against the statement, after every add; returns (the VoterHost, the
    three Voters).  on_device: the groups are handed over as CUDA tensors (what Fuser.add returns); the values always come
    from the host."""
    vh, want = frames.VoterHost(ignore), []
    for g, x in adds:
        vh.add(g, x, stride)
        want.append((vh.state(), vh.snapshot(n, fill, rows), vh.elements))
    voters = []
    for aggregate in (True, None, False):
        v = frames.Voter(ignore, aggregate=aggregate, **dev_kw)
        for (g, x), (state_w, (snap_w, pairs_w), elements_w) in zip(adds, want):
            assert v.add(_dev(g) if on_device else g, x, stride) is None
            assert _same_state(v.state(), state_w)
            got, pairs = v.snapshot(n, fill, rows)
            assert all(t.is_cuda for t in got) and vc.same_lifted(got, snap_w)
            assert pairs == pairs_w == v.pairs and v.elements == elements_w
        voters.append(v)
    return vh, voters


def test_limits_are_the_modules(hip):
    from geoformer_amd import _lib

    lib = _lib.load()
    assert frames.voter_limits() == (vc.MAX_PROBES, 2 ** 31 - 1) == (frames.VOTER_MAX_PROBES, frames.VOTER_MAX_ELEMENTS)
    for P, T in ((0, 0), (0, 1), (0, 4800), (1358, 4800), (7240, 0), (1, 1 << 29), (1 << 20, 100), (3, 511), (3, 513), (16, 512),
                 (40, vc.MANY_VALUES), (1 << 30, 0), (2 ** 31 - 1, 2 ** 31 - 1)):
        assert lib.gf_frames_votes_default_slots(P, T) == frames.voter_slots(P, T)[0], (P, T)
    assert lib.gf_frames_votes_default_slots(-1, 0) == 0 and lib.gf_frames_votes_default_slots(0, 1 << 31) == 0
    assert lib.gf_frames_votes_add_scratch_bytes(1000) >= 8000 and lib.gf_frames_votes_add_scratch_bytes((1 << 29) + 1) == 0
    assert lib.gf_frames_votes_add_scratch_bytes(-1) == 0 and lib.gf_frames_votes_pick_scratch_bytes(-1) == 0
    assert lib.gf_frames_votes_pick_scratch_bytes(10) >= 120 and lib.gf_frames_votes_pick_scratch_bytes(1 << 31) == 0


@pytest.mark.parametrize("which", ["semantic", "instance"])
@pytest.mark.parametrize("ignore", [None, vc.IGNORE])
@pytest.mark.parametrize("split", sorted(vc.SPLITS))
@pytest.mark.parametrize("cell", [0.1, 0.02])
def test_dense_frames_in_chunks(hip, cell, split, ignore, which):
    cells, fz = vc.dense4_cells(cell)
    image = lc.images("dense", 4)[which == "instance"]
    vh, voters = _check(vc.frame_adds(cells, image, vc.SPLITS[split]), fz.cells, ignore)
    want, pairs = frames.vote_host(cells, image, fz.cells, ignore)
    # (the fewest pairs: the instance images with ignore at 10 cm, 418 on the statement)
    assert vc.same_lifted(voters[0].snapshot(fz.cells)[0], want) and vh.pairs == pairs > 100
    assert all(4 * v.pairs <= v.slots for v in voters)


@pytest.mark.parametrize("min_obs", [1, 3])
def test_with_a_fuser_equals_lift_of_the_whole_input(hip, min_obs):
    fr = sc.dense4()
    sem, ins = lc.images("dense", 4)
    fu, fz = frames.Fuser(0.1), vc.dense4_cells(0.1)[1]
    voters = frames.Voter(vc.IGNORE), frames.Voter(vc.IGNORE)
    cells, at = [], 0
    for part in sc.chunks(fr, vc.SPLITS["1+3"]):
        F = part.depth.shape[0]
        cells.append(fu.add(part))
        for v, image in zip(voters, (sem, ins)):
            v.add(cells[-1], image[at:at + F])
        at += F
    kept = fu.kept(min_obs)
    assert kept.is_cuda and kept.dtype == torch.int32 and torch.equal(kept.cpu(), fz.kept(min_obs)) and 0 < kept.numel()
    assert (min_obs == 1) == (kept.numel() == fu.cells)
    fused = fu.snapshot(min_obs, torch.cat(cells))
    for v, image in zip(voters, (sem, ins)):
        got = v.snapshot(fu.cells, rows=kept)[0]
        assert vc.same_lifted(got, frames.lift(fused, image, vc.IGNORE))
        assert vc.same_lifted(got, frames.lift(fz.snapshot(min_obs, vc.dense4_cells(0.1)[0]), image, vc.IGNORE))
    for kw in ({}, {"min_votes": 3, "min_share": 0.9}):
        want = frames.lift_scene_host(fz.snapshot(min_obs, vc.dense4_cells(0.1)[0]), sem, ins, ignore=vc.IGNORE, **kw)
        for _ in range(2):
            got = frames.lift_scene_stream(fu, *voters, min_obs=min_obs, **kw)
            assert all(x.is_cuda and x.dtype == torch.int32 and torch.equal(x.cpu(), w) for x, w in zip(got, want))
        one = frames.lift_scene(fused, sem, ins, ignore=vc.IGNORE, **kw)
        assert all(torch.equal(x, w) for x, w in zip(got, one))
        sem_l, ins_l = (v.snapshot(fu.cells, rows=kept)[0] for v in voters)
        assert all(torch.equal(x, w) for x, w in zip(frames.scene_labels(sem_l, ins_l, **kw), one))


@pytest.mark.parametrize("stride", [2, 3])
def test_full_resolution_images_at_a_stride(hip, stride):
    cells, fz = vc.dense4_cells(0.1, stride)
    sem, ins = lc.images("dense", 4)
    for image in (sem, ins):
        vh, _ = _check(vc.frame_adds(cells, image, vc.SPLITS["1+3"]), fz.cells, vc.IGNORE, stride=stride)
        assert vh.pairs > 100
    # narrow: 67 x 5 is no multiple of either stride
    cells, fz = vc.narrow3_cells(stride)
    _check(vc.frame_adds(cells, lc.images("narrow")[0], (1, 1, 1)), fz.cells, None, stride=stride)


def test_narrow_frames_a_partial_last_wave(hip):
    cells, fz = vc.narrow3_cells()
    assert cells.numel() == lc.NARROW_PIXELS
    for image in lc.images("narrow"):
        _check(vc.frame_adds(cells, image, (1, 1, 1)), fz.cells, vc.IGNORE)
        _check(vc.frame_adds(cells, image, (3,)), fz.cells, vc.IGNORE)  # 1005 elements in one add: 15 waves + 45 lanes


@pytest.mark.parametrize("kind", ["same", "alternate", "runs", "alone"])
def test_one_dimensional_regimes_cut_into_adds(hip, kind):
    group, value, n = lc.one_group(kind)
    vh, _ = _check(vc.cut(group, value, vc.ONE_GROUP_CUTS), n)
    got, pairs = vh.snapshot(n)
    votes = got.votes.numpy()
    if kind == "same":
        assert pairs == 1 and votes.tolist() == [lc.FRAME_PIXELS]       # every wave one run; the second add finds the key
    elif kind == "alternate":
        assert pairs == 2 and got.label.tolist() == [1] and votes.tolist() == [lc.FRAME_PIXELS // 2]
    elif kind == "runs":
        assert pairs == n and (votes == lc.RUN).all()                    # the runs cut by the adds are whole again
    else:
        assert pairs == n == lc.FRAME_PIXELS and (votes == 1).all()


def test_a_winner_that_changes_between_snapshots(hip):
    vh, _ = _check(vc.changing_winner(), 1)
    assert vh.snapshot(1)[0].label.tolist() == [1] and vh.snapshot(1)[0].votes.tolist() == [4]


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.int32])
def test_value_types_rows_and_mixed_dtypes(hip, dtype):
    group, value = (np.array(a) for a in lc.random_votes())
    top = int(np.iinfo(dtype).max)
    value = np.where(value < 0, 3, value).astype(dtype)
    group[::9], value[::9] = 36, top  # the type's largest value wins group 36
    perm = np.random.default_rng(0).permutation(37).astype(np.int32)[:20]
    for ignore in (None, top, 1):
        vh, voters = _check(vc.cut(group, value, (100, 350)), 37, ignore, fill=-9, rows=perm, on_device=False)
        assert (vh.snapshot(37)[0].label[36] == top) == (ignore != top)
    v = voters[0]
    got = v.snapshot(37, rows=perm.copy())[0]
    assert vc.same_lifted(v.snapshot(37, rows=torch.from_numpy(perm.copy()).cuda())[0], got)
    assert all(a.shape == (0,) and a.is_cuda for a in v.snapshot(37, rows=np.zeros(0, np.int32))[0])
    for bad in ([0, 37], [-1], [2 ** 31 - 1]):
        for where in ("cpu", "cuda"):
            with pytest.raises(ValueError, match="rows holds"):
                v.snapshot(37, rows=torch.tensor(bad, dtype=torch.int32, device=where))
    with pytest.raises(ValueError, match="outside the 36 groups"):
        v.snapshot(36)
    with pytest.raises(ValueError, match="outside the 0 groups"):
        v.snapshot(0)
    if dtype == np.int32:  # negative values do not vote; mixed dtypes across the adds of one voter
        g, neg = lc.random_votes()
        assert (np.asarray(neg) < 0).any()
        _check(vc.cut(g, neg, (100, 350)), 37, None, fill=-3)
        parts = vc.cut(group, np.minimum(value, 200), (150, 400))
        mixed = [(parts[0][0], parts[0][1].astype(np.uint8)), (parts[1][0], parts[1][1].astype(np.uint16)), parts[2]]
        vh, _ = _check(mixed, 37, 1)
        assert vc.same_state(vh, _check(parts, 37, 1)[0])


def test_nothing_votes_and_empty_adds(hip):
    group, value = lc.random_votes()
    e = np.zeros(0, np.int32)
    vh, voters = _check([(group, np.full_like(value, 4)), (e, e), (np.full_like(group, -1), np.array(value))], 37, ignore=4, fill=-9)
    assert vh.pairs == 0 and vh.elements == 1200 and all(v.rehashes == 0 for v in voters)
    v = frames.Voter()
    v.add(e, e)
    v.add(np.zeros((0, 3, 4), np.int32), np.zeros((0, 6, 8), np.uint8), 2)
    assert v.slots is None and v.pairs == 0 and v.elements == 0 and v.state()[0].shape == (0,)
    got, pairs = v.snapshot(5)
    assert got.label.tolist() == [-100] * 5 and got.votes.tolist() == [0] * 5 and got.total.tolist() == [0] * 5 and pairs == 0
    assert all(a.shape == (0,) and a.is_cuda for a in v.snapshot(0)[0])


def test_a_failed_add_leaves_no_trace(hip):
    first, many, later = vc.many_values()
    vh = frames.VoterHost()
    vh.add(*first)
    for aggregate in (True, False):
        v = frames.Voter(slots=vc.MIN_SLOTS, aggregate=aggregate)
        v.add(*first)  # 40 keys in 64 slots: cannot fail
        assert v.slots == vc.MIN_SLOTS and v.rehashes == 0 and _same_state(v.state(), vh.state())
        state, keys, cnt = v.state(), v._keys.clone(), v._cnt.clone()
        snap, pairs = v.snapshot(1)
        proven = frames.voter_slots(vc.FIRST_VALUES, vc.MANY_VALUES)[1]
        assert proven == vc.MANY_SLOTS
        # 1000 more pairs cannot fit in the 24 free slots: the flag is certain
        with pytest.raises(ValueError, match=f"overflowed; {proven} slots are always enough"):
            v.add(*many)
        assert v.rehashes == 1 and v.retries == 0 and v.slots == vc.MIN_SLOTS
        assert v.pairs == vc.FIRST_VALUES == pairs and v.elements == vh.elements and _same_state(v.state(), state)
        assert int((v._keys != -1).sum()) == vc.FIRST_VALUES and int((v._cnt > 0).sum()) == vc.FIRST_VALUES  # no claim is left
        assert torch.equal(v._keys.sort().values, keys.sort().values) and torch.equal(v._cnt.sort().values, cnt.sort().values)
        got, p = v.snapshot(1)
        assert vc.same_lifted(got, snap) and p == pairs
    # values that hash among what the failed add claimed are counted exactly (the last voter goes on)
    want = frames.VoterHost()
    want.add(*first)
    want.add(later[0][:vc.FIRST_VALUES // 4], later[1][:vc.FIRST_VALUES // 4])  # 10 of the failed add's values: 50 keys fit
    want.add(later[0][vc.FIRST_VALUES // 2:], later[1][vc.FIRST_VALUES // 2:])  # the first add's own keys again
    v.add(later[0][:vc.FIRST_VALUES // 4], later[1][:vc.FIRST_VALUES // 4])
    v.add(later[0][vc.FIRST_VALUES // 2:], later[1][vc.FIRST_VALUES // 2:])
    assert _same_state(v.state(), want.state()) and vc.same_lifted(v.snapshot(1)[0], want.snapshot(1)[0])
    assert v.pairs == want.pairs == vc.FIRST_VALUES + vc.FIRST_VALUES // 4
    for bad in (0, 32, 63, 96, 1 << 32):
        with pytest.raises(ValueError, match="power of two"):
            frames.Voter(slots=bad)


def test_the_default_table_retries_once_and_the_unbounded_regime(hip):
    first, many, later = vc.many_values()
    vh, voters = _check([first, many, later], 1)
    assert vh.pairs == vc.FIRST_VALUES + vc.MANY_VALUES
    for v in voters:  # the default table overflows at the second add: rehashed once to the proven size, the add run once more
        assert v.retries == 1 and v.rehashes >= 2 and 4 * v.pairs <= v.slots
    _, voters = _check([first, many, later], 1, slots=vc.MANY_SLOTS)   # >= 2 (P + T) at every add: unbounded, never a rehash
    assert all(v.retries == 0 and v.rehashes == 0 and v.slots == vc.MANY_SLOTS for v in voters)
    assert lc.MANY_SLOTS >= 2 * many[0].size                            # the lift tests' unbounded table, as the first add
    _, voters = _check([many], 1, slots=lc.MANY_SLOTS)
    assert all(v.retries == 0 and v.rehashes == 0 for v in voters)


def test_a_third_full_table_is_exact_or_says_overflow(hip):
    group, value = vc.third_full()
    vh = frames.VoterHost()
    vh.add(group, value)
    assert vh.pairs == vc.THIRD_VALUES and vc.THIRD_SLOTS < 2 * value.size
    v = frames.Voter(slots=vc.THIRD_SLOTS)
    try:
        v.add(group, value)
    except ValueError as e:
        assert "overflowed" in str(e) and v.pairs == 0 and v.state()[0].shape == (0,)
        v = frames.Voter()
        v.add(group, value)
    assert _same_state(v.state(), vh.state()) and vc.same_lifted(v.snapshot(1)[0], vh.snapshot(1)[0])


def test_growth_by_rehash_carries_the_counts(hip):
    group, value, n = lc.one_group("alone")
    vh, voters = _check(vc.cut(group, value, vc.ONE_GROUP_CUTS), n)
    for v in voters:  # 4800 pairs from a table that began at 125 -> 128 slots
        assert v.rehashes > 0 and 4 * v.pairs <= v.slots < 8 * v.pairs
        before = v.state()
        for s in (v.slots * 2, v.slots // 2):  # two slots per pair and more: counts do not change across a rehash
            v._rehash(s)
            assert v.slots == s and _same_state(v.state(), before)
        assert vc.same_lifted(v.snapshot(n)[0], vh.snapshot(n)[0])


def test_a_failed_add_into_a_given_table_more_than_half_full(hip):
    # A given table is kept, so successful adds take it above half full; the rehash that cleans up after a failed add
    # must still find room (one slot per pair is enough), and the error must be the ValueError, not the library's.
    adds = vc.crowded()
    _, many, _ = vc.many_values()
    vh, voters = _check(adds[:3], 5, slots=vc.CROWDED_SLOTS)
    for v in voters:
        assert v.pairs == 3 * vc.CROWDED_VALUES > vc.CROWDED_SLOTS // 2 and v.rehashes == 0 and v.slots == vc.CROWDED_SLOTS
        state, snap = v.state(), v.snapshot(5)
        with pytest.raises(ValueError, match=r"overflowed; \d+ slots are always enough"):
            v.add(*many)
        assert v.rehashes == 1 and v.slots == vc.CROWDED_SLOTS and _same_state(v.state(), state)
        assert int((v._keys != -1).sum()) == v.pairs  # no claim is left
        got = v.snapshot(5)
        assert vc.same_lifted(got[0], snap[0]) and got[1] == snap[1]
    # the table still works: keys it knows, and a few new ones
    few = (adds[3][0][:30], adds[3][1][:30])
    vh.add(*adds[0])
    vh.add(*few)
    v.add(_dev(torch.from_numpy(np.array(adds[0][0]))), adds[0][1])
    v.add(*few)
    assert _same_state(v.state(), vh.state()) and v.pairs == 3 * vc.CROWDED_VALUES + 10


def test_the_element_budget_and_other_failed_adds(hip, monkeypatch):
    group, value = lc.random_votes()
    v = frames.Voter()
    v.add(group[:300], value[:300])
    state, slots, rehashes = v.state(), v.slots, v.rehashes
    monkeypatch.setattr(frames, "VOTER_MAX_ELEMENTS", 500)
    with pytest.raises(ValueError, match="at most 500"):
        v.add(group[:201], value[:201])
    monkeypatch.undo()
    for g, x, s, match in ((group[:5], value[:4], None, "differ in shape"), (group[:5].astype(np.int64), value[:5], None, "int32"),
                           (group[:5], value[:5].astype(np.int64), None, "uint8, uint16 or int32"),
                           (group[:6], value[:6], 2, "does not sample")):
        with pytest.raises(ValueError, match=match):
            v.add(g, x, s)
    assert v.elements == 300 and v.slots == slots and v.rehashes == rehashes and _same_state(v.state(), state)


def test_argument_checks_launch_nothing(hip):
    from geoformer_amd import _lib
    from geoformer_amd._lib import GeoFormerHipError, ptr

    lib = _lib.load()
    out = torch.full((4096,), 7, dtype=torch.int32, device="cuda")
    p = ptr(out)
    good = dict(kind=2, F=2, W=4, H=4, stride=1, slots=64, pairs=0)

    def add(a, null=None):
        q = {k: (None if k == null else p) for k in ("group", "value", "keys", "cnt", "scratch", "words")}
        return lib.gf_frames_votes_add(q["group"], q["value"], a["kind"], a["F"], a["W"], a["H"], a["stride"], 0, 0, q["keys"],
                                       q["cnt"], a["slots"], a["pairs"], 1, q["scratch"], q["words"], None)

    big = lib.gf_resample_max_points()
    assert big == 1 << 29
    for k, v in (("kind", 3), ("kind", -1), ("F", -1), ("W", -1), ("H", -1), ("stride", 0), ("W", big + 1), ("F", big),
                 ("slots", 0), ("slots", 32), ("slots", 96), ("slots", (1 << 31) + 1), ("slots", 1 << 32), ("pairs", -1),
                 ("pairs", 65), ("pairs", 2 ** 31 - 1)):
        st = add(dict(good, **{k: v}))
        assert st != 0, (k, v)
        with pytest.raises(GeoFormerHipError):
            _lib.check(st, "gf_frames_votes_add")
    for null in ("group", "value", "keys", "cnt", "scratch", "words"):
        assert add(good, null) != 0, null
    for k in ("F", "W", "H"):  # T == 0: success, nothing launched, nothing written, NULL pointers allowed
        assert add(dict(good, **{k: 0}), "group") == 0, k
    # the two halves on their own
    assert lib.gf_frames_votes_claim(p, p, 3, 2, 4, 4, 1, 0, 0, p, 64, 0, 1, p, p, None) != 0
    assert lib.gf_frames_votes_claim(p, p, 2, 2, 4, 4, 1, 0, 0, None, 64, 0, 1, p, p, None) != 0
    assert lib.gf_frames_votes_claim(p, p, 2, 2, 4, 4, 1, 0, 0, p, 96, 0, 1, p, p, None) != 0
    for T, slots, nulls in ((-1, 64, ()), (big + 1, 64, ()), (5, 32, ()), (5, 64, (0,)), (5, 64, (1,)), (5, 64, (2,))):
        a = [None if k in nulls else p for k in range(3)]
        assert lib.gf_frames_votes_commit(a[0], T, a[1], slots, a[2], None) != 0, (T, slots, nulls)
    assert lib.gf_frames_votes_commit(None, 0, None, 64, None, None) == 0
    far = ptr(out[2048:])
    for old_slots, pairs, new_slots in ((32, 0, 64), (64, 0, 96), (0, 1, 64), (64, -1, 64), (64, 0, 0), (64, 0, 1 << 32), (64, 65, 64)):
        assert lib.gf_frames_votes_rehash(p, p, old_slots, pairs, far, far, new_slots, None) != 0, (old_slots, pairs, new_slots)
    assert lib.gf_frames_votes_rehash(p, p, 64, 0, p, p, 64, None) != 0  # the tables overlap
    assert lib.gf_frames_votes_rehash(None, None, 0, 0, None, p, 64, None) != 0
    assert lib.gf_frames_votes_rehash(None, p, 64, 0, far, far, 64, None) != 0

    def pick(slots=64, n=8, null=None):
        a = [None if k == null else p for k in range(7)]
        return lib.gf_frames_votes_pick(a[0], a[1], slots, n, -100, a[2], a[3], a[4], a[5], a[6], None)

    for slots, n in ((0, 8), (32, 8), (96, 8), (1 << 32, 8), (64, -1), (64, 1 << 31)):
        assert pick(slots, n) != 0, (slots, n)
    for null in range(7):
        assert pick(null=null) != 0, null
    assert pick(n=0, null=0) == 0  # no group: success, nothing launched
    torch.cuda.synchronize()
    assert bool((out == 7).all())


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


def test_a_labelled_stream_through_the_model_equals_the_one_shot_path(model):
    from geoformer_amd import batch_eval
    from geoformer_amd import evaluation as E

    fr = fc.make(fc.dense(), "u16")
    sem_i, ins_i = lc.images("dense")
    fu, sem_v, ins_v = frames.Fuser(0.02), frames.Voter(lc.IGNORE), frames.Voter(lc.IGNORE)
    for k in range(3):
        cells = fu.add(sc.sub(fr, k, k + 1))
        sem_v.add(cells, sem_i[k:k + 1])
        ins_v.add(cells, ins_i[k:k + 1])
    sem, inst = frames.lift_scene_stream(fu, sem_v, ins_v)
    sem = torch.where(sem >= 0, sem - 1, sem)  # the images hold the dataset's class + 1
    raw, shift = fu.snapshot(1).raw_scene(semantic=sem, instance=inst)
    one = frames.fuse(fr, 0.02, origin=fu.origin)
    sem1, inst1 = frames.lift_scene(one, sem_i, ins_i, ignore=lc.IGNORE)
    raw1, shift1 = one.raw_scene(semantic=torch.where(sem1 >= 0, sem1 - 1, sem1), instance=inst1)
    n = one.xyz.shape[0]
    assert raw.tobytes() == raw1.tobytes() and shift.tobytes() == shift1.tobytes() and raw.shape == (n, 8) and n > 1000
    assert set(np.unique(raw[:, 7])) == {-100.0, 0.0} and {0.0, 1.0, 4.0} <= set(np.unique(raw[:, 6])) <= {-100.0, 0.0, 1.0, 4.0}
    items = [("frames", raw)]
    np.random.seed(0)
    ap, avgs = batch_eval.evaluate(model, items, 1, classes=0, final_score_thresh=0.0)
    shape = E.InstanceEvaluator(classes=0)
    assert ap.shape == (len(shape.class_ids), len(shape.overlaps))
    assert (np.isnan(ap) | ((ap >= 0) & (ap <= 1))).all() and "all_ap" in avgs
