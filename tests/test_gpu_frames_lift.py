"""csrc/frames_vote.hip on the GPU: every case bit for bit against the numpy statement frames.vote_host, and each call made
twice (and once without the lane-run aggregation) for equality from call to call.  The sizes and what each straddles are
named in tests/frames_lift_cases.py."""
import numpy as np
import pytest
import torch

from geoformer_amd import frames
from tests import frames_cases as fc
from tests import frames_lift_cases as lc

pytestmark = pytest.mark.gpu


def _cuda(a):
    return a.cuda() if torch.is_tensor(a) else torch.from_numpy(np.array(a)).cuda()


def _equal(lifted, want):
    for x, w, name in zip(lifted, want, ("label", "votes", "total")):
        assert x.is_cuda and x.dtype == torch.int32 and tuple(x.shape) == tuple(w.shape), name
        assert torch.equal(x.cpu(), w), name


def _vote_equals_host(group, value, n, ignore=None, fill=-100, slots=None):
    want, want_pairs = frames.vote_host(group, value, n, ignore, fill)
    g, v = _cuda(group), _cuda(value)
    for agg in (True, True, False):
        got, pairs = frames.vote(g, v, n, ignore, fill, slots, agg)
        _equal(got, want)
        assert pairs == want_pairs
    return want, want_pairs


def _lift_equals_host(fused, image, ignore, stride=None):
    n = fused.xyz.shape[0]
    s = 1 if stride is None else stride
    want, _ = frames.vote_host(fused.point_of.cpu(), np.ascontiguousarray(image[:, ::s, ::s]), n, ignore)
    img = _cuda(image)
    for agg in (None, True, False):
        got = frames.lift(fused, img, ignore, stride=stride, aggregate=agg)
        _equal(got, want)
    return want


def test_limits_are_the_modules(hip):
    from geoformer_amd import _lib

    lib = _lib.load()
    assert lib.gf_frames_vote_max_probes() == frames.VOTE_MAX_PROBES == lc.MAX_PROBES
    for T, n in ((0, 0), (1, 1), (1000, 1), (33, 1000), (lc.FRAME_PIXELS, 7), (19660800, 113305), (1 << 29, 1 << 29)):
        assert lib.gf_frames_vote_default_slots(T, n) == frames.vote_slots(T, n)[0], (T, n)
    assert lib.gf_frames_vote_default_slots((1 << 29) + 1, 1) == 0 and lib.gf_frames_vote_default_slots(1, -1) == 0
    assert lib.gf_frames_vote_scratch_bytes(64, 10) >= 64 * 12 + 80
    assert lib.gf_frames_vote_scratch_bytes(96, 10) == 0 and lib.gf_frames_vote_scratch_bytes(32, 10) == 0


def test_narrow_frames_a_partial_last_wave(hip):
    fused = frames.fuse(fc.make(fc.narrow(), "u16"), 0.05)
    assert fused.point_of.numel() == lc.NARROW_PIXELS
    sem, ins = lc.images("narrow")
    want = _lift_equals_host(fused, sem, lc.IGNORE)
    assert (want.total.numpy() > 0).sum() > 50
    _lift_equals_host(fused, ins, lc.IGNORE)


@pytest.fixture(scope="module")
def dense_fused(hip):
    return frames.fuse(fc.make(fc.dense(), "u16"), 0.05)


@pytest.mark.parametrize("ignore", [None, lc.IGNORE])
@pytest.mark.parametrize("which", ["semantic", "instance", "block_semantic", "block_instance"])
def test_dense_frames_after_fuse(dense_fused, which, ignore):
    pair = lc.block_images("dense") if which.startswith("block") else lc.images("dense")
    image = pair[which.endswith("instance")]
    want = _lift_equals_host(dense_fused, image, ignore)
    label, votes, total = (a.numpy() for a in want)
    count = dense_fused.count.cpu().numpy()
    assert (label >= 0).sum() > 200
    if ignore is None:
        assert (total > votes).any()          # (points that heard more than one label)
        assert np.array_equal(total, count)   # every pixel of a point voted
    else:
        assert (label != lc.IGNORE).all()
        # only the instance images are IGNORE on pixels that have a point (the background has none)
        assert (total < count).any() == which.endswith("instance")


@pytest.mark.parametrize("dtype,top", [(np.uint8, 255), (np.uint16, 65535), (np.int32, 2 ** 31 - 1)])
def test_value_types_up_to_their_largest(hip, dtype, top):
    group, value = (np.array(a) for a in lc.random_votes())
    value = np.where(value < 0, 3, value).astype(dtype)
    group[::9], value[::9] = 36, top  # the type's largest value wins group 36
    for ignore in (None, top, 1):
        want, _ = _vote_equals_host(group, value, 37, ignore)
        assert (want.label[36] == top) == (ignore != top)
    if dtype == np.int32:
        neg = np.array(lc.random_votes()[1])
        assert (neg < 0).any()
        _vote_equals_host(group, neg, 37, None, fill=-3)


@pytest.mark.parametrize("kind", ["same", "alternate", "runs", "alone"])
def test_one_dimensional_regimes(hip, kind):
    group, value, n = lc.one_group(kind)
    want, pairs = _vote_equals_host(group, value, n)
    votes = want.votes.numpy()
    if kind == "same":
        assert pairs == 1 and votes.tolist() == [lc.FRAME_PIXELS]       # every wave one run, one slot
    elif kind == "alternate":
        assert pairs == 2 and want.label.tolist() == [1] and votes.tolist() == [lc.FRAME_PIXELS // 2]  # a tie: the smaller
    elif kind == "runs":
        assert pairs == n and (votes == lc.RUN).all()
    else:
        assert pairs == n == lc.FRAME_PIXELS and (votes == 1).all()


def test_many_values_on_one_group_overflow_and_retry(hip):
    value = np.random.default_rng(2).permutation(lc.MANY_VALUES).astype(np.int32) + 5
    group = np.zeros_like(value)
    want, want_pairs = frames.vote_host(group, value, 1)
    assert want.label.tolist() == [5] and want.votes.tolist() == [1] and want_pairs == lc.MANY_VALUES
    g, v = _cuda(group), _cuda(value)
    # 1000 pairs cannot fit in 64 slots: the flag is certain
    with pytest.raises(ValueError, match=f"{lc.MANY_SLOTS} slots are always enough"):
        frames.vote(g, v, 1, slots=lc.MIN_SLOTS)
    assert frames.vote_slots(lc.MANY_VALUES, 1) == (lc.MIN_SLOTS, lc.MANY_SLOTS)
    _vote_equals_host(group, value, 1)                        # the default size overflows: one retry at the proven size
    _vote_equals_host(group, value, 1, slots=lc.MANY_SLOTS)   # >= 2 T: the unbounded regime
    for bad in (0, 63, 96, 1 << 31):
        with pytest.raises(ValueError, match="power of two"):
            frames.vote(g, v, 1, slots=bad)


def test_a_third_full_table_is_exact_or_says_overflow(hip):
    value = (np.arange(lc.THIRD_ELEMENTS, dtype=np.int32) % lc.THIRD_VALUES) * 17 + 1
    group = np.zeros_like(value)
    want, want_pairs = frames.vote_host(group, value, 1)
    assert want_pairs == lc.THIRD_VALUES and lc.THIRD_SLOTS < 2 * value.size
    g, v = _cuda(group), _cuda(value)
    try:
        got, pairs = frames.vote(g, v, 1, slots=lc.THIRD_SLOTS)
    except ValueError as e:
        assert "overflowed" in str(e)
        got, pairs = frames.vote(g, v, 1)
    _equal(got, want)
    assert pairs == want_pairs


def test_nothing_votes(hip):
    group, value = lc.random_votes()
    want, pairs = _vote_equals_host(group, np.full_like(value, 4), 37, ignore=4, fill=-9)   # all ignored
    assert pairs == 0 and (want.label.numpy() == -9).all() and not want.total.numpy().any()
    want, pairs = _vote_equals_host(np.full_like(group, -1), np.array(value), 37)           # no valid group
    assert pairs == 0 and (want.label.numpy() == -100).all()
    e = _cuda(np.zeros(0, np.int32))
    got, pairs = frames.vote(e, e, 5)                                                        # T == 0
    assert got.label.tolist() == [-100] * 5 and got.votes.tolist() == [0] * 5 and got.total.tolist() == [0] * 5 and pairs == 0
    got, pairs = frames.vote(e, e, 0)
    assert all(a.shape == (0,) and a.is_cuda for a in got)
    got, _ = frames.vote(_cuda(np.full(3, -1, np.int32)), _cuda(np.ones(3, np.int32)), 0)     # n == 0, nothing to place
    assert got.label.shape == (0,)


def test_a_group_out_of_range_is_a_value_error(hip):
    group, value = lc.random_votes()
    g = np.array(group)
    g[77] = 37
    with pytest.raises(ValueError, match="outside the 37 groups"):
        frames.vote(_cuda(g), _cuda(value), 37)
    with pytest.raises(ValueError, match="outside"):
        frames.vote(_cuda(g), _cuda(value), 0)
    with pytest.raises(ValueError):
        frames.vote(_cuda(g), torch.from_numpy(np.array(value)), 38)  # value on another device


@pytest.mark.parametrize("stride", [2, 3])
def test_full_resolution_images_at_a_stride(hip, stride):
    fused = frames.fuse(fc.make(fc.dense(), "u16"), 0.05, stride)
    sem, ins = lc.images("dense")
    assert fused.point_of.shape[1:] == (-(-fc.DENSE[1] // stride), -(-fc.DENSE[0] // stride))
    for image in (sem, ins, lc.block_images("dense")[1]):
        want = _lift_equals_host(fused, image, lc.IGNORE, stride)
        assert (want.total.numpy() > 0).sum() > 50
    # narrow: 67 x 5 is no multiple of either stride
    fused = frames.fuse(fc.make(fc.narrow(), "u16"), 0.05, stride)
    _lift_equals_host(fused, lc.images("narrow")[0], None, stride)


def test_argument_checks_launch_nothing(hip):
    from geoformer_amd import _lib
    from geoformer_amd._lib import GeoFormerHipError, ptr

    lib = _lib.load()
    out = torch.full((4096,), 7, dtype=torch.int32, device="cuda")
    good = dict(kind=2, F=2, W=4, H=4, stride=1, n=8, slots=64)

    def call(a, null=None):
        p = {k: (None if k == null else ptr(out)) for k in ("group", "value", "scratch", "label", "votes", "total", "words")}
        return lib.gf_frames_vote(p["group"], p["value"], a["kind"], a["F"], a["W"], a["H"], a["stride"], a["n"], 0, 0, -100,
                                  a["slots"], 1, p["scratch"], p["label"], p["votes"], p["total"], p["words"], None)

    big = lib.gf_resample_max_points()
    for k, v in (("kind", 3), ("kind", -1), ("F", -1), ("W", -1), ("H", -1), ("stride", 0), ("n", -1), ("n", big + 1),
                 ("W", big + 1), ("F", big), ("slots", 0), ("slots", 32), ("slots", 96), ("slots", (1 << 30) + 1)):
        st = call(dict(good, **{k: v}))
        assert st != 0, (k, v)
        with pytest.raises(GeoFormerHipError):
            _lib.check(st, "gf_frames_vote")
    for null in ("group", "value", "scratch", "label", "votes", "total", "words"):
        assert call(good, null) != 0, null
    # T == 0 or n == 0: success, nothing launched, nothing written, NULL pointers allowed
    for k in ("F", "W", "H", "n"):
        assert call(dict(good, **{k: 0}), "group") == 0, k
    torch.cuda.synchronize()
    assert bool((out == 7).all())


def test_lift_scene_equals_lift_scene_host(dense_fused):
    for pair, kw in ((lc.block_images("dense"), {}), (lc.block_images("dense"), {"min_votes": 3, "min_share": 0.9}),
                     (lc.images("dense"), {})):
        want = frames.lift_scene_host(dense_fused, *pair, ignore=lc.IGNORE, **kw)
        for _ in range(2):
            got = frames.lift_scene(dense_fused, *pair, ignore=lc.IGNORE, **kw)
            for x, w in zip(got, want):
                assert x.is_cuda and x.dtype == torch.int32 and torch.equal(x.cpu(), w)
        assert int(want[1].max()) >= 0 and bool((want[1] == -100).any())
    s0, i0 = frames.lift_scene(dense_fused, lc.images("dense")[0], np.zeros_like(lc.images("dense")[1]), ignore=lc.IGNORE)
    assert bool((i0 == -100).all()) and torch.equal(s0.cpu(), frames.lift(dense_fused, lc.images("dense")[0], lc.IGNORE).label.cpu())


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


def test_frames_to_a_labelled_scene_that_can_be_scored(model):
    from geoformer_amd import batch_eval
    from geoformer_amd import evaluation as E

    fused = frames.fuse(fc.make(fc.dense(), "u16"), 0.02)
    n = fused.xyz.shape[0]
    sem, inst = frames.lift_scene(fused, *lc.images("dense"), ignore=lc.IGNORE)
    sem = torch.where(sem >= 0, sem - 1, sem)  # the images hold the dataset's class + 1
    raw, _ = fused.raw_scene(semantic=sem, instance=inst)
    assert raw.shape == (n, 8) and n > 1000 and set(np.unique(raw[:, 7])) == {-100.0, 0.0}
    assert {0.0, 1.0, 4.0} <= set(np.unique(raw[:, 6])) <= {-100.0, 0.0, 1.0, 4.0}
    items = [("frames", raw)]
    np.random.seed(0)
    ap, avgs = batch_eval.evaluate(model, items, 1, classes=0, final_score_thresh=0.0)
    shape = E.InstanceEvaluator(classes=0)
    assert ap.shape == (len(shape.class_ids), len(shape.overlaps))
    assert (np.isnan(ap) | ((ap >= 0) & (ap <= 1))).all() and "all_ap" in avgs
    ev = E.SemanticEvaluator(n_classes=model.cfg.classes, train_fold=model.cfg.train_fold)
    res = batch_eval.evaluate_semantic(model, items, 1, evaluator=ev)
    lut, mi, mo = E.semantic_label_lut(model.cfg.train_fold)
    rows = E.map_semantic_labels(raw[:, 6].astype(np.int64), model.cfg.classes, lut, E.IGNORE_LABEL, mi, mo)
    conf = ev.confusion()
    assert conf.sum() == n and np.array_equal(conf.sum(1), np.bincount(rows, minlength=model.cfg.classes + 1))
    assert res["points"] + res["ignored"] == n and res["points"] == int((rows < model.cfg.classes).sum())
