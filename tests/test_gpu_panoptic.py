"""GPU: gf_panoptic_overlaps (csrc/panoptic.hip) against its numpy statement (evaluation.panoptic_overlaps_host), exactly,
in both count regimes; the overflow repeat; postprocess.panoptic_points; batch_eval.panoptic_batches /
evaluate_panoptic end to end."""
import numpy as np
import pytest
import torch

from tests.test_gpu_label_map import calibrated_model  # noqa: F401  (the small calibrated model and its four scenes)
from tests.test_panoptic_host import random_batch

pytestmark = pytest.mark.gpu

CLASS_IDS = np.array([5, 1, 9, 2, 3], np.int64)  # not sorted
IS_STUFF = np.array([0, 1, 0, 1, 0], bool)
SOS = np.array([3, 1, -1, 0, 7, -4], np.int32)  # floor, wall, nothing, a thing class, out of range twice
N_STUFF = 2
REGIMES = (-1, 0, 64)  # LDS bins: the default table, never the table, a table only the smallest scenes fit


def dev(a, dtype=torch.int32):
    return torch.as_tensor(np.asarray(a)).to(dtype).cuda().contiguous()


def class_tables():
    return dev(CLASS_IDS), dev(IS_STUFF), dev(SOS)


@pytest.fixture
def lds_bins(hip):
    """Sets the LDS table's capacity (gf_dev_panoptic_lds_bins) and puts the default back afterwards."""
    def knob(bins):
        assert hip.gf_dev_panoptic_lds_bins(bins) == 0

    yield knob
    knob(-1)


def host(owner, ids, sem, gt, off, P, max_gt=None):
    from geoformer_amd import evaluation as E

    return E.panoptic_overlaps_host(owner, sem, gt, off, class_ids=CLASS_IDS, is_stuff=IS_STUFF, stuff_of_sem=SOS, P=P,
                                    ids=ids, max_gt=max_gt)


def device(owner, ids, sem, gt, off, P, max_gt=256, check_offsets=True):
    from geoformer_amd import pointops

    off_h = torch.as_tensor(np.asarray(off)).to(torch.int32).contiguous()
    pan, G, gt_id, inter, used = pointops.panoptic_overlaps(
        dev(owner), dev(ids), dev(sem), dev(gt, torch.int64), off_h.cuda(), *class_tables(), N_STUFF, P, max_gt=max_gt,
        offsets_host=off_h if check_offsets else None)
    return pan.cpu().numpy(), G.copy(), gt_id.copy(), inter.copy(), used


def same(got, want):
    """(pan, G, gt_id, inter) of the device and of the host statement: every integer."""
    for k, g, w in zip(("pan", "G", "gt_id", "inter"), got, want):
        assert g.shape == w.shape and np.array_equal(g, w), k


def pool_gt(rng, N, G):
    """gt ids with exactly G distinct segments of the evaluated thing classes (and some void points)."""
    pool = np.array([c * 1000 + i for i in range(1, 400) for c in (3, 5, 9)], np.int64)[:G]
    gt = pool[rng.integers(0, G, N)] if G else np.zeros(N, np.int64)
    gt[:G] = pool  # every segment occurs
    gt[rng.integers(G, N, N // 16)] = 0
    return gt


def test_limits(hip):
    from geoformer_amd import pointops, postprocess

    rows, run = pointops.panoptic_limits()
    assert rows >= postprocess.NMS_MAX_N + 2 + 1 and run >= 64


@pytest.mark.parametrize("bins", REGIMES)
def test_packed_scenes_one_by_one_and_again(hip, lds_bins, bins):
    """63, 0 and 1025 points: an empty scene in the middle, a scene boundary inside one run."""
    lds_bins(bins)
    Ns, P = (63, 0, 1025), 5
    owner, ids, sem, gt, off = random_batch(np.random.default_rng(1), Ns, P, CLASS_IDS, len(SOS))
    got = device(owner, ids, sem, gt, off, P)
    want = host(owner, ids, sem, gt, off, P, max_gt=256)
    same(got[:4], want)
    assert got[1].tolist() == want[1].tolist() and got[1][1] == 0 and got[4] == 256
    same(device(owner, ids, sem, gt, off, P, check_offsets=False)[:4], got[:4])  # a second call, the same again
    for s in range(3):  # the scenes alone: bit-equal tables and pan
        sl = slice(off[s], off[s + 1])
        one = device(owner[sl], ids[sl], sem[sl], gt[sl], [0, Ns[s]], P)
        assert np.array_equal(one[0], got[0][sl])
        for k in (1, 2, 3):
            assert np.array_equal(one[k][0], got[k][s]), (s, k)


@pytest.mark.parametrize("bins", (-1, 0))
@pytest.mark.parametrize("N,P", [(4097, 51), (-1, 0), (0, 1), (1, 1024)])
def test_sizes_and_pick_counts(hip, lds_bins, bins, N, P):
    """N = 4097 and the run length - 1, + 0, + 1; P = 0, 1, 51, 1024 (about 20 segments: P = 1024 is past the LDS
    table in either setting, the others fit it)."""
    from geoformer_amd import pointops

    lds_bins(bins)
    N = N if N > 1 else pointops.panoptic_limits()[1] + N
    owner, ids, sem, gt, off = random_batch(np.random.default_rng(N + P), (N,), P, CLASS_IDS, len(SOS))
    got = device(owner, ids, sem, gt, off, P, max_gt=32)
    same(got[:4], host(owner, ids, sem, gt, off, P, max_gt=32))
    assert got[3].sum() == N


@pytest.mark.parametrize("bins", (-1, 0))
def test_usual_size_in_both_regimes(hip, lds_bins, bins):
    """P = 51 and 60 segments (a few thousand bins: the LDS table by itself), and the same forced to global atomics."""
    lds_bins(bins)
    rng = np.random.default_rng(7)
    N, P = 4097, 51
    owner, ids, sem, _, off = random_batch(rng, (N,), P, CLASS_IDS, len(SOS), wild=False)
    gt = pool_gt(rng, N, 60)
    got = device(owner, ids, sem, gt, off, P)
    assert got[1].tolist() == [60]
    same(got[:4], host(owner, ids, sem, gt, off, P, max_gt=256))


def test_large_table_regime(hip):
    """P = 1024 with max_gt = 256 at N = 8192: 1027 * 201 bins do not fit the LDS table; near-distinct pairs."""
    rng = np.random.default_rng(8)
    N, P = 8192, 1024
    owner = rng.permutation(N) % P
    sem = rng.integers(0, 4, N)
    gt = pool_gt(rng, N, 200)
    ids = 3000 + owner + 1
    got = device(owner, ids, sem, gt, [0, N], P)
    assert got[1].tolist() == [200] and (got[3] > 0).sum() > N // 2  # more than half of the points alone in their bin
    same(got[:4], host(owner, ids, sem, gt, [0, N], P, max_gt=256))


@pytest.mark.parametrize("bins", (-1, 0))
@pytest.mark.parametrize("P", (3, 1024))
def test_all_points_in_one_pair(hip, lds_bins, bins, P):
    """Maximal contention; with one segment the 1027 rows of P = 1024 fit the LDS table."""
    lds_bins(bins)
    N = 8192
    owner, sem, gt = np.full(N, P - 1), np.zeros(N, np.int64), np.full(N, 9004, np.int64)
    got = device(owner, 3000 + owner + 1, sem, gt, [0, N], P, max_gt=4)
    assert got[3][0, P - 1, 0] == N and got[3].sum() == N and got[2][0].tolist() == [9004, 0, 0, 0]
    same(got[:4], host(owner, 3000 + owner + 1, sem, gt, [0, N], P, max_gt=4))


def test_capacity_reached_and_exceeded(hip):
    """G = max_gt fits; G = max_gt + 1 reports G alone, leaves the batch's other scenes right, and the wrapper repeats."""
    from geoformer_amd import pointops

    rng = np.random.default_rng(9)
    Ns, P, cap = (300, 500, 260), 4, 16
    owner, ids, sem, _, off = random_batch(rng, Ns, P, CLASS_IDS, len(SOS), wild=False)
    gt = np.concatenate([pool_gt(rng, Ns[0], cap), pool_gt(rng, Ns[1], cap + 1), pool_gt(rng, Ns[2], 3)])
    R = P + N_STUFF + 1
    pan, buf, lay = pointops.panoptic_overlaps_packed(dev(owner), dev(ids), dev(sem), dev(gt, torch.int64), dev(off),
                                                      *class_tables(), N_STUFF, P, max_gt=cap)
    G, gt_id, inter = pointops.panoptic_unpack(buf.cpu().numpy(), lay, 3, R, cap)
    want = host(owner, ids, sem, gt, off, P, max_gt=cap)  # (the statement leaves an overflowing scene at zero)
    assert G.tolist() == [cap, cap + 1, 3] == want[1].tolist()
    assert np.array_equal(pan.cpu().numpy(), want[0])
    assert not inter[1].any()
    for s in (0, 2):
        assert np.array_equal(gt_id[s], want[2][s]) and np.array_equal(inter[s], want[3][s]), s
        assert inter[s].sum() == Ns[s]
    got = device(owner, ids, sem, gt, off, P, max_gt=cap)
    assert got[4] == cap + 1
    same(got[:4], host(owner, ids, sem, gt, off, P, max_gt=cap + 1))
    assert [int(got[3][s].sum()) for s in range(3)] == list(Ns)


def test_malformed_offsets_are_refused_before_any_launch(hip):
    N, P = 100, 2
    owner, ids, sem, gt, _ = random_batch(np.random.default_rng(3), (N,), P, CLASS_IDS, len(SOS))
    d = [dev(owner), dev(ids), dev(sem), dev(gt, torch.int64)]
    cls, st, sos = class_tables()
    off_d = dev([0, 40, N])
    R, cap = P + N_STUFF + 1, 8
    scratch = torch.zeros(hip.gf_panoptic_overlaps_scratch_bytes(2, N, 5) // 4 + 1, dtype=torch.int32, device="cuda")
    for what, bad in (("first", [1, 40, N]), ("descending", [0, 60, 40]), ("last", [0, 40, N - 1])):
        pan = torch.full((N,), -7, dtype=torch.int32, device="cuda")
        out = torch.full((2 + 2 * 2 * cap + 2 * R * (cap + 1),), -7, dtype=torch.int32, device="cuda")
        h = torch.tensor(bad, dtype=torch.int32)
        base = out.data_ptr()
        rc = hip.gf_panoptic_overlaps(*[t.data_ptr() for t in d], off_d.data_ptr(), h.data_ptr(), 2, N, cls.data_ptr(),
                                      st.data_ptr(), 5, sos.data_ptr(), len(SOS), N_STUFF, P, cap, scratch.data_ptr(),
                                      pan.data_ptr(), base, base + 8, base + 8 + 8 * 2 * cap, None)
        torch.cuda.synchronize()
        assert rc < 0 and b"gf_panoptic_overlaps" in hip.gf_last_error(), what
        assert (pan == -7).all() and (out == -7).all(), what


def test_labels_alone_and_from_scene_labels(hip):
    """pointops.panoptic_points (no ground truth, one launch) and postprocess.panoptic_points_batched on label maps."""
    from geoformer_amd import pointops, postprocess

    Ns, P = (700, 1300), 6
    owner, ids, sem, gt, off = random_batch(np.random.default_rng(4), Ns, P, CLASS_IDS, len(SOS))
    want = host(owner, ids, sem, gt, off, P)[0]
    pan = pointops.panoptic_points(dev(owner), dev(ids), dev(sem), dev(off), *class_tables(), N_STUFF, P)
    assert np.array_equal(pan.cpu().numpy(), want)
    # label maps of two scenes, the semantic head's classes 0 / 1 as wall / floor
    rng = np.random.default_rng(5)
    labs, sems = [], []
    for N in Ns:
        masks = (rng.random((4, N)) < 0.2).astype(np.int32)
        labs.append(postprocess.label_points(dev(masks), torch.tensor([0.9, 0.8, 0.7, 0.05]).cuda(),
                                             dev([3, 5, 3, 9], torch.int64), dev([0, 1, 2, 3], torch.int64),
                                             torch.zeros((N, 3), device="cuda")))
        sems.append(dev(rng.integers(0, 5, N)))
    pans = postprocess.panoptic_points_batched(labs, sems)
    one = postprocess.panoptic_points(labs[1], sems[1])
    for lab, s, pan in zip(labs, sems, pans):
        o, i, s = lab.owner.cpu().numpy(), lab.ids.cpu().numpy(), s.cpu().numpy()
        ref = np.where(o >= 0, i, np.where(s == 0, 1000, np.where(s == 1, 2000, 0)))
        assert pan.dtype == torch.int32 and np.array_equal(pan.cpu().numpy(), ref)
        assert (ref == 1000).any() and (ref == 2000).any() and (ref > 3000).any() and (ref == 0).any()
    assert torch.equal(one, pans[1])


def _bit_equal(a, b):
    assert np.array_equal(a.owner, b.owner) and np.array_equal(a.ids, b.ids)
    for k, x, y in zip(a.table._fields, a.table, b.table):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k


def test_panoptic_batches_end_to_end(calibrated_model):  # noqa: F811
    from geoformer_amd import batch_eval
    from geoformer_amd import evaluation as E

    model, items = calibrated_model
    shape = np.max([b["spatial_shape"] for B in (1, 4) for b in batch_eval.collate_batches(items, B)[1]], axis=0)
    kw = dict(spatial_shape=shape, reserve=False, final_score_thresh=0.0, min_score=0.0)

    def labels():
        np.random.seed(21)
        return list(batch_eval.label_batches(model, items, 4, **kw))

    before = labels()
    np.random.seed(21)
    got = list(batch_eval.panoptic_batches(model, items, 4, **kw))
    sem = {n: p.cpu().numpy() for n, p in batch_eval.semantic_batches(model, items, 4, spatial_shape=shape, reserve=False)}
    after = labels()
    assert [n for n, *_ in got] == [n for n, _ in items]
    n_things = n_stuff = 0
    for (name, lab), (_, lab2), (gname, glab, pan) in zip(before, after, got):
        _bit_equal(lab, lab2)  # label_batches before and after a panoptic_batches run
        _bit_equal(lab, glab)  # and the labels that travel with pan
        s = sem[name]
        ref = np.where(lab.owner >= 0, lab.ids, np.where(s == 0, 1000, np.where(s == 1, 2000, 0)))
        assert isinstance(pan, np.ndarray) and pan.dtype == np.int32 and np.array_equal(pan, ref), name
        n_things += int((lab.owner >= 0).sum())
        n_stuff += int(((ref == 1000) | (ref == 2000)).sum())
    print(f"{n_things} thing points, {n_stuff} stuff points over {len(items)} scenes")
    assert n_things > 0 and n_stuff > 0
    # PQ of the loop against panoptic_quality on host tables of the same labels
    np.random.seed(21)
    ev = E.PanopticEvaluator(classes=model.cfg.cvfold)
    res = batch_eval.evaluate_panoptic(model, items, 4, classes=model.cfg.cvfold, evaluator=ev, **kw)
    tables = []
    for (name, raw), (_, lab) in zip(items, before):
        gt = E.gt_ids_from_labels(raw[:, 6].astype(np.int64), raw[:, 7].astype(np.int64))
        _, Gs, gt_id, inter = E.panoptic_overlaps_host(lab.owner, sem[name], gt, class_ids=ev.class_ids,
                                                       is_stuff=ev.is_stuff, stuff_of_sem=ev.stuff_of_sem,
                                                       P=len(lab.table.label_id))
        tables += E.panoptic_tables(Gs, gt_id, inter, [lab.table.label_id], ev.class_ids, ev.is_stuff,
                                    len(lab.table.label_id))
    want = E.panoptic_quality(tables, ev.class_names)
    for k in ("tp", "fp", "fn", "iou_sum"):
        assert np.array_equal(res[k], want[k]), k
    for k in ("pq", "sq", "rq", "pq_th", "pq_st"):
        assert np.array_equal(res[k], want[k], equal_nan=True), k
    for name, t, w in zip(ev.names, ev.tables, tables):
        assert np.array_equal(t.inter, w.inter) and np.array_equal(t.gt_id, w.gt_id), name
    print(ev.format_results(res))
    assert int(res["tp"].sum() + res["fp"].sum() + res["fn"].sum()) > 0
