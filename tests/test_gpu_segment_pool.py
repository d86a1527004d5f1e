"""GPU: mask logits pooled over over-segments (csrc/segment_pool.hip, pointops.segment_pool_batched) against the host
statement postprocess.segment_pool_host, and the "segments" key of the eval forward and of batch_eval.

The kernel family has one regime (one workgroup shape, one query tile), so there is no regime knob to go through; the
shapes below reach every path of it: runs inside a wave, across the waves of a workgroup, across workgroups (head /
tail slots, the combine pass, the open-run pass), scenes that end inside a wave, empty scenes."""
import numpy as np
import pytest
import torch

from tests.test_gpu_label_map import calibrated_model  # noqa: F401  (the small calibrated model and its four scenes)

pytestmark = pytest.mark.gpu

BIG = 2 ** 31 - 1


def _ids(rng, k):
    """k distinct segment ids: sparse, unsorted, 0 and the two largest among them (k >= 3)."""
    ids = np.concatenate([[0, BIG, BIG - 1], rng.choice(BIG - 3, size=k, replace=False) + 1])[:k]
    return ids[rng.permutation(k)]


def _scene(rng, nq, runs, singles=0, negatives=0, exact=True, ids=None):
    """(logits fp32 [nq, n], seg int32 [n]): `runs` pooled run lengths, `singles` segments of one point, `negatives`
    points without a segment, the members scattered over the columns."""
    k = len(runs) + singles
    ids = _ids(rng, k) if ids is None else np.asarray(ids)[:k]
    seg = np.concatenate([np.repeat(ids[:len(runs)], runs), ids[len(runs):k],
                          -rng.integers(1, 1000, size=negatives)]).astype(np.int64)
    n = seg.size
    seg = seg[rng.permutation(n)].astype(np.int32)
    if exact:  # multiples of 1/8 in [-32, 32]: every partial sum of up to 4096 of them is exact in fp32
        x = rng.integers(-256, 257, size=(nq, n)).astype(np.float32) / 8
    else:
        x = (rng.standard_normal((nq, n)) * 8).astype(np.float32)
    return x, seg


def _pool(cases):
    from geoformer_amd import pointops

    logits = [torch.from_numpy(x).cuda() for x, _ in cases]
    seg = torch.from_numpy(np.concatenate([s for _, s in cases] + [np.zeros(0, np.int32)])).cuda()
    off = np.concatenate([[0], np.cumsum([s.size for _, s in cases])]).astype(np.int64).tolist()
    out = pointops.segment_pool_batched(logits, seg, off)
    torch.cuda.synchronize()
    assert all((o.numel() == 0 or o.data_ptr() != l.data_ptr()) and o.shape == l.shape and o.dtype == torch.float32
               for o, l in zip(out, logits))
    for l, (x, _) in zip(logits, cases):
        assert l.cpu().numpy().tobytes() == x.tobytes()  # the input is left as it is
    return [o.cpu().numpy() for o in out]


def _cuts(seg, chunk):
    """(runs cut by a workgroup boundary though no longer than a chunk, runs longer than a chunk) of one scene: sorted
    position = rank by (id, point) with the points without a segment behind all others."""
    ids, counts = np.unique(seg[seg >= 0], return_counts=True)
    start = np.concatenate([[0], np.cumsum(counts)[:-1]])
    end = start + counts - 1
    cut = (start // chunk != end // chunk) & (counts <= chunk)
    return int(cut.sum()), int((counts > chunk).sum())


def _exact_batches(rng):
    """name -> list of (logits, seg) per scene; run lengths are powers of two."""
    shared = _ids(rng, 8)
    return {
        # nq = 5; 1 + 64 + ... = 7351 points (not a multiple of 64); a run of 4096 > any chunk; runs cut by chunk boundaries;
        # an empty scene in the middle of three; a scene whose ids are all negative
        "three_scenes": [_scene(rng, 5, [512, 1024, 64, 2, 4096, 8, 1024, 256, 128, 32, 16, 4, 2, 2], 61, 120),
                         (np.zeros((5, 0), np.float32), np.zeros(0, np.int32)),
                         _scene(rng, 5, [], 0, 131)],
        # nq = 1; one run of 4096 of 6826 points (60 %) beside 2730 points of their own; the same ids in the other two scenes
        "skewed": [_scene(rng, 1, [4096], 2730 - 700, 700), _scene(rng, 1, [256, 128, 1024, 2], 4, 3, ids=shared),
                   _scene(rng, 1, [64, 512, 2, 2048], 3, 0, ids=shared)],
        # nq = 256 (16 query tiles), two scenes that end inside a wave
        "many_queries": [_scene(rng, 256, [1024, 2048, 512, 64, 8], 29, 10), _scene(rng, 256, [128, 512, 256], 70, 33)],
    }


def _rounded_batches(rng):
    """The same structure with arbitrary run lengths."""
    shared = _ids(rng, 8)
    return {
        "three_scenes": [_scene(rng, 5, [700, 1500, 3000, 33, 5, 64, 65, 63, 129, 1025, 2, 3], 61, 120, exact=False),
                         (np.zeros((5, 0), np.float32), np.zeros(0, np.int32)),
                         _scene(rng, 5, [], 0, 131, exact=False)],
        "skewed": [_scene(rng, 1, [4100], 2731 - 700, 700, exact=False),
                   _scene(rng, 1, [300, 100, 1111, 2], 4, 3, exact=False, ids=shared),
                   _scene(rng, 1, [77, 500, 2, 2000], 3, 0, exact=False, ids=shared)],
        "many_queries": [_scene(rng, 256, [1000, 2100, 500, 70, 9], 29, 10, exact=False),
                         _scene(rng, 256, [130, 515, 250], 70, 33, exact=False)],
    }


@pytest.fixture(scope="module")
def exact(hip):
    from geoformer_amd import postprocess

    cases = _exact_batches(np.random.default_rng(17))
    return cases, {k: [postprocess.segment_pool_host(x, s) for x, s in v] for k, v in cases.items()}


@pytest.fixture(scope="module")
def rounded(hip):
    from geoformer_amd import postprocess

    cases = _rounded_batches(np.random.default_rng(18))
    return cases, {k: [postprocess.segment_pool_host(x, s) for x, s in v] for k, v in cases.items()}


def test_limits_and_covered_shapes(hip, exact):
    from geoformer_amd import pointops

    fields, chunk = pointops.segment_pool_limits()
    assert fields == 4 and chunk >= 64 and chunk % 64 == 0
    cases, _ = exact
    x, seg = cases["three_scenes"][0]
    cut, longer = _cuts(seg, chunk)
    assert cut >= 1 and longer >= 1 and seg.size % 64 != 0 and seg.size > 2 * chunk
    assert int(seg.max()) == BIG and (seg < 0).any() and (cases["three_scenes"][2][1] < 0).all()
    sk = cases["skewed"][0][1]
    assert np.unique(sk[sk >= 0], return_counts=True)[1].max() >= 0.6 * sk.size
    assert np.intersect1d(cases["skewed"][1][1], cases["skewed"][2][1]).size >= 4  # the same ids in two scenes
    assert {v[0][0].shape[0] for v in cases.values()} == {1, 5, 256}


@pytest.mark.parametrize("name", ["three_scenes", "skewed", "many_queries"])
def test_exact_cases_equal_the_host_statement_bit_for_bit(exact, name):
    cases, want = exact
    got = _pool(cases[name])
    for b, ((x, seg), g, w) in enumerate(zip(cases[name], got, want[name])):
        assert g.shape == w.shape and g.tobytes() == w.tobytes(), (name, b, int((g != w).sum()))
        ids, counts = np.unique(seg, return_counts=True)
        alone = (seg < 0) | np.isin(seg, ids[counts == 1])
        assert g[:, alone].tobytes() == x[:, alone].tobytes()  # singletons and points without a segment: the input's bits


@pytest.mark.parametrize("name", ["three_scenes", "skewed", "many_queries"])
def test_rounded_cases_within_the_summation_bound(rounded, name):
    """|got - float64 mean| <= k * 2^-23 * mean|x| per (query, run of k points): any-order fp32 summation of k terms errs
    by at most (k - 1) * 2^-24 * sum|x| to first order, the division adds one rounding of the mean (<= 2^-24 * mean|x|);
    divided by k that is k * 2^-24 * mean|x|, and the test allows twice that."""
    cases, want = rounded
    got = _pool(cases[name])
    worst = 0.0
    for b, ((x, seg), g) in enumerate(zip(cases[name], got)):
        x64 = x.astype(np.float64)
        for s in np.unique(seg[seg >= 0]):
            m = np.nonzero(seg == s)[0]
            k = m.size
            mean = x64[:, m].mean(1)
            bound = k * 2.0 ** -23 * np.abs(x64[:, m]).mean(1)
            err = np.abs(g[:, m[0]].astype(np.float64) - mean)
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), (name, b, int(s), k, float((err / bound).max()))
            assert (g[:, m] == g[:, m[:1]]).all() and np.ptp(g[:, m].view(np.uint32), axis=1).max() == 0  # one word per run
        assert g[:, seg < 0].tobytes() == x[:, seg < 0].tobytes()
    print(f"{name}: largest error / bound = {worst:.3f}")


@pytest.mark.parametrize("which", ["exact", "rounded"])
def test_same_bits_again_and_for_each_scene_alone(exact, rounded, which):
    cases, _ = exact if which == "exact" else rounded
    for name, batch in cases.items():
        first, second = _pool(batch), _pool(batch)
        for b, (f, s) in enumerate(zip(first, second)):
            assert f.tobytes() == s.tobytes(), (name, b)
        for b, case in enumerate(batch):
            alone = _pool([case])[0]
            assert alone.tobytes() == first[b].tobytes(), (name, b)
        back = _pool(batch[::-1])[::-1]  # another place in the batch, other neighbours
        for b, (f, s) in enumerate(zip(first, back)):
            assert f.tobytes() == s.tobytes(), (name, b)


def test_arguments(hip):
    from geoformer_amd import _lib, pointops, postprocess

    x = torch.zeros((4, 100), dtype=torch.float32, device="cuda")
    out = torch.empty_like(x)
    seg = torch.zeros(100, dtype=torch.int32, device="cuda")
    keys, order = pointops.segment_pool_keys(seg, [0, 100])
    ws = torch.empty(hip.gf_segment_pool_scratch_bytes(1, 100, 4) // 4 + 1, dtype=torch.int32, device="cuda")

    def call(inp, outp, nq=4, n_fg=100, S=1):
        t = postprocess.segment_scene_table([inp.data_ptr()], [outp.data_ptr()], [0, 100])
        t_d = pointops._table_dev(t, x.device)
        return hip.gf_segment_pool_batched(t_d.data_ptr(), t.ctypes.data, S, nq, keys.data_ptr(), order.data_ptr(), n_fg,
                                           100, ws.data_ptr(), _lib.stream_ptr())

    inval = -1  # GF_ERR_INVALID_ARG
    assert call(x, x) == inval and "out == in" in hip.gf_last_error().decode()
    assert call(x, out, nq=0) == inval and "nq = 0" in hip.gf_last_error().decode()
    assert call(x, out, n_fg=99) == inval  # the table's rows do not add up
    assert hip.gf_segment_pool_batched(None, None, 1, 4, None, None, 100, 100, None, _lib.stream_ptr()) == inval
    assert hip.gf_segment_pool_batched(None, None, 1, 4, None, None, -1, 0, None, _lib.stream_ptr()) == inval
    assert hip.gf_segment_pool_batched(None, None, 0, 4, None, None, 0, 0, None, _lib.stream_ptr()) == 0  # S = 0
    assert hip.gf_segment_pool_batched(None, None, 3, 4, None, None, 0, 0, None, _lib.stream_ptr()) == 0  # n_fg = 0
    assert call(x, out) == 0
    torch.cuda.synchronize()
    assert (out == 0).all()
    # the wrapper: no scene, no foreground, wrong shapes and types
    assert pointops.segment_pool_batched([], seg[:0], [0]) == []
    empty = pointops.segment_pool_batched([x[:, :0].contiguous()], seg[:0], [0, 0])
    assert len(empty) == 1 and empty[0].shape == (4, 0)
    with pytest.raises(RuntimeError):
        pointops.segment_pool_batched([x], seg.long(), [0, 100])
    with pytest.raises(RuntimeError):
        pointops.segment_pool_batched([x], seg[:50].contiguous(), [0, 100])
    with pytest.raises(RuntimeError):
        pointops.segment_pool_batched([x], seg, [0, 50, 100])


# ---- the "segments" key of the eval forward ---------------------------------------------------------------------------
def _to_dev(batch):
    return {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in batch.items()}


def _forward(model, batch, segments=None, seed=21, **kw):
    b = dict(batch)
    if segments is not None:
        b["segments"] = segments
    np.random.seed(seed)
    with torch.no_grad():
        out = model(b, 300, training=False, **kw)
    key = "proposal_scores_per_scene" if kw.get("all_scenes") else "proposal_scores"
    per = out.get(key, ([], [], []))
    if hasattr(per, "get"):
        per = per.get()
    torch.cuda.synchronize()
    return out, per


def _same_proposals(a, b):
    if isinstance(a[0], list):
        assert all(isinstance(x, list) and not x for x in b)
        return 0
    for x, y in zip(a, b):
        assert torch.is_tensor(y) and x.dtype == y.dtype and torch.equal(x, y)
    return a[0].shape[0]


def _segment_consistent(masks, seg_scene, fg_local):
    """Every mask [n, N_b] is constant over each segment's foreground points and empty outside the foreground."""
    m = masks.cpu().numpy()
    is_fg = np.zeros(m.shape[1], bool)
    is_fg[fg_local] = True
    assert not m[:, ~is_fg].any()
    s_fg = seg_scene[fg_local]
    order = np.argsort(s_fg, kind="stable")
    s_sorted = s_fg[order]
    first = np.nonzero(np.concatenate([[True], s_sorted[1:] != s_sorted[:-1]]))[0]
    cols = m[:, fg_local[order]]
    tot = np.add.reduceat(cols, first, axis=1)
    size = np.diff(np.concatenate([first, [s_sorted.size]]))
    ok = (tot == 0) | (tot == size[None, :]) | (s_sorted[first] < 0)[None, :]
    assert ok.all()
    return int((size[s_sorted[first] >= 0] > 1).sum())


def _wiring(model, batch, raws, all_scenes):
    """The checks of one batch under forward(..., all_scenes) with and without defer_proposals."""
    from geoformer_amd import pointops, scene

    cfg = model.cfg
    kw = {"all_scenes": True} if all_scenes else {}
    offs = batch["offsets"].cpu().tolist()
    N = offs[-1]
    plain_out, plain = _forward(model, batch, **kw)
    units = plain if all_scenes else [plain]
    # every point its own segment, and no segment at all: the pooled logits are the raw ones, bit for bit
    for ids in (torch.arange(N, dtype=torch.int32, device="cuda"), torch.full((N,), -1, dtype=torch.int32, device="cuda")):
        _, got = _forward(model, batch, ids, **kw)
        for a, b in zip(units, got if all_scenes else [got]):
            _same_proposals(a, b)
    seg = np.concatenate([scene.grid_segments(r) for r in raws])
    seg_d = torch.from_numpy(seg).cuda()
    out, got = _forward(model, batch, seg_d, **kw)
    _, deferred = _forward(model, batch, seg_d, defer_proposals=True, **kw)
    got_units, def_units = (got, deferred) if all_scenes else ([got], [deferred])
    # the raw logits stay the raw logits
    raw_logits = out["mask_predictions"][-1]["mask_logits"]
    for a, b in zip(raw_logits, plain_out["mask_predictions"][-1]["mask_logits"]):
        assert (a is None and b is None) or torch.equal(a, b)
    assert torch.equal(out["fg_idxs"], plain_out["fg_idxs"])
    # the same kernels on the pooled logits of the public call: the same proposals, bit for bit
    fg = out["fg_idxs"]
    fg_off = np.concatenate([[0], np.cumsum(np.bincount(out["batch_idxs"].cpu().numpy(), minlength=len(offs) - 1))])
    assert (np.diff(fg_off) > 0).all()  # (no scene leaves the batch: the scene ids below are 0..B-1)
    fg_off = fg_off.tolist()
    sem = torch.softmax(out["semantic_scores"][fg], dim=1)
    sem_prob = (sem, sem.t().contiguous())
    th = dict(logit_thresh=0.5, score_thresh=cfg.TEST_SCORE_THRESH, npoint_thresh=cfg.TEST_NPOINT_THRESH)
    cls_logits = out["mask_predictions"][-1]["cls_logits"]
    with torch.no_grad():
        if all_scenes:
            pooled = pointops.segment_pool_batched([l.contiguous() for l in raw_logits], seg_d[fg], fg_off)
            want = model.generate_proposals_batched(pooled, cls_logits, fg, batch["offsets"], fg_off,
                                                    list(range(len(offs) - 1)), len(offs) - 1, sem_prob, **th)
        else:
            pooled = pointops.segment_pool_batched([raw_logits[0].contiguous()], seg_d[fg[:fg_off[1]]], fg_off[:2])
            want = [model.generate_proposal(pooled, cls_logits, fg, batch["offsets"], torch.tensor(fg_off),
                                            sem_prob=sem_prob, **th)]
    torch.cuda.synchronize()
    n = pooled_runs = 0
    fg_h = fg.cpu().numpy()
    for b, (g, d, w) in enumerate(zip(got_units, def_units, want)):
        n += _same_proposals(w, g)
        _same_proposals(g, d)
        if torch.is_tensor(g[0]):
            assert g[2].dtype == torch.int32 and g[2].shape == (g[0].shape[0], offs[b + 1] - offs[b])
            pooled_runs += _segment_consistent(g[2], seg[offs[b]:offs[b + 1]], fg_h[fg_off[b]:fg_off[b + 1]] - offs[b])
    assert n > 0 and pooled_runs > 0  # (the checks above did not pass on empty lists)
    return n


def test_forward_batch_1(calibrated_model):  # noqa: F811
    from geoformer_amd import batch_eval, scene

    model, items = calibrated_model
    raw = items[3][1]
    batch = _to_dev(scene.make_batch([batch_eval.scene_dict(raw)]))
    n = _wiring(model, batch, [raw], all_scenes=False)
    print(f"batch 1: {n} proposals with pooling")
    with pytest.raises(TypeError):
        _forward(model, batch, torch.zeros(raw.shape[0], dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):  # one id per point of the batch
        _forward(model, batch, torch.zeros(raw.shape[0] - 1, dtype=torch.int32, device="cuda"))


def test_forward_all_scenes(calibrated_model):  # noqa: F811
    from geoformer_amd import batch_eval, scene

    model, items = calibrated_model
    raws = [r for _, r in items]
    batch = _to_dev(scene.make_batch([batch_eval.scene_dict(r) for r in raws]))
    n = _wiring(model, batch, raws, all_scenes=True)
    print(f"B = 4: {n} proposals with pooling")


def test_batch_eval_end_to_end(calibrated_model):  # noqa: F811
    from geoformer_amd import batch_eval, scene

    model, items = calibrated_model
    segs = {name: scene.grid_segments(raw) for name, raw in items}
    shape = np.max([b["spatial_shape"] for B in (1, 4) for b in batch_eval.collate_batches(items, B)[1]], axis=0)
    kw = dict(spatial_shape=shape, reserve=False, final_score_thresh=0.0, segments=segs)
    runs = {}
    for B in (1, 4):
        np.random.seed(21)
        runs[B] = list(batch_eval.predict_batches(model, items, B, **kw))
        assert [n for n, *_ in runs[B]] == [n for n, _ in items]
    n = 0
    for (name, raw), (_, c1, s1, m1, p1), (_, c4, s4, m4, p4) in zip(items, runs[1], runs[4]):
        assert torch.is_tensor(c1) == torch.is_tensor(c4), name
        if not torch.is_tensor(c1):
            continue
        n += c1.shape[0]
        assert torch.equal(c1, c4) and torch.equal(m1, m4), (name, int((m1 != m4).sum()) if m1.shape == m4.shape else -1)
        # segment-consistent: a member of the mask brings its whole segment's foreground (the mask's own support tells
        # which points are foreground: no non-foreground point is ever in)
        m = m4.cpu().numpy()
        seg = segs[name]
        for row in m:
            inside = np.unique(seg[(row != 0) & (seg >= 0)])
            assert not np.isin(seg[(row == 0) & m.any(0)], inside).any()
    assert n > 0
    np.random.seed(21)
    ap, avgs = batch_eval.evaluate(model, items, 4, classes=model.cfg.cvfold, **kw)
    assert np.asarray(ap).ndim == 2 and "all_ap" in avgs
    # the AP table is the one of the masks checked above
    from geoformer_amd import evaluation

    ev = evaluation.InstanceEvaluator(classes=model.cfg.cvfold)
    for (name, raw), (_, cls, sc, masks, pick) in zip(items, runs[4]):
        if torch.is_tensor(cls):
            r = torch.as_tensor(raw, device="cuda")
            ev.add_scene(name, evaluation.gt_ids_from_labels(r[:, 6].long(), r[:, 7].long()),
                         evaluation.benchmark_label_ids(cls, model.cfg.cvfold), sc, masks, pick)
    assert np.array_equal(ap, ev.evaluate()[0], equal_nan=True)
    # without the keyword the loop is what it was: no "segments" in the batches
    assert all("segments" not in b for b in batch_eval.collate_batches(items, 4)[1])
