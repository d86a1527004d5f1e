"""GPU: the batched eval forward (forward(..., all_scenes=True)) and its post-processing kernels (csrc/batch_post.hip)
against the one-scene paths: matrix NMS per scene, generate_proposal of B = 1, B = 1 forwards of each scene under the
batch's voxel grid, and the B = 1 evaluation loop."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _to_dev(batch):
    return {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in batch.items()}


# ---- matrix NMS ---------------------------------------------------------------------------------------------------
def _nms_case(rng, n, N, n_cls=3):
    """n overlapping proposals over N points: random runs of the points (so that IoUs spread over [0, 1]), distinct
    scores, a few categories."""
    masks = np.zeros((n, N), np.int32)
    for i in range(n):
        ln = int(rng.integers(N // 50 + 1, N // 4 + 2))
        s = int(rng.integers(0, N - ln + 1))
        masks[i, s:s + ln] = 1
        if i % 3 == 0 and n > 0:  # holes
            masks[i, s + ln // 3:s + ln // 3 + ln // 10] = 0
    scores = ((rng.permutation(n) + 1) / (n + 1)).astype(np.float32)
    cats = rng.integers(0, n_cls, n).astype(np.int64)
    return masks, scores, cats


def _decayed(masks, scores, cats, kernel, sigma=2.0):
    """Decayed score of every proposal (float64 restatement of util/utils_3d.py:95-141), by original index."""
    n = len(scores)
    ixs = np.argsort(-scores, kind="stable")
    m = masks[ixs].astype(np.float64)
    inter = m @ m.T
    d = np.diag(inter)
    iou = inter / (d[:, None] + d[None, :] - inter)
    c = cats[ixs]
    lab = np.triu((c[:, None] == c[None, :]).astype(np.float64), 1)
    comp = (iou * lab).max(0)
    dec = iou * lab
    if kernel == "gaussian":
        coef = (np.exp(-sigma * dec ** 2) / np.exp(-sigma * comp[:, None] ** 2)).min(0)
    else:
        coef = ((1 - dec) / (1 - comp[:, None])).min(0)
    out = np.empty(n)
    out[ixs] = scores[ixs] * coef
    return out


@pytest.mark.parametrize("kernel", ["gaussian", "linear"])
@pytest.mark.parametrize("thresh", [0.05, 0.5])
def test_matrix_nms_batched_equals_per_scene(hip, kernel, thresh):
    from geoformer_amd import postprocess

    rng = np.random.default_rng(5)
    sizes = [(0, 1000), (1, 5000), (37, 20000), (128, 150000), (256, 60000)]
    cases = [_nms_case(rng, n, N) for n, N in sizes]
    masks = [torch.from_numpy(m).cuda() if m.shape[0] else [] for m, _, _ in cases]
    scores = [torch.from_numpy(s).cuda() if len(s) else [] for _, s, _ in cases]
    cats = [torch.from_numpy(c).cuda() if len(c) else [] for _, _, c in cases]
    picks = postprocess.matrix_nms_batched(masks, scores, cats, kernel=kernel, final_score_thresh=thresh)
    assert len(picks) == len(sizes)
    near = 0
    for (m, s, c), mt, st, ct, got in zip(cases, masks, scores, cats, picks):
        got = got.cpu().numpy().tolist()
        if len(s) == 0:
            assert got == []
            continue
        want = postprocess.matrix_non_max_suppression(mt, st, ct, kernel=kernel,
                                                      final_score_thresh=thresh).cpu().numpy().tolist()
        if got != want:
            dec = _decayed(m, s, c, kernel)
            diff = set(got) ^ set(want)
            assert all(abs(dec[i] - thresh) <= 1e-5 * thresh for i in diff), (kernel, thresh, len(s), sorted(diff))
            near += len(diff)
            assert [i for i in got if i not in diff] == [i for i in want if i not in diff]
        assert len(got) > 0 or thresh > 0.05
    print(f"matrix NMS {kernel} thresh {thresh}: {near} pick(s) within 1e-5 of the threshold differ")


def test_matrix_nms_batched_ties_by_ascending_index(hip):
    from geoformer_amd import postprocess

    m = torch.zeros((4, 256), dtype=torch.int32, device="cuda")
    for i in range(4):
        m[i, i * 64:(i + 1) * 64] = 1  # disjoint: nothing decays
    s = torch.tensor([0.7, 0.9, 0.7, 0.7], device="cuda")
    c = torch.zeros(4, dtype=torch.int64, device="cuda")
    (p,) = postprocess.matrix_nms_batched([m], [s], [c])
    assert p.cpu().tolist() == [1, 0, 2, 3]


# ---- proposals ----------------------------------------------------------------------------------------------------
def test_batched_proposals_equal_generate_proposal(hip):
    from geoformer_amd.model import GeoFormer, load_config

    m = GeoFormer(load_config("test_geoformer_scannet.yaml"))
    rng = np.random.default_rng(3)
    nq, ncls = 64, 20
    npts = [9000, 15000, 4000, 30000]
    n_fg = [3000, 7000, 1500, 12000]
    logits, fg_local, cls_l, sems = [], [], [], []
    for k, (N, nf) in enumerate(zip(npts, n_fg)):
        lg = rng.normal(0, 3, (nq, nf)) + rng.normal(0, 2, (nq, 1))
        if k == 2:
            lg[:] = -10.0  # a scene without proposals
        logits.append(torch.tensor(lg, dtype=torch.float32, device="cuda"))
        fg_local.append(torch.tensor(np.sort(rng.choice(N, nf, replace=False)), dtype=torch.int64, device="cuda"))
        cls_l.append(torch.tensor(rng.normal(0, 2, (nq, ncls)), dtype=torch.float32, device="cuda"))
        sems.append(torch.softmax(torch.tensor(rng.normal(0, 1, (nf, ncls)), dtype=torch.float32), 1).cuda())
    po = np.concatenate([[0], np.cumsum(npts)])
    fo = np.concatenate([[0], np.cumsum(n_fg)]).tolist()
    fg_all = torch.cat([f + int(po[k]) for k, f in enumerate(fg_local)])
    sem_all = torch.cat(sems)
    with torch.no_grad():
        got = m.generate_proposals_batched(logits, torch.stack(cls_l), fg_all,
                                           torch.tensor(po, dtype=torch.int32), fo, list(range(4)), 4,
                                           (sem_all, sem_all.t().contiguous()), score_thresh=0.5, npoint_thresh=100)
        n_props = 0
        for k in range(4):
            want = m.generate_proposal([logits[k]], cls_l[k][None], fg_local[k], torch.tensor([0, npts[k]]),
                                       torch.tensor([0, n_fg[k]]), sem_prob=(sems[k], sems[k].t().contiguous()),
                                       score_thresh=0.5, npoint_thresh=100)
            if isinstance(want[0], list):
                assert all(isinstance(x, list) and not x for x in got[k]), k
                continue
            cw, sw, mw = want
            cg, sg, mg = got[k]
            n_props += cw.shape[0]
            assert torch.equal(cw, cg) and torch.equal(mw, mg) and mg.shape == (cw.shape[0], npts[k])
            assert ((sg - sw).abs() <= 1e-6 * sw.abs()).all()
        assert isinstance(got[2][0], list) and n_props > 0


# ---- the model ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(hip):
    from geoformer_amd.model import GeoFormer, load_config
    from tests.util import synthetic_state_dict

    m = GeoFormer(load_config("test_geoformer_scannet.yaml"))
    m.load_state_dict(synthetic_state_dict(m.state_dict(), 0))
    m.cuda()
    m.eval()  # (returns None, like the reference's train())
    return m


def _scenes():
    from geoformer_amd import scene

    return [scene.make_small_scene(n, sd) for n, sd in ((6000, 5), (24000, 6), (12000, 7))]


def _batches(scenes):
    from geoformer_amd import scene

    batch = scene.make_batch(scenes)
    singles = []
    for sc in scenes:
        b = scene.make_batch([sc])
        b["spatial_shape"] = batch["spatial_shape"].copy()  # the batch's grid: the same problem per scene
        singles.append(_to_dev(b))
    return _to_dev(batch), singles


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


DIFFERING = {"points": 0, "proposals": 0}


def _compare(single, batched, what):
    """Scene result of a B = 1 forward against the batched forward's entry.  Classes exactly; masks and scores to the
    tolerances of tests/test_gpu_model.py: the backbone of a 3-scene batch sums some rows in another order than the
    one-scene forward (its launches are sized by the batch's voxel count), so a point whose mask logit lies within
    rounding of the 0.5 cut may flip.  The differences are counted in DIFFERING and printed."""
    if isinstance(single[0], list):
        assert all(isinstance(x, list) and not x for x in batched), what
        return 0
    c1, s1, m1 = single
    c2, s2, m2 = batched
    assert torch.equal(c1, c2), what
    assert m1.shape == m2.shape and m1.dtype == m2.dtype == torch.int32, what
    d = (m1 != m2).sum(1).cpu().numpy()
    DIFFERING["points"] += int(d.sum())
    DIFFERING["proposals"] += int((d > 0).sum())
    assert d.max() <= 3 and (d > 0).mean() < 0.1, (what, int(d.sum()), int((d > 0).sum()))
    assert (s1 - s2).abs().max().item() < 1e-4, what
    print(f"{what}: {c1.shape[0]} proposals, {int((d > 0).sum())} differ in {int(d.sum())} point(s); "
          f"max score difference {(s1 - s2).abs().max().item():.3g}")
    return c1.shape[0]


def _run_all(m, batch, singles, seed=11, defer=False):
    np.random.seed(seed)
    with torch.no_grad():
        out = m(batch, 300, training=False, all_scenes=True, defer_proposals=defer)
        per = out["proposal_scores_per_scene"]
        if defer:
            assert hasattr(per, "get")
            per = per.get()
    st_b = np.random.get_state()
    np.random.seed(seed)
    with torch.no_grad():
        ref = []
        for b in singles:
            o = m(b, 300, training=False)
            ref.append(o.get("proposal_scores", ([], [], [])))
    st_s = np.random.get_state()
    torch.cuda.synchronize()
    return out, per, ref, st_b, st_s


@pytest.mark.parametrize("defer", [False, True], ids=["sync", "deferred"])
def test_all_scenes_forward_equals_single_scene_forwards(model, defer):
    batch, singles = _batches(_scenes())
    out, per, ref, st_b, st_s = _run_all(model, batch, singles, defer=defer)
    assert len(per) == 3 and _same_state(st_b, st_s)
    n = sum(_compare(r, p, k) for k, (r, p) in enumerate(zip(ref, per)))
    assert n > 0
    for (c, s, mk), sc in zip(per, _scenes()):
        if not isinstance(c, list):
            assert mk.dtype == torch.int32 and mk.shape[1] == sc["xyz"].shape[0]


def test_scene_without_foreground_does_not_stop_the_batch(model, monkeypatch):
    from geoformer_amd import pointops

    batch, singles = _batches(_scenes())
    empty_scene = 1
    orig = pointops.select_foreground

    def no_fg_in_scene(scores, cls, equal, locs, batch_idxs, *a, **k):
        scores = scores.clone()
        scores[batch_idxs == empty_scene, 0] = 1e4  # every point of the scene predicted as class 0 (background)
        return orig(scores.contiguous(), cls, equal, locs, batch_idxs, *a, **k)

    np.random.seed(11)
    with torch.no_grad():
        plain = [model(b, 300, training=False).get("proposal_scores", ([], [], [])) for b in (singles[0], singles[2])]
    st_s = np.random.get_state()
    for defer in (False, True):
        monkeypatch.setattr(pointops, "select_foreground", no_fg_in_scene)
        np.random.seed(11)
        with torch.no_grad():
            out = model(batch, 300, training=False, all_scenes=True, defer_proposals=defer)
            per = out["proposal_scores_per_scene"]
            per = per.get() if defer else per
        st_b = np.random.get_state()
        monkeypatch.setattr(pointops, "select_foreground", orig)
        assert out["mask_predictions"] is not None and len(per) == 3
        assert all(isinstance(x, list) and not x for x in per[empty_scene])
        _compare(plain[0], per[0], "scene 0")
        _compare(plain[1], per[2], "scene 2")
        assert _same_state(st_b, st_s)  # the empty scene drew nothing, like a forward of it alone


def test_default_forward_unchanged(model):
    batch, singles = _batches(_scenes())
    np.random.seed(11)
    with torch.no_grad():
        plain = model(batch, 300, training=False)
    np.random.seed(11)
    with torch.no_grad():
        per = model(batch, 300, training=False, all_scenes=True)["proposal_scores_per_scene"]
    assert "proposal_scores_per_scene" not in plain
    _compare(plain["proposal_scores"], per[0], "B=3 default: scene 0")
    # B = 1: the new keyword changes nothing of the forward
    outs = []
    for flag in (False, True):
        np.random.seed(4)
        with torch.no_grad():
            o = model(singles[1], 300, training=False, all_scenes=flag)
        outs.append(o)
    a, b = outs
    assert torch.equal(a["semantic_scores"], b["semantic_scores"]) and torch.equal(a["fg_idxs"], b["fg_idxs"])
    ma, mb = a["mask_predictions"][-1], b["mask_predictions"][-1]
    assert torch.equal(ma["cls_logits"], mb["cls_logits"]) and torch.equal(ma["mask_logits"][0], mb["mask_logits"][0])
    ps, (pb,) = a["proposal_scores"], b["proposal_scores_per_scene"]
    assert not isinstance(ps[0], list)
    assert torch.equal(ps[0], pb[0]) and torch.equal(ps[1], pb[1]) and torch.equal(ps[2], pb[2])


# ---- end to end ---------------------------------------------------------------------------------------------------
def test_evaluate_batched_equals_single_scene_loop(model):
    from geoformer_amd import batch_eval, scene

    items = [(f"scene{i:02d}", scene.make_raw_scene(6000 + 2500 * i, 40 + i, n_boxes=1, room=(1.6, 1.6, 0.6)))
             for i in range(8)]
    _, hb = batch_eval.collate_batches(items, 1)
    shape = np.max([b["spatial_shape"] for b in hb], axis=0)  # one grid for both loops
    res = {}
    for B in (4, 1):
        np.random.seed(21)
        res[B] = batch_eval.evaluate(model, items, B, classes=0, spatial_shape=shape, final_score_thresh=0.0)
        np.random.seed(21)
        got = list(batch_eval.predict_batches(model, items, B, spatial_shape=shape, reserve=False,
                                              final_score_thresh=0.0))
        proposals = sum(int(c.shape[0]) for _, c, *_ in got if torch.is_tensor(c))
        picked = sum(int(p.numel()) for *_, p in got)
        print(f"B={B}: {proposals} proposals, {picked} picks over {len(got)} scenes")
        assert picked > 0
    a4, a1 = res[4][1], res[1][1]
    for key in ("all_ap", "all_ap_50%", "all_ap_25%"):
        assert a4[key] == a1[key] or (np.isnan(a4[key]) and np.isnan(a1[key])), (key, a4[key], a1[key])
