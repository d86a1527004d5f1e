"""gf_instance_overlaps (csrc/inst_eval.hip) against an exact numpy count, and the GPU path of
geoformer_amd.evaluation.InstanceEvaluator against the reference golden and against its own host path."""
import os

import numpy as np
import pytest
import torch

from geoformer_amd import evaluation as E

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scannet_eval.npz")
ALL = np.asarray(E.VALID_CLASS_IDS, dtype=np.int64)


def make_gt(rng, N, G):
    """gt_ids [N] with up to G instances of the 18 classes, the rest void: unannotated, wall / floor, negative ids."""
    keys = rng.choice(len(ALL) * 1000, size=G, replace=False) if G else np.zeros(0, np.int64)
    inst = ALL[keys // 1000] * 1000 + keys % 1000
    void = np.array([0, 0, 1003, 2001, -1, -3001, -36000, 40007])
    gt = void[rng.integers(0, len(void), N)]
    if G:
        on = rng.random(N) < 0.85
        gt[on] = inst[rng.integers(0, G, int(on.sum()))]
    return gt.astype(np.int64)


def make_masks(rng, n, N, density=0.3):
    m = np.where(rng.random((n, N)) < density, rng.choice(np.array([1, 2, -7, 1 << 20]), (n, N)), 0)
    return m.astype(np.int32)


def check(masks, gt, cls, rows=None):
    from geoformer_amd import pointops

    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    gid, gcnt, inter = pointops.instance_overlaps(d(masks), d(gt), d(cls.astype(np.int32)),
                                                  None if rows is None else d(rows.astype(np.int32)))
    rid, rcnt, rinter = E.scene_overlaps_host(masks, gt, cls, rows)
    assert gid.cpu().numpy().tolist() == rid.tolist()
    assert gcnt.cpu().numpy().tolist() == rcnt.tolist()
    assert inter.shape == rinter.shape
    assert (inter.cpu().numpy() == rinter).all()
    return rid.shape[0]


@pytest.mark.parametrize("N", [1, 63, 64, 65, 150_269, 400_000])
@pytest.mark.parametrize("G", [0, 1, 50, 2000])
def test_overlaps_exact(hip, N, G):
    rng = np.random.default_rng(N * 7 + G)
    gt = make_gt(rng, N, G)
    masks = make_masks(rng, 40, N)
    got_g = check(masks, gt, ALL)
    assert got_g == len(np.unique(gt[np.isin(gt // 1000, ALL)]))
    rows = rng.permutation(40)[:17]  # an unsorted subset, with a repeat
    rows[3] = rows[11]
    check(masks, gt, ALL, rows)


@pytest.mark.parametrize("N", [65, 150_269])
@pytest.mark.parametrize("n", [0, 1, 256])
def test_overlaps_row_counts(hip, N, n):
    rng = np.random.default_rng(N + n)
    gt = make_gt(rng, N, 40)
    masks = make_masks(rng, n, N, 0.05)
    check(masks, gt, ALL)
    check(masks, gt, ALL, rng.integers(0, max(n, 1), 3) if n else np.zeros(0, np.int64))


def test_overlaps_fold_and_void_scene(hip):
    rng = np.random.default_rng(3)
    gt = make_gt(rng, 20_000, 300)
    masks = make_masks(rng, 12, 20_000)
    check(masks, gt, np.asarray(E.FOLD_CLASS_IDS[1], dtype=np.int64))
    void = np.where(rng.random(20_000) < 0.5, 0, 2005).astype(np.int64)  # nothing of the class set
    assert check(masks, void, ALL) == 0
    check(masks, gt, np.array([39, 3, 24], dtype=np.int64))  # class ids in any order: instances still ascend by id


def test_overlaps_capacity_reported_not_overrun(hip):
    from geoformer_amd import _lib
    from geoformer_amd._lib import ptr, stream_ptr

    rng = np.random.default_rng(5)
    N, n, G = 30_000, 8, 120
    gt = torch.from_numpy(make_gt(rng, N, G)).cuda()
    G = len(np.unique(gt.cpu().numpy()[np.isin(gt.cpu().numpy() // 1000, ALL)]))
    masks = torch.from_numpy(make_masks(rng, n, N)).cuda()
    cls = torch.from_numpy(ALL.astype(np.int32)).cuda()
    lib = _lib.load()
    max_gt, pad, sentinel = 64, 4096, -12345
    d_G = torch.full((1,), sentinel, dtype=torch.int32, device="cuda")
    gt_id = torch.full((max_gt + pad,), sentinel, dtype=torch.int64, device="cuda")
    gt_count = torch.full((max_gt + pad,), sentinel, dtype=torch.int32, device="cuda")
    inter = torch.full((n * (max_gt + 1) + pad,), sentinel, dtype=torch.int32, device="cuda")
    scratch = torch.empty(lib.gf_instance_overlaps_scratch_bytes(N, len(ALL)) // 4 + 1, dtype=torch.int32, device="cuda")
    _lib.check(lib.gf_instance_overlaps(ptr(masks), n, N, None, n, ptr(gt), ptr(cls), len(ALL), max_gt, ptr(scratch),
                                        ptr(d_G), ptr(gt_id), ptr(gt_count), ptr(inter), stream_ptr()))
    torch.cuda.synchronize()
    assert int(d_G) == G > max_gt
    assert (gt_id[max_gt:] == sentinel).all() and (gt_count[max_gt:] == sentinel).all()
    assert (inter[n * (max_gt + 1):] == sentinel).all()
    # ... and the Python layer grows the tables and repeats the call
    from geoformer_amd import pointops

    gid, gcnt, it = pointops.instance_overlaps(masks, gt, cls, max_gt=16)
    rid, rcnt, rit = E.scene_overlaps_host(masks.cpu().numpy(), gt.cpu().numpy(), ALL)
    assert (gid.cpu().numpy() == rid).all() and (gcnt.cpu().numpy() == rcnt).all() and (it.cpu().numpy() == rit).all()


def test_bad_arguments_rejected(hip):
    from geoformer_amd import _lib

    lib = _lib.load()
    assert lib.gf_instance_overlaps(None, 0, 10, None, 0, None, None, 0, 8, None, None, None, None, None, None) < 0
    assert b"gf_instance_overlaps" in lib.gf_last_error()


def _golden_scenes():
    z = np.load(GOLDEN)
    out = []
    for i, name in enumerate(z["scene_names"]):
        gt = z[f"s{i}_gt_ids"]
        off, pts = z[f"s{i}_mask_offsets"], z[f"s{i}_mask_points"]
        masks = np.zeros((len(off) - 1, gt.shape[0]), dtype=np.int32)
        for r in range(len(off) - 1):
            masks[r, pts[off[r]:off[r + 1]]] = 1
        out.append((str(name), gt, masks, z[f"s{i}_labels"], z[f"s{i}_scores"]))
    return z, out


@pytest.mark.parametrize("which,classes", [("0", 0), ("1", 1), ("all", "all")])
def test_evaluator_gpu_path_matches_golden(hip, which, classes):
    z, scenes = _golden_scenes()
    ev = E.InstanceEvaluator(classes=classes)
    for name, gt, masks, labels, scores in scenes:
        ev.add_scene(name, torch.from_numpy(gt).cuda(), torch.from_numpy(labels).cuda(), torch.from_numpy(scores).cuda(),
                     torch.from_numpy(masks).cuda())
    ap, _ = ev.evaluate()
    want = z[f"{which}_ap"][0]
    assert (np.isnan(ap) == np.isnan(want)).all()
    ok = ~np.isnan(want)
    assert np.abs(ap[ok] - want[ok]).max() <= 1e-12


def test_end_to_end_forward_nms_evaluation(hip):
    """GeoFormer forward (proposal threshold 0, as bench.py's with-instances leg) -> matrix NMS -> evaluation: the GPU
    evaluator on the device masks equals the host evaluator on the copied masks, bit for bit."""
    from geoformer_amd import postprocess, scene
    from geoformer_amd.model import GeoFormer, load_config
    from tests.util import synthetic_state_dict

    m = GeoFormer(load_config("test_geoformer_scannet.yaml"))
    m.load_state_dict(synthetic_state_dict(m.state_dict(), 0))
    m.cuda()
    m.eval()
    m.cfg.TEST_SCORE_THRESH = 0.0
    ev_gpu, ev_host = E.InstanceEvaluator(classes=0), E.InstanceEvaluator(classes=0)
    n_pred = 0
    for s, (npts, seed) in enumerate([(40_000, 11), (60_000, 12)]):
        sc = scene.make_scene(npts, seed)
        batch = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in scene.make_batch([sc]).items()}
        np.random.seed(100 + s)
        with torch.no_grad():
            out = m(batch, 300, training=False)
        ps = out["proposal_scores"]
        cls_final, scores_final, masks_final = ps.get() if hasattr(ps, "get") else ps
        pick = postprocess.matrix_non_max_suppression(masks_final, scores_final, cls_final, final_score_thresh=0.0)
        labels = E.benchmark_label_ids(cls_final, 0)
        gt = E.gt_ids_from_labels(torch.from_numpy(sc["label"]).cuda(), torch.from_numpy(sc["instance"]).cuda())
        ev_gpu.add_scene(f"s{s}", gt, labels, scores_final, masks_final, pick=pick)
        ev_host.add_scene(f"s{s}", gt.cpu().numpy(), labels.cpu().numpy(), scores_final.cpu().numpy(),
                          masks_final.cpu().numpy(), pick=pick.cpu().numpy())
        n_pred += int(pick.shape[0])
    assert n_pred > 0
    for a, b in zip(ev_gpu.scenes, ev_host.scenes):
        for k in ("gt_id", "gt_count", "label", "conf", "count", "void", "inter"):
            assert np.array_equal(getattr(a, k), getattr(b, k)), k
    ap_g, avg_g = ev_gpu.evaluate()
    ap_h, avg_h = ev_host.evaluate()
    assert np.array_equal(ap_g, ap_h, equal_nan=True)
    assert (np.isnan(ap_g) == np.isnan(ap_h)).all()
