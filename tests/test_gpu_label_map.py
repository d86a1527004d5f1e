"""GPU: the scene-labelling kernels (csrc/label_map.hip) against the numpy path of postprocess.label_points and the
float64 restatement of tests/test_label_map_host.py; batched against per-scene; batch_eval.label_batches end to end."""
import numpy as np
import pytest
import torch

from tests.test_label_map_host import SIZES, all_cases, check_against, label_case, restated

pytestmark = pytest.mark.gpu

INT_COLS = ("count", "owned", "label_id", "index", "kept")


def _dev(case, mask_dtype=torch.int32):
    masks, scores, label_ids, pick, xyz = case
    if masks.shape[0] == 0:  # a scene without proposals, as predict_batches yields it
        return [], [], [], torch.zeros(0, dtype=torch.int64, device="cuda"), torch.from_numpy(xyz).cuda()
    return (torch.from_numpy(masks).cuda().to(mask_dtype), torch.from_numpy(scores).cuda(),
            torch.from_numpy(label_ids).cuda(), torch.from_numpy(pick).cuda(), torch.from_numpy(xyz).cuda())


def _bit_equal(a, b):
    """Two host SceneLabels, every array bit for bit."""
    assert np.array_equal(a.owner, b.owner) and np.array_equal(a.ids, b.ids)
    for k, x, y in zip(a.table._fields, a.table, b.table):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k


def _check(got, case, min_score):
    """Device result against the numpy path (integers, boxes, scores bit-equal) and the float64 centroid."""
    from geoformer_amd import postprocess

    got = got.to_host()
    ref = postprocess.label_points(*case, min_score)
    assert got.owner.dtype == np.int32 and got.ids.dtype == np.int32
    assert np.array_equal(got.owner, ref.owner) and np.array_equal(got.ids, ref.ids)
    for k in INT_COLS + ("score", "box_min", "box_max"):
        x, y = getattr(got.table, k), getattr(ref.table, k)
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k
    return check_against(got, restated(*case, min_score), case[4])


@pytest.mark.parametrize("mask_dtype", [torch.int32, torch.bool, torch.uint8])
@pytest.mark.parametrize("min_score", [0.09, 0.5])
def test_kernel_equals_numpy_path_single_and_batched(hip, min_score, mask_dtype):
    from geoformer_amd import postprocess

    cases = all_cases()
    devs = [_dev(c, mask_dtype) for c in cases]
    singles = [postprocess.label_points(*d, min_score) for d in devs]
    worst = 0.0
    for (n, N), case, got in zip(SIZES, cases, singles):
        assert got.owner.is_cuda and got.owner.shape == (N,) and got.table.count.shape == ((3 * n + 3) // 4,)
        worst = max(worst, _check(got, case, min_score))
    print(f"centroid error, worst scene: {worst:.2f} fp32 eps of max|xyz| (bound 32)")
    batched = postprocess.label_points_batched(*[list(x) for x in zip(*devs)], min_score)
    again = postprocess.label_points_batched(*[list(x) for x in zip(*devs)], min_score)
    assert len(batched) == len(cases)
    for case, one, b, a in zip(cases, singles, batched, again):
        _check(b, case, min_score)
        _bit_equal(b.to_host(), one.to_host())  # batched == per scene, table included
        _bit_equal(b.to_host(), a.to_host())  # and the same from call to call


def test_empty_scene_alone(hip):
    from geoformer_amd import postprocess

    xyz = torch.zeros((700, 3), device="cuda")
    lab = postprocess.label_points([], [], [], torch.zeros(0, dtype=torch.int64), xyz).to_host()
    assert (lab.owner == -1).all() and (lab.ids == 0).all() and lab.owner.shape == (700,)
    assert all(len(c) == 0 for c in lab.table)


@pytest.mark.parametrize("n,N,p", [(9, 4097, None), (9, 8191, None), (3, 63, None), (6, 12345, 1), (1024, 4096, 1024)])
def test_ragged_sizes_and_pick_limits(hip, n, N, p):
    """N off the multiples of 64 and of the 4096-point chunk; p = 1; p = GF_NMS_MAX_N."""
    from geoformer_amd import postprocess

    assert postprocess.NMS_MAX_N == 1024 and postprocess.LBL_CHUNK == 4096
    masks, scores, label_ids, pick, xyz = label_case(np.random.default_rng(100 + N), n, N)
    pick = np.argsort(-scores, kind="stable").astype(np.int64)[:p] if p else pick
    case = (masks, scores, label_ids, pick, xyz)
    for min_score in (0.09, 0.5):
        _check(postprocess.label_points(*_dev(case), min_score), case, min_score)


def test_more_picks_than_the_limit_is_an_error(hip):
    from geoformer_amd import postprocess

    m = torch.ones((2, 128), dtype=torch.int32, device="cuda")
    s = torch.ones(2, device="cuda")
    with pytest.raises(ValueError):
        postprocess.label_points(m, s, torch.ones(2, dtype=torch.int64, device="cuda"),
                                 torch.zeros(1025, dtype=torch.int64, device="cuda"), torch.zeros((128, 3), device="cuda"))


@pytest.fixture(scope="module")
def calibrated_model(hip, oracle):
    from geoformer_amd import batch_eval, scene
    from geoformer_amd.model import GeoFormer, load_config
    from tests.util import calibrated_benchmark_state

    items = [(f"scene{i:02d}", scene.make_raw_scene(6000 + 2500 * i, 40 + i, n_boxes=1, room=(1.6, 1.6, 0.6)))
             for i in range(4)]
    host = scene.make_batch([batch_eval.scene_dict(items[3][1])])
    state, _ = calibrated_benchmark_state(host)
    m = GeoFormer(load_config("test_geoformer_scannet.yaml"))
    m.load_state_dict(state)
    m.cuda()
    m.eval()
    return m, items


@pytest.mark.parametrize("batch_size", [1, 4])
def test_label_batches_end_to_end(calibrated_model, batch_size):
    from geoformer_amd import batch_eval, evaluation, postprocess

    model, items = calibrated_model
    _, hb = batch_eval.collate_batches(items, 1)
    shape = np.max([b["spatial_shape"] for b in hb], axis=0)
    kw = dict(spatial_shape=shape, reserve=False, final_score_thresh=0.0)
    np.random.seed(21)
    preds = list(batch_eval.predict_batches(model, items, batch_size, **kw))
    np.random.seed(21)
    plain = list(batch_eval.label_batches(model, items, batch_size, **kw))
    np.random.seed(21)
    with_masks = list(batch_eval.label_batches(model, items, batch_size, keep_masks=True, min_score=0.0, **kw))
    assert [n for n, _ in plain] == [n for n, _ in items] == [n for n, _ in with_masks]
    picked = labelled = 0
    top = 0.0
    for (name, raw), (_, cls, sc, masks, pick), (_, lab), (_, labm) in zip(items, preds, plain, with_masks):
        xyz = raw[:, :3].astype(np.float32)
        assert lab.masks is None and isinstance(lab.ids, np.ndarray) and isinstance(lab.table.count, np.ndarray)
        if torch.is_tensor(cls):
            host = (masks.cpu().numpy(), sc.cpu().numpy(),
                    evaluation.benchmark_label_ids(cls, model.cfg.cvfold).cpu().numpy(), pick.cpu().numpy(), xyz)
        else:
            host = ([], [], [], np.zeros(0, np.int64), xyz)
        for got, ms in ((lab, postprocess.MIN_SCORE), (labm, 0.0)):
            ref = postprocess.label_points(*host, ms)
            assert np.array_equal(got.owner, ref.owner) and np.array_equal(got.ids, ref.ids)
            for k in INT_COLS + ("score", "box_min", "box_max"):
                assert np.array_equal(getattr(got.table, k), getattr(ref.table, k)), (name, k)
            if ref.table.centroid.size:
                bound = 32 * np.finfo(np.float32).eps * float(np.abs(xyz).max())
                assert np.abs(got.table.centroid.astype(np.float64) - ref.table.centroid).max() <= bound
        want_masks = host[0][host[3]] if len(host[3]) else np.zeros((0, xyz.shape[0]), np.int32)
        assert labm.masks.shape == (len(host[3]), xyz.shape[0]) and np.array_equal(labm.masks, want_masks)
        picked += len(host[3])
        labelled += int((labm.owner >= 0).sum())
        top = max(top, float(host[1].max()) if len(host[1]) else 0.0)
    # (the synthetic weights score low: the default threshold may keep nothing, min_score = 0 keeps every pick)
    print(f"B={batch_size}: {picked} picks, best score {top:.3f}, {labelled} points labelled at min_score 0 over "
          f"{len(items)} scenes")
    assert picked > 0 and labelled > 0
