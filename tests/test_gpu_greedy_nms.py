"""GPU: the greedy NMS kernels (csrc/batch_post.hip: k_bp_greedy_ious / k_bp_greedy_nms) against the picks the
reference's non_max_suppression_gpu gave on the same inputs (tests/golden/greedy_nms.npz).  Picks are integers: every
comparison is exact.  n = 1, 2, 3, 65 (crosses a wave), 200 and 1024 (the capacity) are the smallest sizes at which the
ranking, the lane masks and the walk over several alive words can each go wrong."""
import numpy as np
import pytest
import torch

from tests.greedy_nms_cases import case_ids, cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", case_ids())
def test_cuda_path_equals_reference(hip, name):
    from geoformer_amd.postprocess import non_max_suppression_gpu

    c = cases()[name]
    ious, scores = c.ious.cuda(), c.scores.cuda()
    for thr, want in zip(c.thresholds, c.picks):
        got = non_max_suppression_gpu(ious, scores, thr)
        assert got.dtype == torch.int64 and got.device == scores.device
        assert got.cpu().tolist() == want, (name, thr)


SCENES = ["empty", "one", "chain3", "r65", "r200", "r1024"]  # (n, N) = (0, 100), (1, 64), (3, 64), (65, 700), ...


@pytest.fixture(scope="module")
def scene_tensors(hip):
    out = {}
    for name in SCENES[1:]:
        c = cases()[name]
        out[name] = (torch.from_numpy(c.masks.astype(np.int32)).cuda(), c.scores.cuda())
    return out


@pytest.mark.parametrize("order", [SCENES, SCENES[1:3] + ["empty"] + SCENES[3:], SCENES[1:] + ["empty"]],
                         ids=["empty-first", "empty-middle", "empty-last"])
def test_batched_equals_per_scene_reference(scene_tensors, order):
    from geoformer_amd.postprocess import greedy_nms_batched

    masks = [scene_tensors[k][0] if k != "empty" else [] for k in order]
    scores = [scene_tensors[k][1] if k != "empty" else [] for k in order]
    for k, thr in enumerate((0.05, 0.3, 0.5)):
        picks = greedy_nms_batched(masks, scores, thr)
        assert len(picks) == len(order)
        for name, got in zip(order, picks):
            assert got.dtype == torch.int64
            if name == "empty":
                assert got.numel() == 0
                continue
            c = cases()[name]
            assert c.thresholds[k] == thr
            assert got.cpu().tolist() == c.picks[k], (name, thr)


def test_equal_scores_by_ascending_index_and_reproducible(scene_tensors):
    from geoformer_amd.postprocess import greedy_nms_batched, non_max_suppression_gpu

    c = cases()["r200"]
    scores = torch.floor(c.scores * 8) / 8  # eight levels: runs of about 25 equal scores
    assert scores.unique().numel() <= 9
    want = non_max_suppression_gpu(c.ious, scores, 0.3).tolist()
    assert 2 <= len(want) < 100
    a = non_max_suppression_gpu(c.ious.cuda(), scores.cuda(), 0.3)
    b = non_max_suppression_gpu(c.ious.cuda(), scores.cuda(), 0.3)
    (d,) = greedy_nms_batched([scene_tensors["r200"][0]], [scores.cuda()], 0.3)
    assert a.cpu().tolist() == want and torch.equal(a, b) and torch.equal(a, d)
    m = torch.zeros((4, 256), dtype=torch.int32, device="cuda")
    for i in range(4):
        m[i, i * 64:(i + 1) * 64] = 1  # disjoint: nothing is suppressed
    (p,) = greedy_nms_batched([m], [torch.tensor([0.7, 0.9, 0.7, 0.7], device="cuda")], 0.3)
    assert p.cpu().tolist() == [1, 0, 2, 3]


def test_non_symmetric_matrix_reads_the_picks_row(hip):
    from geoformer_amd.postprocess import non_max_suppression_gpu

    c = cases()["nonsym"]
    assert c.picks[0] == [2, 1]
    assert non_max_suppression_gpu(c.ious.t().contiguous().cuda(), c.scores.cuda(), 0.5).cpu().tolist() == [2, 0]
    nan = torch.tensor([[1.0, float("nan"), 0.5], [float("nan"), 1.0, 0.0], [0.5, 0.0, 1.0]], device="cuda")
    assert non_max_suppression_gpu(nan, torch.tensor([0.9, 0.8, 0.7], device="cuda"), 0.5).cpu().tolist() == [0, 1, 2]


def test_more_than_the_capacity_raises_before_a_launch(hip):
    from geoformer_amd import pointops, postprocess

    n = postprocess.NMS_MAX_N + 1
    before = hip.gf_last_error()
    with pytest.raises(ValueError, match="at most 1024"):
        postprocess.non_max_suppression_gpu(torch.zeros((n, n), device="cuda"), torch.zeros(n, device="cuda"), 0.3)
    with pytest.raises(ValueError, match="at most 1024"):
        postprocess.greedy_nms_batched([torch.zeros((n, 64), dtype=torch.int32, device="cuda")],
                                       [torch.zeros(n, device="cuda")], 0.3)
    assert hip.gf_last_error() == before  # nothing reached the library
    # the library refuses the size as well, and leaves the buffers alone
    picks = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    count = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    st = hip.gf_greedy_nms_ious(pointops.ptr(torch.zeros((n, n), device="cuda")),
                                pointops.ptr(torch.zeros(n, device="cuda")), n, 0.3, pointops.ptr(picks),
                                pointops.ptr(count), pointops.stream_ptr())
    torch.cuda.synchronize()
    assert st < 0 and count.item() == -7 and (picks == -7).all()


@pytest.fixture(scope="module")
def model(hip):
    from geoformer_amd.model import GeoFormer, load_config
    from tests.util import synthetic_state_dict

    m = GeoFormer(load_config("test_geoformer_scannet.yaml"))
    m.load_state_dict(synthetic_state_dict(m.state_dict(), 0))
    m.cuda()
    m.eval()
    return m


def _raw(sc):
    return np.concatenate([sc["xyz"], sc["rgb"], sc["label"][:, None], sc["instance"][:, None]], 1).astype(np.float64)


def test_predict_batches_greedy(model):
    from geoformer_amd import batch_eval, scene
    from geoformer_amd.postprocess import non_max_suppression_gpu

    items = [(f"s{i}", _raw(scene.make_small_scene(8192, 7 + i))) for i in range(2)]
    runs = {}
    for key, kw in (("plain", {}), ("matrix", {"nms": "matrix"}), ("greedy", {"nms": "greedy"}),
                    ("greedy.5", {"nms": "greedy", "nms_thresh": 0.5})):
        np.random.seed(21)
        runs[key] = list(batch_eval.predict_batches(model, items, 2, final_score_thresh=0.0, **kw))
    n_props = 0
    for plain, matrix, greedy, g5 in zip(*[runs[k] for k in ("plain", "matrix", "greedy", "greedy.5")]):
        assert plain[0] == matrix[0] == greedy[0]
        assert torch.is_tensor(plain[3]), "the synthetic scenes give proposals"
        assert torch.equal(plain[4], matrix[4]) and torch.equal(plain[3], matrix[3]) and torch.equal(plain[2], matrix[2])
        assert torch.equal(plain[3], greedy[3]) and torch.equal(plain[2], greedy[2])  # the same forward
        _, _, sc, masks, pick = greedy
        f = masks.float()
        inter = torch.mm(f, f.t())
        pn = f.sum(1)
        cross_ious = inter / (pn[:, None] + pn[None, :] - inter)
        assert torch.equal(pick, non_max_suppression_gpu(cross_ious, sc, model.cfg.TEST_NMS_THRESH))
        assert torch.equal(g5[4], non_max_suppression_gpu(cross_ious, sc, 0.5))
        assert pick.dtype == torch.int64 and 0 < pick.numel() <= sc.numel()
        n_props += sc.numel()
    assert n_props > 2
