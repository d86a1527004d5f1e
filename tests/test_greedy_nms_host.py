"""CPU: greedy NMS (postprocess.non_max_suppression_gpu, the reference's util/utils_3d.py:76-93) against the picks the
reference's function gave on the same inputs (tests/golden/greedy_nms.npz), and the host side of the batched path."""
import numpy as np
import pytest
import torch

from tests.greedy_nms_cases import case_ids, cases


def test_fixture_lists_the_cases():
    assert sorted(cases()) == sorted(case_ids())
    c = cases()
    assert [c[k].scores.shape[0] for k in ("one", "half", "chain3", "r65", "r200", "r1024")] == [1, 2, 3, 65, 200, 1024]
    assert c["half"].ious[0, 1].item() == 0.5 and c["half"].picks[2] == [0, 1]  # exactly at the threshold: kept
    assert c["chain"].picks[0] == [0, 2]  # the dead middle suppresses nothing


@pytest.mark.parametrize("name", case_ids())
def test_cpu_path_equals_reference(name):
    from geoformer_amd.postprocess import non_max_suppression_gpu

    c = cases()[name]
    for thr, want in zip(c.thresholds, c.picks):
        got = non_max_suppression_gpu(c.ious, c.scores, thr)
        assert got.dtype == torch.int64 and got.device == c.scores.device
        assert got.tolist() == want, (name, thr)


def test_equal_scores_pick_the_lower_index_first():
    from geoformer_amd.postprocess import non_max_suppression_gpu

    ious = torch.eye(4)
    ious[1, 3] = ious[3, 1] = 0.8
    s = torch.tensor([0.7, 0.9, 0.7, 0.7])
    assert non_max_suppression_gpu(ious, s, 0.5).tolist() == [1, 0, 2]
    ious = torch.eye(2)
    ious[0, 1] = ious[1, 0] = 0.9
    assert non_max_suppression_gpu(ious, torch.tensor([0.5, 0.5]), 0.5).tolist() == [0]


def test_nan_never_suppresses_and_comparison_is_strict():
    from geoformer_amd.postprocess import non_max_suppression_gpu

    ious = torch.tensor([[1.0, float("nan"), 0.5], [float("nan"), 1.0, 0.0], [0.5, 0.0, 1.0]])
    assert non_max_suppression_gpu(ious, torch.tensor([0.9, 0.8, 0.7]), 0.5).tolist() == [0, 1, 2]


def test_greedy_nms_batched_refuses_cpu_tensors():
    from geoformer_amd import postprocess as pp

    m = torch.zeros((2, 8), dtype=torch.int32)
    s = torch.tensor([0.5, 0.4])
    with pytest.raises(RuntimeError, match="run on the GPU"):
        pp.greedy_nms_batched([m], [s], 0.3)
    with pytest.raises(RuntimeError, match="run on the GPU"):
        pp.matrix_nms_batched([m], [s], [torch.zeros(2, dtype=torch.int64)])
    assert [p.numel() for p in pp.greedy_nms_batched([[], []], [[], []], 0.3)] == [0, 0]
    with pytest.raises(ValueError):
        pp.greedy_nms_batched([m], [s, s], 0.3)


def test_scene_table_refuses_more_than_the_capacity():
    from geoformer_amd import postprocess as pp

    assert pp.NMS_MAX_N == 1024
    pp.nms_scene_table([0], [64], [1024], [0], [0])
    with pytest.raises(ValueError):
        pp.nms_scene_table([0], [64], [1025], [0], [0])


def test_bad_shapes_and_keywords():
    from geoformer_amd import batch_eval
    from geoformer_amd.postprocess import non_max_suppression_gpu

    with pytest.raises(ValueError):
        non_max_suppression_gpu(torch.zeros(3, 2), torch.zeros(3), 0.3)
    with pytest.raises(ValueError, match="nms"):
        next(batch_eval.predict_batches(None, [], 1, nms="soft"))
    assert np.array_equal(non_max_suppression_gpu(torch.zeros(0, 0), torch.zeros(0), 0.3).numpy(), np.zeros(0, np.int64))
