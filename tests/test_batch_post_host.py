"""Host side of the batched post-processing (geoformer_amd/postprocess.py, no GPU): scene tables, the packed layout of
the per-scene outputs, and a numpy restatement of the fused matrix NMS (csrc/batch_post.hip) against the CPU path of
matrix_non_max_suppression."""
import numpy as np
import pytest
import torch

from geoformer_amd import postprocess as pp


def test_packed_layout_and_split():
    counts, widths = [2, 0, 3], [5, 7, 4]
    rows, elems = pp.packed_layout(counts, widths)
    assert rows.tolist() == [0, 2, 2, 5] and elems.tolist() == [0, 10, 10, 22]
    buf = torch.arange(22, dtype=torch.int32)
    parts = pp.split_packed(buf, counts, widths)
    assert [tuple(p.shape) for p in parts] == [(2, 5), (0, 7), (3, 4)]
    assert parts[0][1, 0].item() == 5 and parts[2][0, 0].item() == 10 and parts[2][2, 3].item() == 21
    assert [p.shape for p in pp.split_packed(np.arange(22), counts, widths)] == [(2, 5), (0, 7), (3, 4)]
    assert pp.packed_layout([], [])[1].tolist() == [0]


def test_proposal_scene_table():
    t = pp.proposal_scene_table([1000, 2000], [0, 30, 75], [0, 900], [900, 400])
    assert t.shape == (2, pp.PROP_SCENE_FIELDS) and t.dtype == np.int64
    assert t[0].tolist() == [1000, 30, 0, 0, 900, 0]
    assert t[1].tolist() == [2000, 45, 30, 900, 400, 0]
    with pytest.raises(ValueError):
        pp.proposal_scene_table([1], [0], [0], [1])


def test_nms_scene_table_offsets_and_empty_scenes():
    t, sz = pp.nms_scene_table([11, 0, 33, 44], [100, 50, 64, 65], [3, 0, 1, 2], [5, 0, 6, 7], [8, 0, 9, 10])
    assert t.shape == (4, pp.NMS_SCENE_FIELDS)
    words = [3 * 2, 0, 1, 2 * 2]
    assert t[:, 3].tolist() == [0, 6, 6, 7] and sz["bits"] == sum(words) and sz["max_waves"] == 6
    assert t[:, 4].tolist() == [0, 9, 9, 10] and sz["inter"] == 14 and sz["max_pairs"] == 9
    assert t[:, 7].tolist() == [0, 3, 3, 4] and sz["picks"] == 6
    assert t[1].tolist()[:3] == [0, 0, 0]  # a scene with n = 0 proposals reads nothing
    assert t[:, 0].tolist() == [11, 0, 33, 44] and t[:, 5].tolist() == [5, 0, 6, 7] and t[:, 6].tolist() == [8, 0, 9, 10]
    t0, sz0 = pp.nms_scene_table([], [], [], [], [])
    assert t0.shape == (0, pp.NMS_SCENE_FIELDS) and sz0["picks"] == 0
    with pytest.raises(ValueError):
        pp.nms_scene_table([1], [10], [pp.NMS_MAX_N + 1], [1], [1])


def _nms_kernel_numpy(inter, scores, cats, kernel="gaussian", sigma=2.0, thresh=0.05):
    """The per-scene algebra of k_bp_matrix_nms as written there (fp32): rank by score, descending, equal scores by
    ascending index; compensation = max same-class IoU with a higher-ranked proposal; decay = min over all rows."""
    n = len(scores)
    if n == 0:
        return []
    f = np.float32
    order = sorted(range(n), key=lambda i: (-scores[i], i))
    d = np.array([inter[o, o] for o in order], f)
    I = inter[np.ix_(order, order)].astype(f)
    iou = I / ((d[:, None] + d[None, :]) - I)
    c = cats[order]
    lab = (c[:, None] == c[None, :]) & (np.arange(n)[:, None] < np.arange(n)[None, :])
    x = np.where(lab, iou, f(0))
    comp = x.max(0)
    neg = f(-sigma)
    if kernel == "gaussian":
        ratio = np.exp(neg * (x * x)) / np.exp(neg * (comp * comp))[:, None]
    else:
        ratio = (f(1) - x) / (f(1) - comp)[:, None]
    coef = ratio.min(0)
    keep = scores[order] * coef >= f(thresh)
    return [order[a] for a in range(n) if keep[a]]


@pytest.mark.parametrize("kernel", ["gaussian", "linear"])
@pytest.mark.parametrize("seed", range(6))
def test_numpy_restatement_matches_matrix_nms_cpu(kernel, seed):
    rng = np.random.default_rng(seed)
    n, N = int(rng.integers(1, 60)), int(rng.integers(50, 400))
    masks = np.zeros((n, N), np.float32)
    for i in range(n):
        ln = int(rng.integers(5, N // 2))
        s = int(rng.integers(0, N - ln))
        masks[i, s:s + ln] = 1
    scores = rng.permutation(n).astype(np.float32) / n + np.float32(0.01)  # distinct
    cats = rng.integers(0, 3, n).astype(np.int64)
    for thresh in (0.05, 0.3):
        want = pp.matrix_non_max_suppression(torch.from_numpy(masks), torch.from_numpy(scores), torch.from_numpy(cats),
                                             kernel=kernel, final_score_thresh=thresh).tolist()
        inter = (masks.astype(np.int64) @ masks.T.astype(np.int64))
        assert _nms_kernel_numpy(inter, scores, cats, kernel, thresh=thresh) == want


def test_numpy_restatement_tie_rule_and_empty():
    inter = np.diag([10, 10, 10]).astype(np.int64)
    assert _nms_kernel_numpy(inter, np.array([0.5, 0.9, 0.5], np.float32), np.zeros(3, np.int64)) == [1, 0, 2]
    assert _nms_kernel_numpy(np.zeros((0, 0)), np.zeros(0, np.float32), np.zeros(0, np.int64)) == []


def test_matrix_nms_batched_without_proposals_needs_no_gpu():
    assert [p.numel() for p in pp.matrix_nms_batched([[], []], [[], []], [[], []])] == [0, 0]
