"""GPU: the model a test.py-shaped driver gets after dropin.install(model=True) (geoformer_amd.reference_names.GeoFormer
built from util.config.cfg) against the reference-generated golden of tests/test_gpu_model.py, bit for bit against
geoformer_amd.model.GeoFormer, and through test.py's own post-process (lines 61-97) with both NMS functions of the
mirrored util.utils_3d."""
import os
import sys

import numpy as np
import pytest
import torch

from tests.dropin_model_tree import driver_tree  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _to_dev(batch):
    return {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in batch.items()}


def _forward(m, z):
    from geoformer_amd import scene

    batch = _to_dev(scene.make_batch([scene.make_small_scene(int(z["scene_points"]), int(z["scene_seed"]))]))
    np.random.seed(int(z["numpy_seed"]))
    with torch.no_grad():
        out = m(batch, 300, training=False)
    torch.cuda.synchronize()
    return out


def test_driver_shaped_eval_and_post_process(hip, driver_tree):
    import geoformer_amd.model as gm
    from geoformer_amd import dropin, evaluation
    from tests.util import synthetic_state_dict

    driver_tree("test_geoformer_scannet.yaml")
    dropin.install(model=True)
    # test.py:7-15
    from util.config import cfg
    from model.geoformer.geoformer import GeoFormer
    from util.utils_3d import load_ids, non_max_suppression_gpu, matrix_non_max_suppression  # noqa: F401

    z = np.load(os.path.join(G, "geoformer_s8k_eval.npz"))
    model = GeoFormer()
    model = model.cuda(0)
    assert isinstance(model, gm.GeoFormer) and model.cfg is cfg and cfg is sys.modules["util.config"].cfg
    direct = gm.GeoFormer(gm.load_config("test_geoformer_scannet.yaml"))
    assert {k: v.shape for k, v in model.state_dict().items()} == {k: v.shape for k, v in direct.state_dict().items()}
    sd = synthetic_state_dict(model.state_dict(), int(z["weight_seed"]))
    model.load_state_dict(sd)
    direct.load_state_dict(sd)
    direct.cuda(0)
    model.eval(), direct.eval()
    out = _forward(model, z)
    # the golden, with the tolerances of tests/test_gpu_model.py
    assert np.abs(out["semantic_scores"].cpu().numpy() - z["semantic_scores"]).max() < 1e-4
    assert (out["fg_idxs"].cpu().numpy() == z["fg_idxs"]).all()
    assert (model.last_sampling_indices.cpu().numpy() == z["sampling_indices"]).all()
    mp = out["mask_predictions"][-1]
    assert np.abs(mp["cls_logits"].cpu().numpy() - z["cls_logits"]).max() < 1e-4
    ml = mp["mask_logits"][0].cpu().numpy()
    assert np.abs(ml[::8, ::4] - z["mask_logits_sub"]).max() < 1e-4
    assert np.abs(ml.astype(np.float64).sum(1) - z["mask_logits_rowsum"]).max() < 1e-4 * ml.shape[1]
    cls_final, scores_final, masks_final = out["proposal_scores"]
    assert (cls_final.cpu().numpy() == z["proposal_cls"]).all()
    assert np.abs(scores_final.cpu().numpy() - z["proposal_scores"]).max() < 1e-4
    d = np.abs(masks_final.sum(1).cpu().numpy() - z["proposal_npoints"])
    assert d.max() <= 3 and (d > 0).mean() < 0.1
    # the same class underneath: identical bits
    ref = _forward(direct, z)
    assert torch.equal(out["semantic_scores"], ref["semantic_scores"]) and torch.equal(out["fg_idxs"], ref["fg_idxs"])
    rp = ref["mask_predictions"][-1]
    assert torch.equal(mp["cls_logits"], rp["cls_logits"]) and torch.equal(mp["mask_logits"][0], rp["mask_logits"][0])
    assert all(torch.equal(a, b) for a, b in zip(out["proposal_scores"], ref["proposal_scores"]))
    # test.py:61-97
    assert not isinstance(cls_final, list)
    temp = torch.tensor(evaluation.FOLD_SEMANTIC_LABELS[cfg.cvfold], device=scores_final.device)[cls_final - 4]
    semantic_id = torch.tensor(evaluation.BENCHMARK_SEMANTIC_LABELS, device=scores_final.device)[temp]
    assert torch.equal(semantic_id, evaluation.benchmark_label_ids(cls_final, cfg.cvfold))
    assert semantic_id.shape[0] > 1
    proposals_pred_f = masks_final.float()
    intersection = torch.mm(proposals_pred_f, proposals_pred_f.t())
    proposals_pointnum = proposals_pred_f.sum(1)
    proposals_pn_h = proposals_pointnum.unsqueeze(-1).repeat(1, proposals_pointnum.shape[0])
    proposals_pn_v = proposals_pointnum.unsqueeze(0).repeat(proposals_pointnum.shape[0], 1)
    cross_ious = intersection / (proposals_pn_h + proposals_pn_v - intersection)
    greedy = non_max_suppression_gpu(cross_ious, scores_final, cfg.TEST_NMS_THRESH)
    matrix = matrix_non_max_suppression(masks_final.float(), scores_final, semantic_id, final_score_thresh=0.5)
    for pick_idxs in (greedy, matrix):
        assert pick_idxs.dtype == torch.int64 and pick_idxs.device == scores_final.device
        clusters = masks_final[pick_idxs].cpu().numpy()
        assert clusters.shape == (pick_idxs.numel(), masks_final.shape[1])
        assert scores_final[pick_idxs].shape == semantic_id[pick_idxs].shape == (pick_idxs.numel(),)
    assert 0 < greedy.numel() <= scores_final.numel()
    want = non_max_suppression_gpu(cross_ious.cpu(), scores_final.cpu(), cfg.TEST_NMS_THRESH)
    assert greedy.cpu().tolist() == want.tolist()
