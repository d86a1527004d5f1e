"""Post-processing of the eval forward: matrix NMS over the proposals (util/utils_3d.py:95-141, called by
test.py:88-93 right after the forward)."""
from __future__ import annotations

import numpy as np
import torch

PROP_SCENE_FIELDS = 6  # GF_PROP_SCENE_FIELDS, include/geoformer_hip.h
NMS_SCENE_FIELDS = 8  # GF_NMS_SCENE_FIELDS
NMS_MAX_N = 1024  # GF_NMS_MAX_N


def matrix_non_max_suppression(proposals_pred, scores, categories, kernel="gaussian", sigma=2.0,
                               final_score_thresh=0.05):
    """Same signature and result as the reference: indices (into the inputs) of the proposals whose decayed score
    stays >= final_score_thresh, in descending score order.  proposals_pred [n,N] 0/1 (int or float), scores [n],
    categories [n].  On the GPU the [n,n] intersection matrix comes from the bit-packed popcount kernel
    (csrc/proposal.hip) instead of a dense float einsum over N points; the rest is the reference's [n,n] algebra."""
    ixs = torch.argsort(scores, descending=True)
    n = len(ixs)
    categories_sorted = categories[ixs]
    scores_sorted = scores[ixs]
    if proposals_pred.is_cuda:
        from . import pointops

        masks = proposals_pred if proposals_pred.dtype == torch.int32 else (proposals_pred != 0).int()
        inter = pointops.mask_intersections(masks.contiguous())
        intersection = inter[ixs][:, ixs].to(scores.dtype)
    else:
        p = proposals_pred[ixs].type(scores.dtype)
        intersection = torch.einsum("nc,mc->nm", p, p)
    pointnum = torch.diagonal(intersection)
    ious = intersection / (pointnum[:, None] + pointnum[None, :] - intersection)
    cat_x = categories_sorted[None, :].expand(n, n)
    label_matrix = (cat_x == cat_x.transpose(1, 0)).float().triu(diagonal=1)
    compensate_iou, _ = (ious * label_matrix).max(0)
    compensate_iou = compensate_iou.expand(n, n).transpose(1, 0)
    decay_iou = ious * label_matrix
    if kernel == "gaussian":
        decay_matrix = torch.exp(-1 * sigma * (decay_iou ** 2))
        compensate_matrix = torch.exp(-1 * sigma * (compensate_iou ** 2))
        decay_coefficient, _ = (decay_matrix / compensate_matrix).min(0)
    elif kernel == "linear":
        decay_coefficient, _ = ((1 - decay_iou) / (1 - compensate_iou)).min(0)
    else:
        raise NotImplementedError
    return ixs[(scores_sorted * decay_coefficient) >= final_score_thresh]


# ---- batched post-processing (csrc/batch_post.hip): host side ---------------------------------------------------------
def packed_layout(counts, widths):
    """(row offsets [S+1], element offsets [S+1]) of per-scene blocks [counts[b], widths[b]] stored one after the
    other in one flat buffer -- the layout gf_proposal_scatter_batched writes."""
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    widths = np.asarray(widths, dtype=np.int64).reshape(-1)
    rows = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    elems = np.concatenate([[0], np.cumsum(counts * widths)]).astype(np.int64)
    return rows, elems


def split_packed(packed, counts, widths):
    """Per-scene [counts[b], widths[b]] views of a packed buffer (packed_layout)."""
    _, elems = packed_layout(counts, widths)
    return [packed[int(elems[b]):int(elems[b + 1])].view(int(c), int(w)) if torch.is_tensor(packed)
            else packed[int(elems[b]):int(elems[b + 1])].reshape(int(c), int(w))
            for b, (c, w) in enumerate(zip(counts, widths))]


def proposal_scene_table(logit_ptrs, fg_offsets, point_starts, point_counts):
    """int64 [S, PROP_SCENE_FIELDS] proposal scene table: scene b's mask logits at logit_ptrs[b] ([nq, N_b]), its
    foreground rows fg_offsets[b]:fg_offsets[b+1] of the batch's foreground arrays (sem_t columns, fg_idxs), its
    point_counts[b] points from point_starts[b] on in the batch."""
    fo = np.asarray(fg_offsets, dtype=np.int64).reshape(-1)
    S = len(logit_ptrs)
    ps = np.asarray(point_starts, dtype=np.int64).reshape(-1)
    pc = np.asarray(point_counts, dtype=np.int64).reshape(-1)
    if fo.shape != (S + 1,) or ps.shape != (S,) or pc.shape != (S,):
        raise ValueError(f"proposal_scene_table: {S} scenes need S+1 foreground offsets and S point starts / counts")
    t = np.zeros((S, PROP_SCENE_FIELDS), dtype=np.int64)
    t[:, 0] = np.asarray(logit_ptrs, dtype=np.int64)
    t[:, 1] = np.diff(fo)
    t[:, 2] = fo[:-1]
    t[:, 3] = ps
    t[:, 4] = pc
    return t


def nms_scene_table(mask_ptrs, widths, ns, score_ptrs, cat_ptrs):
    """(int64 [S, NMS_SCENE_FIELDS] NMS scene table, sizes) for scenes of ns[b] proposals over widths[b] points each.
    sizes: total uint64 words of the bit-packed masks ("bits"), int32 elements of the intersection blocks ("inter"), of
    the picks ("picks"), and the largest per-scene wave / pair counts of the two intersection launches."""
    n = np.asarray(ns, dtype=np.int64).reshape(-1)
    N = np.asarray(widths, dtype=np.int64).reshape(-1)
    if (n < 0).any() or (N < 0).any():
        raise ValueError("nms_scene_table: negative size")
    if (n > NMS_MAX_N).any():
        raise ValueError(f"matrix NMS: at most {NMS_MAX_N} proposals per scene, got {int(n.max())}")
    words = n * ((N + 63) // 64)
    S = n.shape[0]
    t = np.zeros((S, NMS_SCENE_FIELDS), dtype=np.int64)
    t[:, 0] = np.asarray(mask_ptrs, dtype=np.int64)
    t[:, 1] = np.where(n > 0, N, 0)
    t[:, 2] = n
    t[:, 3] = np.concatenate([[0], np.cumsum(words)[:-1]]) if S else []
    t[:, 4] = np.concatenate([[0], np.cumsum(n * n)[:-1]]) if S else []
    t[:, 5] = np.asarray(score_ptrs, dtype=np.int64)
    t[:, 6] = np.asarray(cat_ptrs, dtype=np.int64)
    t[:, 7] = np.concatenate([[0], np.cumsum(n)[:-1]]) if S else []
    sizes = {"bits": int(words.sum()), "inter": int((n * n).sum()), "picks": int(n.sum()),
             "max_waves": int(words.max()) if S else 0, "max_pairs": int((n * n).max()) if S else 0}
    return t, sizes


def matrix_nms_batched(masks, scores, categories, kernel="gaussian", sigma=2.0, final_score_thresh=0.05):
    """matrix_non_max_suppression of several scenes at once on the GPU: lists of per-scene masks [n_b, N_b] (int32 0/1;
    other dtypes are converted), scores fp32 [n_b] and categories [n_b]; a scene without proposals may be given as
    empty lists.  Returns one int64 tensor of picks per scene: indices into the scene's proposals, in descending-score
    order.  Fixed launches per batch (table upload, bit packing, intersections, fused NMS, one read-back of the counts);
    equal scores are ordered by ascending index (torch.argsort gives no guarantee)."""
    from . import pointops

    if kernel not in ("gaussian", "linear"):
        raise NotImplementedError(kernel)
    if not (len(masks) == len(scores) == len(categories)):
        raise ValueError("matrix_nms_batched: masks, scores and categories need one entry per scene")
    dev = next((m.device for m in masks if torch.is_tensor(m)), None)
    if dev is None:  # no scene has proposals
        return [torch.zeros(0, dtype=torch.int64) for _ in masks]
    if dev.type != "cuda":
        raise RuntimeError("matrix_nms_batched: the batched kernels run on the GPU; matrix_non_max_suppression is the "
                           "CPU path")
    keep, ms, ss, cs, ns, ws = [], [], [], [], [], []
    for m, s, c in zip(masks, scores, categories):
        if not torch.is_tensor(m) or m.shape[0] == 0:
            ns.append(0), ws.append(0), ms.append(0), ss.append(0), cs.append(0)
            continue
        m = (m if m.dtype == torch.int32 else (m != 0).int()).contiguous()
        s = s.to(torch.float32).contiguous()
        c = c.to(torch.int64).contiguous()
        if s.shape != (m.shape[0],) or c.shape != (m.shape[0],):
            raise ValueError("matrix_nms_batched: scores / categories must be [n] for masks [n, N]")
        keep += [m, s, c]
        ns.append(m.shape[0]), ws.append(m.shape[1])
        ms.append(m.data_ptr()), ss.append(s.data_ptr()), cs.append(c.data_ptr())
    table, sizes = nms_scene_table(ms, ws, ns, ss, cs)
    table_d = pointops._table_dev(table, dev)
    inter = pointops.mask_intersections_batched(table_d, sizes)
    picks, counts = pointops.matrix_nms_batched(table_d, inter, sizes, 1 if kernel == "linear" else 0, sigma,
                                                final_score_thresh)
    counts_h = counts.cpu().tolist()
    picks = picks.long()
    return [picks[int(table[b, 7]):int(table[b, 7]) + counts_h[b]] for b in range(len(ns))]
