"""Post-processing of the eval forward: matrix NMS over the proposals (util/utils_3d.py:95-141, called by
test.py:88-93 right after the forward) and the reference's other post-process, class-agnostic greedy
NMS (util/utils_3d.py:76-93, test.py:78-86 with cfg.TEST_NMS_THRESH)."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from . import _abi

PROP_SCENE_FIELDS = _abi.const("GF_PROP_SCENE_FIELDS")
NMS_SCENE_FIELDS = _abi.const("GF_NMS_SCENE_FIELDS")
NMS_MAX_N = _abi.const("GF_NMS_MAX_N")


# ---- a scene table's layout is its row struct in include/geoformer_hip.h: here a numpy record dtype, read by member name --
PROP_ROW, NMS_ROW, LBL_ROW, SEG_ROW, TILE_ROW, TILE_SCORE_ROW, BOX_SCENE_ROW, BOX_IOU_ROW = (
    np.dtype(_abi.struct("Gf" + name)) for name in ("PropScene", "NmsScene", "LblScene", "SegScene", "TileScene",
                                                    "TileScore", "BoxScene", "BoxIouScene"))


def scene_table(S, row):
    """(table, rows): a zeroed int64 [S, F] scene table and its [S] record view (the same memory) for the row struct."""
    rows = np.zeros(S, dtype=row)
    return rows.view(np.int64).reshape(S, row.itemsize // 8), rows


def scene_rows(table, row):
    """The [S] record view of a host scene table int64 [S, F] (the same memory when the table is contiguous)."""
    return np.ascontiguousarray(table, dtype=np.int64).view(row).reshape(-1)


def _columns(name):
    """The columns of an output row struct whose members share one scalar type, by member name: an index, or a slice
    for an array member -- for numpy arrays and tensors [rows, columns] alike."""
    cols = {}
    for m, (dt, off, *_) in np.dtype(_abi.struct(name)).fields.items():
        at, n = off // dt.base.itemsize, dt.itemsize // dt.base.itemsize
        cols[m] = slice(at, at + n) if dt.shape else at
    return type(name, (), cols)


def _excl(a):
    """Exclusive cumulative sum of a [S] array ([] when S == 0)."""
    return np.concatenate([[0], np.cumsum(a)[:-1]]) if len(a) else []


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
    t, r = scene_table(S, PROP_ROW)
    r["logits"] = np.asarray(logit_ptrs, dtype=np.int64)
    r["N"] = np.diff(fo)
    r["fg_off"] = fo[:-1]
    r["pt_off"] = ps
    r["num_points"] = pc
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
    t, r = scene_table(S, NMS_ROW)
    r["masks"] = np.asarray(mask_ptrs, dtype=np.int64)
    r["N"] = np.where(n > 0, N, 0)
    r["n"] = n
    r["bits_off"], r["inter_off"], r["pick_off"] = _excl(words), _excl(n * n), _excl(n)
    r["scores"] = np.asarray(score_ptrs, dtype=np.int64)
    r["cats"] = np.asarray(cat_ptrs, dtype=np.int64)
    sizes = {"bits": int(words.sum()), "inter": int((n * n).sum()), "picks": int(n.sum()),
             "max_waves": int(words.max()) if S else 0, "max_pairs": int((n * n).max()) if S else 0}
    return t, sizes


def _nms_batch_table(who, masks, scores, categories=None):
    """(device, host scene table, device scene table, sizes, tensors to keep alive) of per-scene lists, for the batched
    NMS kernels; device None: no scene has proposals.  categories None: the table's category pointers are 0."""
    from . import pointops

    categories = [None] * len(masks) if categories is None else categories
    if not (len(masks) == len(scores) == len(categories)):
        raise ValueError(f"{who}: masks, scores and categories need one entry per scene")
    dev = next((m.device for m in masks if torch.is_tensor(m)), None)
    if dev is None:
        return None, None, None, None, []
    if dev.type != "cuda":
        raise RuntimeError(f"{who}: the batched kernels run on the GPU; "
                           f"{'matrix_non_max_suppression' if who == 'matrix_nms_batched' else 'non_max_suppression_gpu'}"
                           " is the CPU path")
    keep, ms, ss, cs, ns, ws = [], [], [], [], [], []
    for m, s, c in zip(masks, scores, categories):
        if not torch.is_tensor(m) or m.shape[0] == 0:
            ns.append(0), ws.append(0), ms.append(0), ss.append(0), cs.append(0)
            continue
        m = (m if m.dtype == torch.int32 else (m != 0).int()).contiguous()
        s = s.to(torch.float32).contiguous()
        c = c.to(torch.int64).contiguous() if c is not None else None
        if s.shape != (m.shape[0],) or (c is not None and c.shape != (m.shape[0],)):
            raise ValueError(f"{who}: scores / categories must be [n] for masks [n, N]")
        keep += [m, s, c]
        ns.append(m.shape[0]), ws.append(m.shape[1])
        ms.append(m.data_ptr()), ss.append(s.data_ptr()), cs.append(c.data_ptr() if c is not None else 0)
    table, sizes = nms_scene_table(ms, ws, ns, ss, cs)
    return dev, table, pointops._table_dev(table, dev), sizes, keep


def _split_picks(table, picks, counts):
    counts_h = counts.cpu().tolist()  # the one read-back
    picks = picks.long()
    return [picks[int(o):int(o) + counts_h[b]] for b, o in enumerate(scene_rows(table, NMS_ROW)["pick_off"])]


def matrix_nms_batched(masks, scores, categories, kernel="gaussian", sigma=2.0, final_score_thresh=0.05):
    """matrix_non_max_suppression of several scenes at once on the GPU: lists of per-scene masks [n_b, N_b] (int32 0/1;
    other dtypes are converted), scores fp32 [n_b] and categories [n_b]; a scene without proposals may be given as
    empty lists.  Returns one int64 tensor of picks per scene: indices into the scene's proposals, in descending-score
    order.  Fixed launches per batch (table upload, bit packing, intersections, fused NMS, one read-back of the counts);
    equal scores are ordered by ascending index (torch.argsort gives no guarantee)."""
    from . import pointops

    if kernel not in ("gaussian", "linear"):
        raise NotImplementedError(kernel)
    dev, table, table_d, sizes, _keep = _nms_batch_table("matrix_nms_batched", masks, scores, categories)
    if dev is None:  # no scene has proposals
        return [torch.zeros(0, dtype=torch.int64) for _ in masks]
    inter = pointops.mask_intersections_batched(table_d, sizes)
    picks, counts = pointops.matrix_nms_batched(table_d, inter, sizes, 1 if kernel == "linear" else 0, sigma,
                                                final_score_thresh)
    return _split_picks(table, picks, counts)


# ---- greedy NMS (csrc/batch_post.hip: k_bp_greedy_nms / k_bp_greedy_ious) ----------------------------------------------
def greedy_nms_loop(ious, scores, threshold):
    """The walk of non_max_suppression_gpu in framework operations, on the tensors' device: proposals in descending score
    order (equal scores by ascending index); a proposal still alive is picked and suppresses every later proposal j
    with ious[pick, j] > threshold.  One read-back per proposal: the CPU path, and what the kernel is measured against
    on device tensors."""
    n = scores.shape[0]
    if n == 0:
        return torch.zeros(0, dtype=torch.int64, device=scores.device)
    order = torch.argsort(scores, descending=True, stable=True)
    rows = ious[order][:, order]
    alive = torch.ones(n, dtype=torch.bool, device=scores.device)
    pick = []
    for a in range(n):
        if not bool(alive[a]):
            continue
        pick.append(a)
        alive[a + 1:] &= ~(rows[a, a + 1:] > threshold)
    return order[torch.tensor(pick, dtype=torch.int64, device=scores.device)]


def non_max_suppression_gpu(ious, scores, threshold):
    """Same signature and result as the reference (util/utils_3d.py:76-93): class-agnostic greedy NMS over a given
    [n, n] IoU matrix; the picked indices in pick order, int64 on scores.device.  Equal scores are walked by ascending
    index (torch.argsort gives no guarantee); the comparison is strict and the row is the pick, so a non-symmetric
    matrix matters.  CUDA tensors: one launch of the walk kernel and one read-back (the count), n <= GF_NMS_MAX_N;
    CPU tensors: greedy_nms_loop."""
    n = scores.shape[0]
    if ious.dim() != 2 or ious.shape[0] != n or ious.shape[1] != n:
        raise ValueError(f"non_max_suppression_gpu: ious must be [n, n] for scores [n], got {tuple(ious.shape)}")
    if not scores.is_cuda:
        return greedy_nms_loop(ious, scores, threshold)
    if n > NMS_MAX_N:
        raise ValueError(f"greedy NMS: at most {NMS_MAX_N} proposals per scene, got {n}")
    if n == 0:
        return torch.zeros(0, dtype=torch.int64, device=scores.device)
    from . import pointops

    picks, count = pointops.greedy_nms_ious(ious.to(device=scores.device, dtype=torch.float32).contiguous(),
                                            scores.to(torch.float32).contiguous(), threshold)
    return picks[:int(count.item())].long()


def greedy_nms_batched(masks, scores, threshold):
    """Greedy NMS (non_max_suppression_gpu on IoUs of the masks, as test.py:78-86 builds them) of several scenes at once
    on the GPU: lists of per-scene masks [n_b, N_b] (int32 0/1; other dtypes are converted) and scores fp32 [n_b]; a
    scene without proposals may be given as [].  Returns one int64 tensor of picks per scene, in pick order.  Fixed
    launches per batch (table upload, bit packing, intersections, the walk, one read-back of the counts)."""
    from . import pointops

    dev, table, table_d, sizes, _keep = _nms_batch_table("greedy_nms_batched", masks, scores)
    if dev is None:  # no scene has proposals
        return [torch.zeros(0, dtype=torch.int64) for _ in masks]
    inter = pointops.mask_intersections_batched(table_d, sizes)
    picks, counts = pointops.greedy_nms_batched(table_d, inter, sizes, threshold)
    return _split_picks(table, picks, counts)


# ---- scene labelling (csrc/label_map.hip): one label per point, one table row per picked instance ---------------------
LBL_SCENE_FIELDS = _abi.const("GF_LBL_SCENE_FIELDS")
LBL_CHUNK = _abi.const("GF_LBL_CHUNK")
LBL_OWN_SPLIT = _abi.const("GF_LBL_OWN_SPLIT")
LBL_TABLE_INTS = _abi.const("GF_LBL_TABLE_INTS")
LBL_TABLE_FLOATS = _abi.const("GF_LBL_TABLE_FLOATS")
MIN_SCORE = 0.09  # util/visualize.py:221


class InstanceTable(NamedTuple):
    """One row per rank r of pick.  Geometry is over the whole mask (zeros when count == 0)."""
    count: object  # int32 [p]: points of the mask
    owned: object  # int32 [p]: points whose owner is r
    label_id: object  # int32 [p]: label_ids[pick[r]]
    index: object  # int32 [p]: pick[r], the original proposal
    kept: object  # bool [p]: score >= min_score
    score: object  # fp32 [p]
    centroid: object  # fp32 [p, 3]
    box_min: object  # fp32 [p, 3]
    box_max: object  # fp32 [p, 3]


class SceneLabels(NamedTuple):
    owner: object  # int32 [N]: rank into pick of the instance that owns the point, -1 without one
    ids: object  # int32 [N]: label_id * 1000 + owner + 1 (the val_gt encoding), 0 without an owner
    table: InstanceTable
    masks: object = None  # label_batches(keep_masks=True): the picked masks [p, N], rank order

    def to_host(self):
        """The same labels as numpy arrays."""
        h = lambda a: a.detach().cpu().numpy() if torch.is_tensor(a) else (None if a is None else np.asarray(a))  # noqa: E731
        return SceneLabels(h(self.owner), h(self.ids), InstanceTable(*[h(c) for c in self.table]), h(self.masks))


_LBL_I, _LBL_F = _columns("GfLblRowI"), _columns("GfLblRowF")


def _table_from_packed(ti, tf):
    i, f = _LBL_I, _LBL_F
    return InstanceTable(ti[:, i.count], ti[:, i.owned], ti[:, i.label_id], ti[:, i.pick], ti[:, i.kept] != 0,
                         tf[:, f.score], tf[:, f.centroid], tf[:, f.box_min], tf[:, f.box_max])


def _label_points_host(masks, scores, label_ids, pick, xyz, min_score):
    """numpy path of label_points: the same integers as the kernels; centroid accumulated in float64."""
    xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    N = xyz.shape[0]
    pick = np.asarray(pick, dtype=np.int64).reshape(-1)
    p = pick.shape[0]
    masks = np.asarray(masks).reshape(-1, N) if p else np.zeros((0, N), np.int32)
    scores = np.asarray(scores, dtype=np.float32).reshape(-1)
    label_ids = np.asarray(label_ids, dtype=np.int64).reshape(-1)
    if p and (pick.min() < 0 or pick.max() >= masks.shape[0]):
        raise ValueError("label_points: pick outside the masks")
    if p > NMS_MAX_N:
        raise ValueError(f"label_points: at most {NMS_MAX_N} picked instances per scene, got {p}")
    m = masks[pick] != 0
    sc = scores[pick]
    kept = sc >= np.float32(min_score)
    lab = label_ids[pick].astype(np.int32)
    owner = np.full(N, -1, np.int32)
    for r in np.nonzero(kept)[0]:
        sel = m[r] & (owner < 0)
        owner[sel] = r
    own = np.maximum(owner, 0)
    ids = np.where(owner >= 0, lab[own] * 1000 + owner + 1, 0).astype(np.int32) if p else np.zeros(N, np.int32)
    count = m.sum(1).astype(np.int32)
    owned = np.bincount(owner[owner >= 0], minlength=p).astype(np.int32)
    centroid = np.zeros((p, 3), np.float32)
    box_min = np.zeros((p, 3), np.float32)
    box_max = np.zeros((p, 3), np.float32)
    x64 = xyz.astype(np.float64)
    for r in range(p):
        if count[r]:
            q = m[r]
            centroid[r] = (x64[q].sum(0) / count[r]).astype(np.float32)
            box_min[r], box_max[r] = xyz[q].min(0), xyz[q].max(0)
    return SceneLabels(owner, ids, InstanceTable(count, owned, lab, pick.astype(np.int32), kept, sc, centroid, box_min,
                                                 box_max))


def label_scene_table(mask_ptrs, widths, ns, ps, pick_ptrs, score_ptrs, label_ptrs, xyz_ptrs):
    """(int64 [S, LBL_SCENE_FIELDS] label scene table, sizes) for scenes of ps[b] picks out of ns[b] masks over widths[b]
    points.  sizes: uint64 words of the packed bits ("bits"), partial records ("parts"), table rows ("rows"), points
    ("points") in total, and the largest per-scene point / pick counts of the launches."""
    N = np.asarray(widths, dtype=np.int64).reshape(-1)
    n = np.asarray(ns, dtype=np.int64).reshape(-1)
    p = np.asarray(ps, dtype=np.int64).reshape(-1)
    if (n < 0).any() or (N < 0).any() or (p < 0).any():
        raise ValueError("label_scene_table: negative size")
    if (p > NMS_MAX_N).any():
        raise ValueError(f"label_points: at most {NMS_MAX_N} picked instances per scene, got {int(p.max())}")
    S = N.shape[0]
    words = p * ((N + 63) // 64)
    parts = p * ((N + LBL_CHUNK - 1) // LBL_CHUNK)
    t, r = scene_table(S, LBL_ROW)
    r["masks"] = np.asarray(mask_ptrs, dtype=np.int64)
    r["N"], r["n"], r["p"] = N, n, p
    r["pick"] = np.asarray(pick_ptrs, dtype=np.int64)
    r["scores"] = np.asarray(score_ptrs, dtype=np.int64)
    r["label_ids"] = np.asarray(label_ptrs, dtype=np.int64)
    r["xyz"] = np.asarray(xyz_ptrs, dtype=np.int64)
    r["bits_off"], r["part_off"], r["row_off"], r["pt_off"] = _excl(words), _excl(parts), _excl(p), _excl(N)
    sizes = {"bits": int(words.sum()), "parts": int(parts.sum()), "rows": int(p.sum()), "points": int(N.sum()),
             "max_points": int(N.max()) if S else 0, "max_picks": int(p.max()) if S else 0}
    return t, sizes


def _label_batch_packed(masks, scores, label_ids, picks, xyzs, min_score):
    """The batch's launches: (scene table (host), packed device buffers of pointops.label_map_batched)."""
    from . import pointops

    S = len(xyzs)
    if not (len(masks) == len(scores) == len(label_ids) == len(picks) == S):
        raise ValueError("label_points_batched: one entry per scene in every list")
    dev = next((x.device for x in xyzs if torch.is_tensor(x)), None)
    if dev is None or dev.type != "cuda":
        raise RuntimeError("label_points_batched: the kernels run on the GPU; label_points has the numpy path")
    keep, rows, Ns, ns, ps = [], [], [], [], []
    for m, s, l, pk, x in zip(masks, scores, label_ids, picks, xyzs):
        x = torch.as_tensor(x, device=dev).to(torch.float32).reshape(-1, 3).contiguous()
        N = x.shape[0]
        pk = torch.as_tensor(pk, device=dev).to(torch.int64).reshape(-1).contiguous() if len(pk) else None
        if not torch.is_tensor(m) or m.shape[0] == 0 or pk is None:
            keep.append(x)
            rows.append((0, 0, 0, 0, x.data_ptr())), Ns.append(N), ns.append(0), ps.append(0)
            continue
        m = (m if m.dtype == torch.int32 else (m != 0).int()).contiguous()
        s = torch.as_tensor(s, device=dev).to(torch.float32).contiguous()
        l = torch.as_tensor(l, device=dev).to(torch.int64).contiguous()
        if m.dim() != 2 or m.shape[1] != N or s.shape != (m.shape[0],) or l.shape != (m.shape[0],):
            raise ValueError("label_points: masks [n, N], scores [n], label_ids [n], xyz [N, 3]")
        keep += [m, s, l, pk, x]
        rows.append((m.data_ptr(), pk.data_ptr(), s.data_ptr(), l.data_ptr(), x.data_ptr()))
        Ns.append(N), ns.append(m.shape[0]), ps.append(pk.shape[0])
    table, sizes = label_scene_table([r[0] for r in rows], Ns, ns, ps, [r[1] for r in rows], [r[2] for r in rows],
                                     [r[3] for r in rows], [r[4] for r in rows])
    table_d = pointops._table_dev(table, dev)
    return table, pointops.label_map_batched(table_d, sizes, min_score)


def _split_labels(table, pts, ti, tf):
    """One SceneLabels per row of the scene table: views of the packed buffers (device tensors or numpy arrays)."""
    out = []
    for t in scene_rows(table, LBL_ROW):
        N, p, r, o = int(t["N"]), int(t["p"]), int(t["row_off"]), int(t["pt_off"])
        out.append(SceneLabels(pts[0, o:o + N], pts[1, o:o + N], _table_from_packed(ti[r:r + p], tf[r:r + p])))
    return out


def label_points_batched(masks, scores, label_ids, picks, xyzs, min_score=MIN_SCORE):
    """label_points of several scenes at once on the GPU: lists with one entry per scene (a scene without proposals may
    give [] for masks / scores / label_ids, as predict_batches yields it; xyz is always needed).  One table upload and the
    three launches of gf_label_map_batched for the whole batch; returns one SceneLabels per scene, on the device (views of
    the batch's buffers)."""
    table, (pts, ti, tf) = _label_batch_packed(masks, scores, label_ids, picks, xyzs, min_score)
    return _split_labels(table, pts, ti, tf)


def label_points(masks, scores, label_ids, pick, xyz, min_score=MIN_SCORE):
    """Per-point instance labels and the instance table of one scene from its picked masks: masks [n, N] 0/1, scores
    [n], label_ids [n] (benchmark ids, evaluation.benchmark_label_ids), pick [p] rows of masks in descending score order
    (the NMS result), xyz [N, 3].  The owner of a point is the lowest rank r in pick with score >= min_score whose mask
    covers it (util/visualize.py:219-227 paints from the last to the first).  CUDA tensors take the kernels and the
    results stay on the device; numpy arrays / CPU tensors take the numpy path.  A scene without proposals ([] for
    masks) gives an all -1 / all 0 map and an empty table."""
    if torch.is_tensor(xyz) and xyz.is_cuda:
        return label_points_batched([masks], [scores], [label_ids], [pick], [xyz], min_score)[0]
    h = lambda a: a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)  # noqa: E731
    return _label_points_host(h(masks), h(scores), h(label_ids), h(pick), h(xyz), min_score)


# ---- panoptic labels (csrc/panoptic.hip): things from the label map, stuff from the semantic head -------------------
def panoptic_points_batched(labels, sems, stuff=(1, 2), stuff_of_sem=None):
    """Panoptic id of every point of several scenes at once on the GPU: labels: one SceneLabels per scene (device,
    label_points_batched), sems: per scene the semantic head's class of every point (int32 [N_b], device;
    batch_eval.semantic_batches, pointops.semantic_confusion).  pan = ids where the point has an owner, stuff id * 1000
    where the semantic class names a stuff class (stuff: their nyu40 ids; stuff_of_sem: semantic class -> index into
    `stuff` or -1, default class j -> stuff[j]: wall, floor), 0 elsewhere.  One launch (gf_panoptic_overlaps without
    ground truth); returns one int32 tensor per scene, views of the batch's buffer."""
    from . import pointops

    if len(labels) != len(sems):
        raise ValueError("panoptic_points_batched: one entry per scene in both lists")
    if not labels:
        return []
    dev = labels[0].owner.device if torch.is_tensor(labels[0].owner) else None
    if dev is None or dev.type != "cuda":
        raise RuntimeError("panoptic_points_batched: the kernel runs on the GPU; evaluation.panoptic_overlaps_host has "
                           "the numpy path")
    Ns = [int(l.owner.shape[0]) for l in labels]
    if any(int(x.shape[0]) != n for x, n in zip(sems, Ns)):
        raise ValueError("panoptic_points_batched: sems and labels differ in their point counts")
    i32 = lambda ts: torch.cat([torch.as_tensor(t, device=dev).to(torch.int32).reshape(-1) for t in ts]).contiguous()  # noqa: E731
    off = np.concatenate([[0], np.cumsum(Ns)]).astype(np.int32)
    stuff = [int(c) for c in stuff]
    sos = np.arange(len(stuff), dtype=np.int32) if stuff_of_sem is None else np.asarray(stuff_of_sem, dtype=np.int32)
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.int32), device=dev)  # noqa: E731
    P = max(int(l.table.count.shape[0]) for l in labels)
    pan = pointops.panoptic_points(i32([l.owner for l in labels]), i32([l.ids for l in labels]), i32(sems), t(off),
                                   t(stuff), t(np.ones(len(stuff))), t(sos), len(stuff), P)
    return [pan[off[i]:off[i + 1]] for i in range(len(Ns))]


def panoptic_points(labels, sem, stuff=(1, 2), stuff_of_sem=None):
    """panoptic_points_batched of one scene: SceneLabels and the semantic classes in, pan int32 [N] out (device)."""
    return panoptic_points_batched([labels], [sem], stuff, stuff_of_sem)[0]


# ---- mask logits pooled over over-segments (csrc/segment_pool.hip): the host statement ----------------------------------
def segment_pool_host(logits, seg_fg):
    """One scene's mask logits pooled over its over-segments -- the statement gf_segment_pool_batched is tested against,
    and the CPU path of GeoFormer.generate_proposal.  logits fp32 [nq, n] over the scene's foreground points, seg_fg
    int [n]: pooled[q, p] = mean of logits[q, p'] over {p' : seg_fg[p'] == seg_fg[p]} where seg_fg[p] >= 0 (float64
    inside, rounded once to fp32), logits[q, p] where it is negative.  A segment of one point keeps its logit bit for
    bit."""
    x = logits.detach().cpu().numpy() if torch.is_tensor(logits) else np.asarray(logits)
    seg = seg_fg.detach().cpu().numpy() if torch.is_tensor(seg_fg) else np.asarray(seg_fg)
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim != 2 or seg.shape != (x.shape[1],) or not np.issubdtype(seg.dtype, np.integer):
        raise ValueError(f"segment_pool_host: logits [nq, n] and integer seg_fg [n] expected, got {x.shape} / "
                         f"{seg.dtype} {seg.shape}")
    out = x.copy()
    pooled = np.nonzero(seg >= 0)[0]
    if pooled.size:
        _, inv, counts = np.unique(seg[pooled], return_inverse=True, return_counts=True)
        inv = inv.reshape(-1)
        by_seg = pooled[np.argsort(inv, kind="stable")]  # the members of each segment next to each other
        starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
        sums = np.add.reduceat(x[:, by_seg].astype(np.float64), starts, axis=1)
        many = counts[inv] > 1  # (a segment of one point: the copy above, not a round trip through float64)
        mean = (sums / counts[None, :]).astype(np.float32)
        out[:, pooled[many]] = mean[:, inv[many]]
    return out


def segment_scene_table(in_ptrs, out_ptrs, fg_offsets):
    """int64 [S, fields] segment scene table of gf_segment_pool_batched: scene b's logits at in_ptrs[b], the pooled ones
    at out_ptrs[b] (both [nq, N_b]), its foreground rows fg_offsets[b]:fg_offsets[b+1] of the batch."""
    fo =np.asarray(fg_offsets, dtype=np.int64).reshape(-1)
    S = len(in_ptrs)
    if fo.shape != (S + 1,) or len(out_ptrs) != S:
        raise ValueError(f"segment_scene_table: {S} scenes need S output pointers and S+1 foreground offsets")
    t, r = scene_table(S, SEG_ROW)
    r["in"] = np.asarray(in_ptrs, dtype=np.int64)
    r["out"] = np.asarray(out_ptrs, dtype=np.int64)
    r["N"] = np.diff(fo)
    r["off"] = fo[:-1]
    return t


# ---- geometric over-segmentation (csrc/oversegment.hip): the host statement ---------------------------------------------
OVERSEGMENT_DEFAULTS = dict(k=16, radius=0.07, normal_deg=15.0, offset=0.012, flatness=0.01, min_points=8)
_SIGN_EPS = 1e-6  # a normal's first component of magnitude above this is made positive


def _np(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def knn_radius_host(xyz, k, radius):
    """(I int32 [n, k], deg int32 [n]) in the format of gf_knn_radius: per point the k nearest points with
    sqrt(d2) <= radius in fp32, ordered by (d2, index), itself included, -1 where there are fewer; deg = valid entries
    after column 0.  Brute force in blocks of rows (O(n^2)): the CPU path of small scenes and tests."""
    x = np.ascontiguousarray(_np(xyz), dtype=np.float32).reshape(-1, 3)
    n = x.shape[0]
    I = np.full((n, k), -1, np.int32)
    deg = np.zeros(n, np.int32)
    r = np.float32(radius)
    idx = np.arange(n, dtype=np.int64)
    for lo in range(0, n, 512):
        d = x[lo:lo + 512, None, :] - x[None, :, :]
        d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]  # fp32, as the kernel forms it
        inside = np.sqrt(d2) <= r
        key = np.where(inside, d2.view(np.int32).astype(np.int64) << 32 | idx[None, :], np.iinfo(np.int64).max)
        kk = min(k, n)
        part = np.argpartition(key, kk - 1, axis=1)[:, :kk] if kk < n else np.broadcast_to(idx, key.shape)
        pk = np.take_along_axis(key, part, axis=1)
        order = np.argsort(pk, axis=1, kind="stable")
        cols = np.take_along_axis(part, order, axis=1)
        ok = np.take_along_axis(pk, order, axis=1) != np.iinfo(np.int64).max
        I[lo:lo + 512, :kk] = np.where(ok, cols, -1)
        deg[lo:lo + 512] = np.maximum(ok.sum(axis=1) - 1, 0)
    return I, deg


def _valid_entries(I, deg, n):
    """bool [n, k]: the row entries that count -- column c <= deg[i] with an index inside [0, n)."""
    k = I.shape[1]
    return (np.arange(k)[None, :] <= deg[:, None]) & (I >= 0) & (I < n)


def point_normals_host(xyz, I, deg, return_eigenvalues=False):
    """Stage A of oversegment_host in float64: [n, 4] = (nx, ny, nz, sigma) per point from the kNN rows (I, deg).
    The neighbourhood of point i is the valid entries of row i (gf_knn_radius lists i itself).  C is the covariance of
    the differences x_j - x_i about their mean; with fewer than 3 entries, or where C's trace is not positive (all
    entries in one place), the point is invalid: normal 0, sigma -1.  Otherwise the normal is the unit eigenvector of
    the smallest eigenvalue with its first component of magnitude > 1e-6 positive and sigma = max(l0, 0) /
    (l0 + l1 + l2).  return_eigenvalues: also C's eigenvalues [n, 3], ascending (a test's measure of how well the normal
    is determined)."""
    x = np.ascontiguousarray(_np(xyz), dtype=np.float32).reshape(-1, 3).astype(np.float64)
    I, deg = np.asarray(_np(I)), np.asarray(_np(deg))
    n = x.shape[0]
    out = np.zeros((n, 4), np.float64)
    out[:, 3] = -1.0
    if n == 0:
        return (out, np.zeros((0, 3))) if return_eigenvalues else out
    ok = _valid_entries(I, deg, n)
    m = ok.sum(axis=1)
    d = (x[np.where(ok, I, 0)] - x[:, None, :]) * ok[..., None]
    mm = np.maximum(m, 1)[:, None]
    mean = d.sum(axis=1) / mm
    dc = (d - mean[:, None, :]) * ok[..., None]
    C = np.einsum("nka,nkb->nab", dc, dc) / mm[..., None]
    w, v = np.linalg.eigh(C)
    nrm = v[:, :, 0]
    nrm = nrm / np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-300)
    big = np.abs(nrm) > _SIGN_EPS
    first = np.take_along_axis(nrm, np.argmax(big, axis=1)[:, None], axis=1)[:, 0]
    nrm = nrm * np.where(big.any(axis=1) & (first < 0), -1.0, 1.0)[:, None]
    tr = w.sum(axis=1)
    sigma = np.where(tr > 0, np.maximum(w[:, 0], 0.0) / np.where(tr > 0, tr, 1.0), -1.0)
    valid = (m >= 3) & (tr > 0)
    out[valid, :3] = nrm[valid]
    out[valid, 3] = sigma[valid]
    return (out, w) if return_eigenvalues else out


def smooth_components_host(xyz, normals4, I, deg, *, normal_deg=15.0, offset=0.012, flatness=0.01, min_points=8,
                           margins=None):
    """Stages B-D of oversegment_host in float64 from ANY rows and ANY normals4: int32 [n] ids (the smallest point
    index of the component, or -1).  margins = (on the dot product, on the offsets): also returns the number of edge
    and attach decisions whose left side lies within the margin of its threshold."""
    x = np.ascontiguousarray(_np(xyz), dtype=np.float32).reshape(-1, 3).astype(np.float64)
    nrm4 = np.asarray(_np(normals4), dtype=np.float64).reshape(-1, 4)
    I, deg = np.asarray(_np(I)), np.asarray(_np(deg))
    n = x.shape[0]
    if min_points < 1:
        raise ValueError("smooth_components_host: min_points >= 1")
    if n == 0:
        ids = np.zeros(0, np.int32)
        return (ids, 0) if margins is not None else ids
    cos_t = float(np.float32(np.cos(np.radians(normal_deg))))  # the fp32 word the kernel compares with
    off_t = float(np.float32(offset))
    nv, sigma = nrm4[:, :3], nrm4[:, 3]
    flat = (sigma >= 0) & (sigma <= float(np.float32(flatness)))
    ok = _valid_entries(I, deg, n)
    src, col = np.nonzero(ok)
    dst = I[src, col].astype(np.int64)
    ambiguous = 0
    # stage B: the row entries that link two flat points
    e = (dst != src) & flat[src] & flat[dst]
    a, b = src[e], dst[e]
    dot = np.abs(np.einsum("ij,ij->i", nv[a], nv[b]))
    dist = np.abs(np.einsum("ij,ij->i", nv[a], x[b] - x[a]))
    link = (dot >= cos_t) & (dist <= off_t)
    if margins is not None:
        ambiguous += int(((np.abs(dot - cos_t) <= margins[0]) | (np.abs(dist - off_t) <= margins[1])).sum())
    a, b = a[link], b[link]
    # stage C: components by hooking the larger root under the smaller and halving the paths, until nothing moves
    parent = np.arange(n, dtype=np.int64)
    while True:
        ra, rb = parent[a], parent[b]
        hi, lo = np.maximum(ra, rb), np.minimum(ra, rb)
        if not (hi != lo).any():
            break
        np.minimum.at(parent, hi, lo)
        while True:
            nxt = parent[parent]
            if (nxt == parent).all():
                break
            parent = nxt
    ids = np.full(n, -1, np.int64)
    ids[flat] = parent[flat]
    size = np.bincount(ids[flat], minlength=n) if flat.any() else np.zeros(n, np.int64)
    kept = flat & (size[np.maximum(ids, 0)] >= min_points)
    ids[~kept] = -1
    # stage D: a non-flat point takes the id of the first kept flat entry of its row whose plane it lies on
    t = ~flat[src] & kept[dst]
    s, c, j = src[t], col[t], dst[t]
    dist = np.abs(np.einsum("ij,ij->i", nv[j], x[s] - x[j]))
    if margins is not None:
        ambiguous += int((np.abs(dist - off_t) <= margins[1]).sum())
    hit = dist <= off_t
    s, c, j = s[hit], c[hit], j[hit]
    first = np.full(n, I.shape[1], np.int64)
    np.minimum.at(first, s, c)
    take = first[s] == c
    ids[s[take]] = ids[j[take]]
    ids = ids.astype(np.int32)
    return (ids, ambiguous) if margins is not None else ids


def oversegment_host(xyz, I=None, deg=None, *, k=16, radius=0.07, normal_deg=15.0, offset=0.012, flatness=0.01,
                     min_points=8, return_ambiguous=False, margins=None):
    """Geometric over-segmentation of one scene -- the statement gf_point_normals / gf_smooth_components are tested
    against, and the CPU path of pointops.oversegment.  xyz [n, 3]; (I, deg): kNN rows as gf_knn_radius emits them, built
    here (knn_radius_host(k, radius)) when not given.  int32 [n]: ids >= 0 (the smallest point index of the segment) or -1.
      A  per point the normal and the surface variation sigma of its row's points (point_normals_host); a point is
         FLAT when 0 <= sigma <= flatness.
      B  a row entry (i, j), j != i, links i and j when both are flat, |n_i . n_j| >= cos(normal_deg) and
         |n_i . (x_j - x_i)| <= offset; one passing direction suffices.
      C  connected components of the flat points; one with fewer than min_points points is dissolved (-1).
      D  a non-flat point takes the id of the first j of its row, in row order, that is flat and kept and has
         |n_j . (x_i - x_j)| <= offset; -1 without one.
    return_ambiguous: also the number of edge (B) and attach (D) decisions whose left side lies within margins =
    (on the dot product, on the offsets; default (1e-5, 1e-5 * radius)) of its threshold."""
    x = np.ascontiguousarray(_np(xyz), dtype=np.float32).reshape(-1, 3)
    if I is None:
        I, deg = knn_radius_host(x, k, radius)
    if margins is None and return_ambiguous:
        margins = (1e-5, 1e-5 * radius)
    normals4 = point_normals_host(x, I, deg)
    return smooth_components_host(x, normals4, I, deg, normal_deg=normal_deg, offset=offset, flatness=flatness,
                                  min_points=min_points, margins=margins if return_ambiguous else None)


# ---- picked masks split into connected clusters (csrc/mask_split.hip): the host statement -------------------------------
MSP_TABLE_INTS = _abi.const("GF_MSP_TABLE_INTS")
_MSP = _columns("GfMspRow")
SPLIT_DEFAULTS = dict(radius=0.1, k=16, min_samples=1, min_points=50, mode="largest")
SPLIT_MODES = ("largest", "split")


def _min_index_components(n, a, b):
    """int64 [n]: for every vertex the smallest index of its component under the edges (a[e], b[e]) -- the larger root
    hooked under the smaller and the paths halved until nothing moves (stage C of smooth_components_host)."""
    parent = np.arange(n, dtype=np.int64)
    while True:
        ra, rb = parent[a], parent[b]
        hi, lo = np.maximum(ra, rb), np.minimum(ra, rb)
        if not (hi != lo).any():
            return parent
        np.minimum.at(parent, hi, lo)
        while True:
            nxt = parent[parent]
            if (nxt == parent).all():
                break
            parent = nxt


def mask_components_host(masks, pick, I, deg, min_samples=1, min_points=1):
    """DBSCAN of every picked mask over one scene's kNN rows -- the statement gf_mask_components is tested against, in
    integers alone.  masks int32 [n_rows, N] (nonzero = member), pick int64 [p] rows of masks (a value outside
    [0, n_rows) is an empty row), rows I int32 [N, k] / deg int32 [N] read as gf_smooth_components reads them: columns
    0 .. min(deg[i], k - 1) of row i, an entry outside [0, N) skipped and never followed.  For pick rank r with member
    set M:
      cnt(i) = 1 + the read entries j of row i with j != i and j in M (a repeated entry counts each time);
      i in M is a CORE point when cnt(i) >= min_samples;
      a read entry (i, j) with both i and j core puts them in one cluster (one direction suffices), and a cluster's id
      is the smallest index among its core points;
      a member that is not core is a BORDER point: it takes the smallest cluster id among the core entries of its OWN
      row, and is noise (-1) without one;
      a cluster's size counts core and border points; one smaller than min_points is dissolved (all its points -1);
      the largest cluster of a pick has the greatest size, ties go to the smaller id.
    With min_samples = 1 this is connected components of the graph restricted to the mask; with complete symmetric
    rows it is sklearn.cluster.DBSCAN(eps, min_samples) on the mask's points with the clusters named by their smallest
    core index.  Returns (comp int32 [p, N]: the cluster id of every member point or -1, tab int32 [p, MSP_TABLE_INTS]:
    one GfMspRow of the header per rank)."""
    masks = np.asarray(_np(masks))
    pick = np.asarray(_np(pick)).astype(np.int64).reshape(-1)
    I, deg = np.asarray(_np(I)), np.asarray(_np(deg))
    if min_samples < 1 or min_points < 1:
        raise ValueError("mask_components_host: min_samples >= 1 and min_points >= 1")
    if masks.ndim != 2 or I.ndim != 2 or I.shape[0] != masks.shape[1] or deg.shape != (masks.shape[1],):
        raise ValueError(f"mask_components_host: expected masks [n_rows, N], I [N, k] and deg [N], got {masks.shape}, "
                         f"{I.shape}, {deg.shape}")
    n_rows, N = masks.shape
    p = pick.shape[0]
    comp = np.full((p, N), -1, np.int32)
    tab = np.zeros((p, MSP_TABLE_INTS), np.int32)
    tab[:, _MSP.largest] = -1
    if N == 0 or p == 0:
        return comp, tab
    src, col = np.nonzero(_valid_entries(I, deg, N))
    dst = I[src, col].astype(np.int64)
    other = dst != src
    src, dst = src[other], dst[other]
    done = {}
    for r, row in enumerate(pick.tolist()):
        if not 0 <= row < n_rows:
            continue
        if row in done:  # (a row picked twice: the same statement, the same result)
            comp[r], tab[r] = comp[done[row]], tab[done[row]]
            continue
        done[row] = r
        M = masks[row] != 0
        tab[r, _MSP.members] = M.sum()
        inside = M[src] & M[dst]
        cnt = 1 + np.bincount(src[inside], minlength=N)
        core = M & (cnt >= min_samples)
        both = core[src] & core[dst]
        root = _min_index_components(N, src[both], dst[both])
        ids = np.where(core, root, -1)
        edge = M[src] & ~core[src] & core[dst]  # a border point's own row only
        low = np.full(N, N, np.int64)
        np.minimum.at(low, src[edge], root[dst[edge]])
        border = M & ~core & (low < N)
        ids[border] = low[border]
        size = np.bincount(ids[ids >= 0], minlength=N)
        ids[(ids >= 0) & (size[np.maximum(ids, 0)] < min_points)] = -1
        comp[r] = ids
        kept = np.unique(ids[ids >= 0])  # ascending: argmax takes the smaller id among equal sizes
        tab[r, _MSP.clusters], tab[r, _MSP.kept_points] = len(kept), (ids >= 0).sum()
        if len(kept):
            big = kept[np.argmax(size[kept])]
            tab[r, _MSP.largest], tab[r, _MSP.largest_size] = big, size[big]
    return comp, tab


def mask_keep_largest_host(masks, pick, comp, tab):
    """The statement of gf_mask_keep_largest: a copy of masks in which every picked row keeps its values at the points of
    its largest kept cluster (mask_components_host's comp and tab) and is zero elsewhere."""
    masks = np.asarray(_np(masks))
    out = masks.copy()
    for r, row in enumerate(np.asarray(_np(pick)).reshape(-1).tolist()):
        if 0 <= row < masks.shape[0]:
            big = int(tab[r, _MSP.largest])
            out[row] = np.where((comp[r] == big) & (big >= 0), masks[row], 0)
    return out


def split_masks(masks, scores, cls, pick, xyz, *, radius=0.1, k=16, min_samples=1, min_points=50, mode="largest"):
    """Split the picked instance masks of one scene into spatially connected clusters (DBSCAN per mask, as query-based
    3D instance segmenters post-process their masks): a mask that fires on two objects at once, or on an object plus
    stray points far from it, is cleaned.  masks int32 [n, N], scores [n], cls [n], pick int64 [p] (the NMS result),
    xyz fp32 [N, 3]; the graph is knn_radius(xyz, k, radius), the clusters those of mask_components_host(min_samples,
    min_points).  Returns (cls', scores', masks', pick'):
      mode="largest"  masks' [n, N] with every picked row cut down to its largest kept cluster (all zero without one);
                      cls, scores and pick unchanged.  On the GPU nothing is read back.
      mode="split"    every kept cluster becomes a row of masks' int32 [n_out, N], ordered by pick rank, then cluster
                      id; scores' and cls' are those of the parent row, pick' = arange(n_out).  On the GPU the rows are
                      built by framework operations from comp (one comparison per row), and the number of kept clusters
                      is the one device-to-host read (torch.nonzero's).
    GPU tensors run csrc/mask_split.hip (pointops.mask_components / mask_keep_largest) on the current stream, CPU
    tensors the host statement.  A scene without proposals (masks = []) passes through."""
    if mode not in SPLIT_MODES:
        raise ValueError(f"split_masks: mode must be one of {SPLIT_MODES}, got {mode!r}")
    if not torch.is_tensor(masks):
        return cls, scores, masks, pick
    pick = pick.to(torch.int64)
    m32 = (masks if masks.dtype == torch.int32 else (masks != 0).int()).contiguous()
    if masks.is_cuda:
        from . import pointops

        pick = pick.to(masks.device).contiguous()
        _, I, deg = pointops.knn_radius(xyz.to(torch.float32).contiguous(), k, radius, sqrt_out=False)
        comp, tab = pointops.mask_components(m32, pick, I, deg, min_samples, min_points)
        if mode == "largest":
            return cls, scores, pointops.mask_keep_largest(m32, pick, comp, tab), pick
    else:
        I, deg = knn_radius_host(xyz, k, radius)
        comp, tab = mask_components_host(m32, pick, I, deg, min_samples, min_points)
        if mode == "largest":
            return cls, scores, torch.from_numpy(mask_keep_largest_host(m32, pick, comp, tab)), pick
        comp = torch.from_numpy(comp)
    # a kept cluster is named by its smallest core point, which carries its own index: one (rank, id) pair per cluster,
    # and nonzero lists them by rank, then id
    N = comp.shape[1]
    found = (comp == torch.arange(N, dtype=torch.int32, device=comp.device)[None, :]).nonzero()
    rank, ids = found[:, 0], found[:, 1]
    parent = pick[rank]
    out = (comp[rank] == ids[:, None].to(torch.int32)).to(torch.int32)
    return cls[parent], scores[parent], out, torch.arange(rank.shape[0], dtype=torch.int64, device=comp.device)


# ---- instances joined across the tiles of a large scan (csrc/tile_merge.hip): the host statement ------------------------
TILE_SCENE_FIELDS = _abi.const("GF_TILE_SCENE_FIELDS")
TILE_DEFAULTS = dict(iom=0.5, min_shared=20)


def _tile_rows(plan, per_tile):
    """The picked rows of all tiles, tile-major: per tile (masks int32 [n_rows, n_s] or None, pick int64 [p_s] on the
    host or the device, cls, scores), with the shapes checked against the plan."""
    T = plan.T
    if len(per_tile) != T:
        raise ValueError(f"merge_tiles: the plan has {T} tiles, got results of {len(per_tile)}")
    out = []
    for s, (cls, scores, masks, pick) in enumerate(per_tile):
        n_s = int(plan.offsets[s + 1] - plan.offsets[s])
        p_s = 0 if pick is None else int(len(pick))
        if p_s == 0 or isinstance(masks, (list, tuple)):
            if p_s:
                raise ValueError(f"merge_tiles: tile {s} has {p_s} picks and no masks")
            out.append((None, None, None, None))
            continue
        if masks.ndim != 2 or masks.shape[1] != n_s or len(cls) != masks.shape[0] or len(scores) != masks.shape[0]:
            raise ValueError(f"merge_tiles: tile {s}: masks {tuple(masks.shape)}, {len(cls)} classes and {len(scores)} "
                             f"scores do not fit the tile's {n_s} points")
        out.append((masks, pick, cls, scores))
    return out


def merge_tiles_host(plan, per_tile, *, iom=0.5, min_shared=20, return_tables=False):
    """Instances of a scan that was run as the tiles of `plan` (scene.tile_plan), joined across the tiles -- the
    statement csrc/tile_merge.hip is tested against, in integers alone.  per_tile: per tile (cls, scores, masks int32
    [n_rows_s, n_s], pick) as predict_batches yields them; a tile without picks may give [] for the first three.
      Rows are the picked masks of all tiles, tile-major and then by rank in pick: P of them, row_tile[r] the tile.
      inter[a, b], for rows of different tiles s, t: the points of the scan that lie in both tiles and in both masks.
      shared[a, t], for t other than a's tile: the points of mask a that also lie in tile t.
      Rows a, b are joined when cls[a] == cls[b], inter[a, b] >= min_shared and
      float64(inter[a, b]) >= iom * float64(min(shared[a, t], shared[b, s])): intersection over the smaller side
      WITHIN the region the two tiles share (not IoU: where a tile's border cuts an object, the part it holds must
      match the whole as the neighbour sees it).
      Instances are the connected components; the representative is the smallest row, global ids 0 .. G-1 follow the
      representatives in ascending order; the class is the members' common class, the score the largest member score
      (the same float), the mask the union of the members' masks over the scan's N points.
    Returns (cls int64 [G], scores fp32 [G], masks int32 [G, N], pick int64 [G]: the stable argsort of -scores,
    members int32 [P]: row -> global id); with return_tables also a dict of inter int32 [P, P], shared int32 [P, T],
    comp int32 [P], count int32 [G] and row_tile int32 [P]."""
    T, N = plan.T, plan.N
    rows = _tile_rows(plan, per_tile)
    A, row_tile, cls_all, sc_all, first = [], [], [], [], [0]
    for s, (masks, pick, cls, scores) in enumerate(rows):
        if masks is None:
            A.append(np.zeros((0, int(plan.offsets[s + 1] - plan.offsets[s])), bool))
        else:
            pk = np.asarray(_np(pick)).astype(np.int64).reshape(-1)
            m = np.asarray(_np(masks))
            ok = (pk >= 0) & (pk < m.shape[0])  # a pick outside the masks is an empty row
            a = np.zeros((pk.size, m.shape[1]), bool)
            a[ok] = m[pk[ok]] != 0
            A.append(a)
            safe = np.where(ok, pk, 0)
            cls_all.append(np.asarray(_np(cls)).astype(np.int64)[safe])
            sc_all.append(np.asarray(_np(scores)).astype(np.float32)[safe])
        row_tile += [s] * A[-1].shape[0]
        first.append(first[-1] + A[-1].shape[0])
    P = first[-1]
    row_tile = np.asarray(row_tile, np.int32)
    cls_all = np.concatenate(cls_all) if cls_all else np.zeros(0, np.int64)
    sc_all = np.concatenate(sc_all) if sc_all else np.zeros(0, np.float32)
    inter = np.zeros((P, P), np.int32)
    shared = np.zeros((P, T), np.int32)
    # the shared points of every pair of tiles, from the point tables: (s, t, index in s, index in t)
    for i in range(4):
        for j in range(i + 1, 4):
            both = plan.tile_of[:, j] >= 0
            s_, t_ = plan.tile_of[both, i].astype(np.int64), plan.tile_of[both, j].astype(np.int64)
            la, lb = plan.local_of[both, i], plan.local_of[both, j]
            key = s_ * T + t_
            for k in np.unique(key):
                sel = key == k
                s, t = int(k) // T, int(k) % T
                a, b = A[s][:, la[sel]], A[t][:, lb[sel]]
                if a.shape[0]:
                    shared[first[s]:first[s + 1], t] += a.sum(1, dtype=np.int32)
                if b.shape[0]:
                    shared[first[t]:first[t + 1], s] += b.sum(1, dtype=np.int32)
                if a.shape[0] and b.shape[0]:
                    blk = a.astype(np.int32) @ b.T.astype(np.int32)
                    inter[first[s]:first[s + 1], first[t]:first[t + 1]] += blk
                    inter[first[t]:first[t + 1], first[s]:first[s + 1]] += blk.T
    a, b = np.nonzero(np.triu(row_tile[:, None] != row_tile[None, :], 1))
    small = np.minimum(shared[a, row_tile[b]], shared[b, row_tile[a]])
    edge = (cls_all[a] == cls_all[b]) & (inter[a, b] >= min_shared) & \
           (inter[a, b].astype(np.float64) >= float(iom) * small.astype(np.float64))
    comp = _min_index_components(P, a[edge], b[edge])
    reps, members = np.unique(comp, return_inverse=True)
    members = members.reshape(-1).astype(np.int32)
    G = reps.size
    scores = np.full(G, -np.inf, np.float32)
    np.maximum.at(scores, members, sc_all)
    masks = np.zeros((G, N), np.int32)
    for s in range(T):
        idx = plan.points(s)
        for r in range(A[s].shape[0]):
            masks[members[first[s] + r], idx[A[s][r]]] = 1
    out = (cls_all[reps], scores, masks, np.argsort(-scores, kind="stable").astype(np.int64), members)
    if return_tables:
        out += (dict(inter=inter, shared=shared, comp=comp.astype(np.int32), count=masks.sum(1, dtype=np.int32),
                     row_tile=row_tile),)
    return out


def tile_scene_table(plan, rows):
    """(table int64 [T, GF_TILE_SCENE_FIELDS], sizes) of gf_tile_pack_picks / gf_tile_overlaps / gf_tile_assemble from
    _tile_rows' device tensors, one GfTileScene of the header per tile; sizes: P rows, uint32 words of the bitsets,
    row_tile int32 [P]."""
    table, recs = scene_table(plan.T, TILE_ROW)
    row = word = 0
    row_tile = []
    for s, (masks, pick, _, _) in enumerate(rows):
        n_s = int(plan.offsets[s + 1] - plan.offsets[s])
        p_s = 0 if masks is None else int(pick.shape[0])
        r = recs[s]
        r["n_s"], r["first_row"], r["first_word"] = n_s, row, word
        if p_s:
            r["masks"], r["n_rows"], r["pick"], r["p_s"] = masks.data_ptr(), masks.shape[0], pick.data_ptr(), p_s
        row += p_s
        word += n_s * ((p_s + 31) // 32)
        row_tile += [s] * p_s
    return table, dict(rows=row, words=word, row_tile=np.asarray(row_tile, np.int32))


def merge_tiles(plan, per_tile, *, iom=0.5, min_shared=20, return_tables=False):
    """merge_tiles_host on the tensors' device and the current stream (csrc/tile_merge.hip: pointops.tile_pack_picks,
    tile_overlaps, tile_merge, tile_assemble -- a fixed number of launches for any number of tiles and picks): the picked
    instances of a scan's tiles joined into (cls [G], scores [G], masks int32 [G, N], pick, members), every output
    bit-identical to the host statement and from call to call.  One device-to-host read, of G, sizes the dense output
    (4 * G * N bytes).  More than pointops.TILE_MAX_PICKS picks in a tile or TILE_MAX_ROWS in all is an error before
    anything is launched.  Host arrays (no tensor on a GPU among them) go to merge_tiles_host."""
    dev = next((x.device for tile in per_tile for x in tile if torch.is_tensor(x) and x.is_cuda), None)
    if dev is None:
        out = merge_tiles_host(plan, per_tile, iom=iom, min_shared=min_shared, return_tables=return_tables)
        if any(torch.is_tensor(x) for tile in per_tile for x in tile):
            out = tuple(torch.from_numpy(x) for x in out[:5]) + out[5:]
        return out
    from . import pointops

    T, N = plan.T, plan.N
    rows = []
    for masks, pick, cls, scores in _tile_rows(plan, per_tile):
        if masks is not None:
            masks = (masks if masks.dtype == torch.int32 else (masks != 0).int()).to(dev).contiguous()
            pick = torch.as_tensor(pick).to(dev, torch.int64).contiguous()
            cls, scores = torch.as_tensor(cls).to(dev, torch.int64), torch.as_tensor(scores).to(dev, torch.float32)
        rows.append((masks, pick, cls, scores))
    table, sizes = tile_scene_table(plan, rows)
    pointops.tile_check_caps(table)
    P = sizes["rows"]
    if P == 0:
        out = (torch.empty(0, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.float32, device=dev),
               torch.zeros((0, N), dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int64, device=dev),
               torch.empty(0, dtype=torch.int32, device=dev))
        if return_tables:
            z = torch.zeros(0, dtype=torch.int32, device=dev)
            out += (dict(inter=z.reshape(0, 0), shared=z.reshape(0, T), comp=z, count=z, row_tile=z),)
        return out
    # a pick outside the masks is an empty row: its class and score are those of row 0, as in the statement
    with_picks = [r for r in rows if r[0] is not None]
    safe = [torch.where((p >= 0) & (p < m.shape[0]), p, torch.zeros_like(p)) for m, p, _, _ in with_picks]
    cls_all = torch.cat([c[p] for (_, _, c, _), p in zip(with_picks, safe)]).contiguous()
    sc_all = torch.cat([s[p] for (_, _, _, s), p in zip(with_picks, safe)]).contiguous()
    table_d = pointops._table_dev(table, dev)
    tile_of = torch.from_numpy(plan.tile_of).to(dev, non_blocking=True)
    local_of = torch.from_numpy(plan.local_of).to(dev, non_blocking=True)
    row_tile = torch.from_numpy(sizes["row_tile"]).to(dev, non_blocking=True)
    bits = pointops.tile_pack_picks(table_d, table, sizes)
    inter, shared = pointops.tile_overlaps(table_d, table, tile_of, local_of, bits, P)
    comp, members, d_G, inst_cls, inst_scores = pointops.tile_merge(inter, shared, cls_all, sc_all, row_tile, iom,
                                                                    min_shared)
    G = int(d_G.item())  # the one read-back: the dense output is sized by it
    masks, count = pointops.tile_assemble(table_d, table, tile_of, local_of, bits, members, G)
    scores = inst_scores[:G]
    out = (inst_cls[:G], scores, masks, torch.sort(-scores, stable=True)[1], members)
    if return_tables:
        out += (dict(inter=inter, shared=shared, comp=comp, count=count, row_tile=row_tile),)
    return out


# ---- semantic scores stitched across the tiles of a large scan (csrc/tile_stitch.hip): the host statement ----------------
TILE_SCORE_FIELDS = _abi.const("GF_TILE_SCORE_FIELDS")
STITCH_MODES = ("core", "mean")


def _stitch_tiles_checked(plan, per_tile_scores, mode, who):
    """(C, the tiles' scores with None for every empty tile) of stitch_tiles / stitch_tiles_host, with the mode, the
    shapes against the plan and the dtype checked (ValueError); nothing is copied or moved."""
    if mode not in STITCH_MODES:
        raise ValueError(f"{who}: mode must be one of {STITCH_MODES}, got {mode!r}")
    if len(per_tile_scores) != plan.T:
        raise ValueError(f"{who}: the plan has {plan.T} tiles, got scores of {len(per_tile_scores)}")
    C, out = None, []
    for s, x in enumerate(per_tile_scores):
        n_s = int(plan.offsets[s + 1] - plan.offsets[s])
        if x is None:
            if n_s:
                raise ValueError(f"{who}: tile {s} holds {n_s} points and has no scores")
            out.append(None)
            continue
        f32 = x.dtype == torch.float32 if torch.is_tensor(x) else getattr(x, "dtype", None) == np.float32
        if not f32:
            raise ValueError(f"{who}: tile {s}: expected float32 scores, got {getattr(x, 'dtype', type(x).__name__)}")
        if x.ndim != 2 or x.shape[0] != n_s or x.shape[1] < 1:
            raise ValueError(f"{who}: tile {s}: expected scores [{n_s}, C], got {tuple(x.shape)}")
        if C is not None and x.shape[1] != C:
            raise ValueError(f"{who}: tile {s} has {x.shape[1]} classes, the tiles before {C}")
        C = int(x.shape[1])
        out.append(x if n_s else None)
    if C is None:
        raise ValueError(f"{who}: no tile gives the number of classes")
    return C, out


def stitch_tiles_host(plan, per_tile_scores, mode):
    """Per-point semantic scores fp32 [N, C] of a scan that was run as the tiles of `plan` (scene.tile_plan) -- the
    statement csrc/tile_stitch.hip is tested against, in exact float32.  per_tile_scores[s]: float32 [n_s, C], tile s'
    scores in the tile's own point order (plan.points(s)); None or [0, C] for an empty tile.
      A slot j of point g counts when tile_of[g, j] lies in [0, T) and local_of[g, j] in [0, n_s) of that tile (every
      slot with tile_of >= 0 of a plan made by scene.tile_plan); its row is per_tile_scores[tile_of[g, j]][local_of[g, j]].
      "core": out[g] = the row of the first slot j with tile_of[g, j] == core_of[g], the same words.  The core tile is
        the one that shows the point the most context: the point is at least halo away from that tile's outer edge and
        at most halo away from the outer edge of every other tile that holds it.
      "mean": over the slots j = 0..3 in that order (ascending tile id) that count: acc = row for the first one, then
        acc = acc + row in float32, one add per slot; out[g] = acc / float32(count), the IEEE division (exact for the
        counts 1, 2 and 4 that scene.tile_plan makes; correctly rounded for the 3 of a hand-built table).
      A point without such a slot (hand-built tables only) gets zeros.
    ValueError for scores that are not float32 [n_s, C] with one C, and for a mode outside the two."""
    C, tiles = _stitch_tiles_checked(plan, per_tile_scores, mode, "stitch_tiles_host")
    N, T = plan.N, plan.T
    flat = np.concatenate([np.zeros((0, C), np.float32)] + [np.asarray(_np(x)) for x in tiles if x is not None])
    n = np.diff(plan.offsets).astype(np.int64)  # (the row of (s, l) in flat is offsets[s] + l)
    tile_of, local_of = plan.tile_of.astype(np.int64), plan.local_of.astype(np.int64)
    safe = np.clip(tile_of, 0, T - 1)
    ok = (tile_of >= 0) & (tile_of < T) & (local_of >= 0) & (local_of < n[safe])
    row = np.where(ok, plan.offsets[safe] + local_of, 0)
    out = np.zeros((N, C), np.float32)
    if mode == "core":
        match = tile_of == plan.core_of.astype(np.int64)[:, None]
        g, j = np.nonzero(match & (np.cumsum(match, 1) == 1) & ok)
        out[g] = flat[row[g, j]]
        return out
    cnt = np.zeros(N, np.int64)
    for j in range(4):
        g = np.nonzero(ok[:, j])[0]
        v = flat[row[g, j]]
        out[g] = np.where((cnt[g] == 0)[:, None], v, out[g] + v)
        cnt[g] += 1
    g = np.nonzero(cnt)[0]
    out[g] = out[g] / cnt[g].astype(np.float32)[:, None]
    return out


def tile_score_table(tiles):
    """int64 [T, GF_TILE_SCORE_FIELDS] tile score table of gf_tile_stitch_scores, one GfTileScore of the header per
    tile: the tile's scores tensor [n_s, C], or None for an empty tile (a row of zeros)."""
    table, recs = scene_table(len(tiles), TILE_SCORE_ROW)
    for r, x in zip(recs, tiles):
        if x is not None:
            r["scores"], r["n_s"] = x.data_ptr(), x.shape[0]
    return table


def stitch_tiles(plan, per_tile_scores, mode):
    """stitch_tiles_host on the tensors' device and the current stream (csrc/tile_stitch.hip, one launch of
    pointops.tile_stitch_scores for any number of tiles): fp32 [N, C], bit-identical to the host statement and from call
    to call; nothing is read back.  The tiles' tensors must be float32 [n_s, C], contiguous and on one device (checked
    on the host against the plan, ValueError, before anything is launched; C above pointops.TILE_STITCH_MAX_CLASSES is
    pointops' RuntimeError).  Host arrays (no tensor on a GPU among them) go to stitch_tiles_host."""
    dev = next((x.device for x in per_tile_scores if torch.is_tensor(x) and x.is_cuda), None)
    if dev is None:
        out = stitch_tiles_host(plan, per_tile_scores, mode)
        return torch.from_numpy(out) if any(torch.is_tensor(x) for x in per_tile_scores) else out
    from . import pointops

    C, tiles = _stitch_tiles_checked(plan, per_tile_scores, mode, "stitch_tiles")
    for s, x in enumerate(tiles):
        if x is not None and not (torch.is_tensor(x) and x.device == dev and x.is_contiguous()):
            raise ValueError(f"stitch_tiles: tile {s}: expected a contiguous float32 tensor on {dev}")
    table = tile_score_table(tiles)
    if plan.N == 0:
        return torch.empty((0, C), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        return pointops.tile_stitch_scores(pointops._table_dev(table, dev),
                                           table, torch.from_numpy(plan.tile_of).to(dev, non_blocking=True),
                                           torch.from_numpy(plan.local_of).to(dev, non_blocking=True),
                                           torch.from_numpy(plan.core_of).to(dev, non_blocking=True), C, mode)


# ---- instances and scores joined across the views of a scan (csrc/view_merge.hip): the host statement --------------------
VIEW_DEFAULTS = dict(iou=0.5, min_views=None, vote=0.5)  # chosen by reasoning; no measurement stands behind them
VIEW_MAX_VIEWS = 32  # gf_view_merge_max_views(): asserted against the library in view_merge.view_limits()


def _view_args(V, iou, min_views, vote, who):
    """min_views (the default (V + 1) // 2 filled in) after the checks of the three parameters (ValueError)."""
    if not 1 <= V <= VIEW_MAX_VIEWS:
        raise ValueError(f"{who}: {V} views (1 to {VIEW_MAX_VIEWS})")
    if not float(iou) == float(iou):
        raise ValueError(f"{who}: iou is NaN")
    if not 0.0 < float(vote) <= 1.0:
        raise ValueError(f"{who}: vote in (0, 1], got {vote!r}")
    min_views = (V + 1) // 2 if min_views is None else int(min_views)
    if not 1 <= min_views <= V:
        raise ValueError(f"{who}: min_views in 1 .. V = {V}, got {min_views}")
    return min_views


def _view_rows(per_view, N, who):
    """Per view (masks [n_rows, N], pick [p_v], cls, scores), or four Nones for a view without picks, shapes checked."""
    out = []
    for v, (cls, scores, masks, pick) in enumerate(per_view):
        p_v = 0 if pick is None else int(len(pick))
        if p_v == 0 or isinstance(masks, (list, tuple)):
            if p_v:
                raise ValueError(f"{who}: view {v} has {p_v} picks and no masks")
            out.append((None, None, None, None))
            continue
        if masks.ndim != 2 or masks.shape[1] != N or masks.shape[0] < 1 or len(cls) != masks.shape[0] \
                or len(scores) != masks.shape[0]:
            raise ValueError(f"{who}: view {v}: masks {tuple(masks.shape)}, {len(cls)} classes and {len(scores)} "
                             f"scores do not fit [n_rows >= 1, {N}]")
        out.append((masks, pick, cls, scores))
    return out


def merge_views_host(per_view, N, *, iou=0.5, min_views=None, vote=0.5, return_tables=False):
    """Instances of a scan that was run under V views -- the same N points in the same order, rotated or mirrored --
    joined across the views: the statement csrc/view_merge.hip is tested against.  per_view: per view (cls, scores,
    masks [n_v, N], pick) as predict_batches yields them; a view without proposals gives ([], [], [], empty pick).
      Rows 0 .. P-1 are the picked rows, view-major and then by rank in pick; a pick outside the masks is an empty row.
      B[a] = the points of row a (masks != 0), cnt[a] = |B[a]|, inter[a, b] = |B[a] & B[b]|, union = cnt[a] + cnt[b] -
      inter.
      best[a, v], for every view v other than a's: among the rows b of view v with cls[b] == cls[a] and inter[a, b] > 0
      the one of the largest IoU, compared exactly (inter[a, b] * union[a, c] against inter[a, c] * union[a, b] in
      int64), the smaller row on ties, -1 without one.
      Rows a < b of different views join when best[a, view(b)] == b, best[b, view(a)] == a and
      float64(inter[a, b]) >= iou * float64(union[a, b]) (one multiplication, one compare): one to one between two
      views, so one sloppy mask cannot glue two neighbours of another view together through the threshold alone.
      Instances are the connected components (comp[r]: the smallest row).  support = the number of distinct views among
      the members; a component is kept when support >= min_views (default (V + 1) // 2) and its rows hold a point (an
      empty row joins nothing and is dropped).  Global ids 0 .. G-1 follow the kept representatives in ascending order.
      The class is the representative's (all members share it).  The score: m_v = the largest member score of view v,
      float32(0) without a member; acc = m_0, then acc = acc + m_v in float32 for v = 1 .. V-1; score = acc /
      float32(V), the IEEE division -- an instance that only some views found is marked down in proportion.
      The mask: votes[p] = the views with a member row that holds p (two rows of one view count once); p belongs to the
      instance when votes[p] > 0 and float64(votes[p]) >= vote * float64(support).  (With vote near 1 the mask of a
      chain whose ends do not meet can be empty; the instance stays, with count 0.)
    Returns (cls int64 [G], scores fp32 [G], masks int32 [G, N], pick int64 [G]: the stable argsort of -scores,
    tables); tables is None, or with return_tables a dict of inter int32 [P, P], cnt int32 [P], best int32 [P, V],
    comp int32 [P], members int32 [P] (row -> global id, -1 dropped), support int32 [G], count int32 [G] and row_view
    int32 [P]."""
    per_view = list(per_view)
    V, N = len(per_view), int(N)
    min_views = _view_args(V, iou, min_views, vote, "merge_views_host")
    rows = _view_rows(per_view, N, "merge_views_host")
    A, cls_all, sc_all, first = [], [], [], [0]
    for masks, pick, cls, scores in rows:
        if masks is None:
            first.append(first[-1])
            continue
        pk = np.asarray(_np(pick)).astype(np.int64).reshape(-1)
        m = np.asarray(_np(masks))
        ok = (pk >= 0) & (pk < m.shape[0])
        a = np.zeros((pk.size, N), bool)
        a[ok] = m[pk[ok]] != 0
        A.append(a)
        safe = np.where(ok, pk, 0)  # (an empty row's class and score are never used: it is dropped)
        cls_all.append(np.asarray(_np(cls)).astype(np.int64)[safe])
        sc_all.append(np.asarray(_np(scores)).astype(np.float32)[safe])
        first.append(first[-1] + pk.size)
    P = first[-1]
    B = np.concatenate(A) if A else np.zeros((0, N), bool)
    cls_all = np.concatenate(cls_all) if cls_all else np.zeros(0, np.int64)
    sc_all = np.concatenate(sc_all) if sc_all else np.zeros(0, np.float32)
    row_view = np.repeat(np.arange(V, dtype=np.int32), np.diff(first))
    inter = np.zeros((P, P), np.int64)
    for s in range(0, N, 1 << 16):  # float32 products of 0 / 1 over at most 2^16 points: exact
        blk = B[:, s:s + (1 << 16)].astype(np.float32)
        inter += (blk @ blk.T).astype(np.int64)
    cnt = B.sum(1, dtype=np.int64)
    best = np.full((P, V), -1, np.int32)
    for a in range(P):
        for v in range(V):
            if v == row_view[a]:
                continue
            b0 = first[v]
            cand = b0 + np.nonzero((inter[a, b0:first[v + 1]] > 0) & (cls_all[b0:first[v + 1]] == cls_all[a]))[0]
            bi, bu, bx = 0, 1, -1
            for b in cand.tolist():
                i = int(inter[a, b])
                u = int(cnt[a] + cnt[b]) - i
                if bx < 0 or i * bu > bi * u:  # ascending b: a tie keeps the smaller row
                    bi, bu, bx = i, u, b
            best[a, v] = bx
    ea, eb = [], []
    for a in range(P):
        for v in range(V):
            b = int(best[a, v])
            if b > a and best[b, row_view[a]] == a:
                union = cnt[a] + cnt[b] - inter[a, b]
                if np.float64(inter[a, b]) >= np.float64(iou) * np.float64(union):
                    ea.append(a)
                    eb.append(b)
    comp = _min_index_components(P, np.asarray(ea, np.int64), np.asarray(eb, np.int64)).astype(np.int64)
    reps = np.unique(comp)
    support_of = {int(r): len(set(row_view[comp == r].tolist())) for r in reps}
    kept = [int(r) for r in reps if support_of[int(r)] >= min_views and cnt[r] > 0]
    gid_of = {r: g for g, r in enumerate(kept)}
    members = np.asarray([gid_of.get(int(c), -1) for c in comp], np.int32).reshape(P)
    G = len(kept)
    scores = np.zeros(G, np.float32)
    masks = np.zeros((G, N), np.int32)
    support = np.asarray([support_of[r] for r in kept], np.int32).reshape(G)
    for g, r in enumerate(kept):
        rows_g = np.nonzero(comp == r)[0]
        votes = np.zeros(N, np.int64)
        acc = None
        for v in range(V):
            rv = rows_g[row_view[rows_g] == v]
            m = sc_all[rv].max() if rv.size else np.float32(0.0)
            acc = np.float32(m) if acc is None else np.float32(acc + np.float32(m))
            if rv.size:
                votes += B[rv].any(0)
        scores[g] = np.float32(acc / np.float32(V))
        masks[g] = (votes > 0) & (votes.astype(np.float64) >= np.float64(vote) * np.float64(support[g]))
    tables = None
    if return_tables:
        tables = dict(inter=inter.astype(np.int32), cnt=cnt.astype(np.int32), best=best, comp=comp.astype(np.int32),
                      members=members, support=support, count=masks.sum(1, dtype=np.int32), row_view=row_view)
    return (cls_all[kept].reshape(G), scores, masks, np.argsort(-scores, kind="stable").astype(np.int64), tables)


def view_scene_table(rows, N):
    """(table int64 [V, GF_TILE_SCENE_FIELDS], sizes) of gf_view_pack from _view_rows' device tensors, one GfTileScene
    of the header per view (n_s = N, first_word unused); sizes: P rows, row_view int32 [P], view_first int32 [V + 1]."""
    table, recs = scene_table(len(rows), TILE_ROW)
    row, first = 0, [0]
    for v, (masks, pick, _, _) in enumerate(rows):
        p_v = 0 if masks is None else int(pick.shape[0])
        r = recs[v]
        r["n_s"], r["first_row"] = N, row
        if p_v:
            r["masks"], r["n_rows"], r["pick"], r["p_s"] = masks.data_ptr(), masks.shape[0], pick.data_ptr(), p_v
        row += p_v
        first.append(row)
    first = np.asarray(first, np.int32)
    return table, dict(rows=row, row_view=np.repeat(np.arange(len(rows), dtype=np.int32), np.diff(first)),
                       view_first=first)


def merge_views(per_view, N, *, iou=0.5, min_views=None, vote=0.5, return_tables=False):
    """merge_views_host on the tensors' device and the current stream (csrc/view_merge.hip: view_merge.view_pack,
    view_overlaps, view_best, view_merge, view_assemble -- five launches for any number of views and picks): (cls [G],
    scores [G], masks int32 [G, N], pick, tables), every output bit-identical to the host statement and from call to
    call.  One device-to-host read, of G, sizes the dense output (4 * G * N bytes).  More than view_merge.VIEW_MAX_VIEWS
    views or VIEW_MAX_ROWS picked rows in all is an error before anything is launched.  Host arrays (no tensor on a GPU
    among them) go to merge_views_host."""
    per_view = list(per_view)
    dev = next((x.device for view in per_view for x in view if torch.is_tensor(x) and x.is_cuda), None)
    if dev is None:
        out = merge_views_host(per_view, N, iou=iou, min_views=min_views, vote=vote, return_tables=return_tables)
        if any(torch.is_tensor(x) for view in per_view for x in view):
            out = tuple(torch.from_numpy(x) for x in out[:4]) + out[4:]
        return out
    from . import pointops, view_merge

    V, N = len(per_view), int(N)
    min_views = _view_args(V, iou, min_views, vote, "merge_views")
    rows = []
    for masks, pick, cls, scores in _view_rows(per_view, N, "merge_views"):
        if masks is not None:
            masks = (masks if masks.dtype == torch.int32 else (masks != 0).int()).to(dev).contiguous()
            pick = torch.as_tensor(pick).to(dev, torch.int64).contiguous()
            cls, scores = torch.as_tensor(cls).to(dev, torch.int64), torch.as_tensor(scores).to(dev, torch.float32)
        rows.append((masks, pick, cls, scores))
    table, sizes = view_scene_table(rows, N)
    P = view_merge.view_check_caps(table, N)
    with torch.cuda.device(dev):
        with_picks = [r for r in rows if r[0] is not None]
        safe = [torch.where((p >= 0) & (p < m.shape[0]), p, torch.zeros_like(p)) for m, p, _, _ in with_picks]
        i64, f32 = dict(dtype=torch.int64, device=dev), dict(dtype=torch.float32, device=dev)
        cls_all = torch.cat([c[p] for (_, _, c, _), p in zip(with_picks, safe)] + [torch.empty(0, **i64)]).contiguous()
        sc_all = torch.cat([s[p] for (_, _, _, s), p in zip(with_picks, safe)] + [torch.empty(0, **f32)]).contiguous()
        table_d = pointops._table_dev(table, dev)
        row_view = torch.from_numpy(sizes["row_view"]).to(dev, non_blocking=True)
        view_first = torch.from_numpy(sizes["view_first"]).to(dev, non_blocking=True)
        bits, cnt = view_merge.view_pack(table_d, table, N)
        inter = view_merge.view_overlaps(bits, N)
        best = view_merge.view_best(inter, cnt, cls_all, row_view, view_first)
        merged = view_merge.view_merge(inter, cnt, best, cls_all, sc_all, row_view, iou, min_views)
        G = int(merged["G"].item())  # the one read-back: the dense output is sized by it
        masks, count = view_merge.view_assemble(bits, merged, row_view, G, N, vote)
    scores = merged["scores"][:G]
    tables = None
    if return_tables:
        tables = dict(inter=inter, cnt=cnt, best=best, comp=merged["comp"], members=merged["members"],
                      support=merged["support"][:G], count=count, row_view=row_view)
    return merged["cls"][:G], scores, masks, torch.sort(-scores, stable=True)[1], tables


def _mean_views_checked(per_view_scores, who):
    """(N, C) of the views' scores after the checks: 1 .. 32 float32 arrays or tensors of one shape [N, C >= 1]."""
    xs = list(per_view_scores)
    if not 1 <= len(xs) <= VIEW_MAX_VIEWS:
        raise ValueError(f"{who}: {len(xs)} views (1 to {VIEW_MAX_VIEWS})")
    for v, x in enumerate(xs):
        f32 = x.dtype == torch.float32 if torch.is_tensor(x) else getattr(x, "dtype", None) == np.float32
        if not f32:
            raise ValueError(f"{who}: view {v}: expected float32 scores, got {getattr(x, 'dtype', type(x).__name__)}")
        if x.ndim != 2 or x.shape[1] < 1 or tuple(x.shape) != tuple(xs[0].shape):
            raise ValueError(f"{who}: view {v}: expected scores {tuple(xs[0].shape)} = [N, C], got {tuple(x.shape)}")
    return int(xs[0].shape[0]), int(xs[0].shape[1])


def mean_views_host(per_view_scores):
    """fp32 [N, C]: the mean of the V views' semantic scores (each float32 [N, C] over the scan's own points) -- the
    statement gf_view_mean_scores is tested against, in exact float32: acc = s_0, then acc = acc + s_v for v = 1 .. V-1,
    one rounded add per view, and acc / float32(V), the IEEE division."""
    xs = list(per_view_scores)
    _mean_views_checked(xs, "mean_views_host")
    acc = np.array(_np(xs[0]), np.float32)
    for x in xs[1:]:
        acc = acc + np.asarray(_np(x), np.float32)
    return acc / np.float32(len(xs))


def mean_views(per_view_scores):
    """mean_views_host on the tensors' device and the current stream (one launch of view_merge.view_mean_scores for any
    number of views, no atomics, nothing read back): fp32 [N, C], bit-identical to the host statement and from call to
    call.  The tensors must be float32 [N, C], contiguous and on one device (ValueError before anything is launched; C
    above view_merge.TILE_STITCH_MAX_CLASSES is view_merge's RuntimeError).  Host arrays go to mean_views_host."""
    xs = list(per_view_scores)
    dev = next((x.device for x in xs if torch.is_tensor(x) and x.is_cuda), None)
    if dev is None:
        out = mean_views_host(xs)
        return torch.from_numpy(out) if any(torch.is_tensor(x) for x in xs) else out
    from . import pointops, view_merge

    N, C = _mean_views_checked(xs, "mean_views")
    for v, x in enumerate(xs):
        if not (torch.is_tensor(x) and x.device == dev and x.is_contiguous()):
            raise ValueError(f"mean_views: view {v}: expected a contiguous float32 tensor on {dev}")
    table = tile_score_table(xs)
    with torch.cuda.device(dev):
        return view_merge.view_mean_scores(pointops._table_dev(table, dev), table, N, C)


# ---- scans of any density: grid subsample, labels carried back (csrc/resample.hip) ---------------------------------------
GRID_MODES = ("first", "center")
GRID_AXIS_CELLS = 1 << 21  # gf_grid_subsample_max_cells(): asserted against the library in pointops.resample_limits()


def _xyz3(xyz, name):
    x = _np(xyz)
    if x.ndim != 2 or x.shape[1] != 3:
        raise ValueError(f"{name}: expected [n, 3], got {x.shape}")
    return np.ascontiguousarray(x, dtype=np.float32)


def _grid_args(cell, mode, who):
    if mode not in GRID_MODES:
        raise ValueError(f"{who}: mode must be one of {GRID_MODES}, got {mode!r}")
    c = np.float32(cell)
    if not (c > 0 and np.isfinite(c)):
        raise ValueError(f"{who}: cell must be positive and finite in float32, got {cell!r}")
    return c


def grid_subsample_host(xyz, cell, mode="center", origin=None):
    """(rep int32 [M], cell_of int32 [N], count int32 [M]): one representative point per occupied cell of a grid of
    `cell` metres -- the statement gf_grid_subsample is held to, bit for bit.  All arithmetic is float32, in the order
    written.  xyz float32 [N, 3]; origin float32 [3], default xyz.min(0).  t = (xyz - origin) / cell, c = floor(t); a
    point is valid when t is finite and 0 <= c < 2^21 on every axis, and any invalid point is a ValueError.  Cells (key
    cx | cy << 21 | cz << 42) are numbered in ascending order of their lowest point index -- the order of first
    occurrence, in both modes.  mode "first": rep[m] is that lowest index; "center": the point of the cell minimising
    (d2, index) with ctr = origin + (c + 0.5) * cell, d = xyz - ctr, d2 = (dx dx + dy dy) + dz dz.  Representatives are
    real points: every column of a scene goes through by one gather, nothing is averaged.  cell_of[rep[m]] == m,
    count.sum() == N, rep ascends in "first" mode; N = 0 gives empty outputs."""
    x = _xyz3(xyz, "grid_subsample_host: xyz")
    cell = _grid_args(cell, mode, "grid_subsample_host")
    N = x.shape[0]
    if origin is not None:
        origin = np.ascontiguousarray(_np(origin), dtype=np.float32)
        if origin.shape != (3,):
            raise ValueError(f"grid_subsample_host: origin: expected [3], got {origin.shape}")
    if N == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32)
    with np.errstate(all="ignore"):
        if origin is None:
            origin = x.min(0)
        t = (x - origin) / cell
        c = np.floor(t)
        bad = ~(np.isfinite(t) & (c >= 0) & (c < GRID_AXIS_CELLS)).all(1)
    if bad.any():
        raise ValueError(f"grid_subsample_host: {int(bad.sum())} point(s) outside the grid (not finite, below the origin "
                         f"or {GRID_AXIS_CELLS} cells or more from it); the first is point {int(np.nonzero(bad)[0][0])}")
    ci = c.astype(np.int64)
    key = ci[:, 0] | ci[:, 1] << 21 | ci[:, 2] << 42
    order = np.argsort(key, kind="stable")           # groups of equal keys, each in ascending point order
    head = np.r_[True, key[order][1:] != key[order][:-1]]
    lowest = order[head]                             # a group's lowest point index
    M = lowest.shape[0]
    number = np.empty(M, np.int64)
    number[np.argsort(lowest)] = np.arange(M)        # groups numbered by ascending lowest index
    cell_of = np.empty(N, np.int32)
    cell_of[order] = number[np.cumsum(head) - 1]
    count = np.bincount(cell_of, minlength=M).astype(np.int32)
    if mode == "first":
        return np.sort(lowest).astype(np.int32), cell_of, count
    with np.errstate(all="ignore"):
        d = x - (origin + (c + np.float32(0.5)) * cell)
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    by = np.lexsort((np.arange(N), d2, cell_of))     # per cell, ascending (d2, index)
    rep = by[np.r_[True, cell_of[by][1:] != cell_of[by][:-1]]]
    return rep.astype(np.int32), cell_of, count


def nearest_point_host(query, xyz, max_dist, chunk_elems=1 << 22):
    """(idx int32 [Q], d2 float32 [Q]): for every query the point of xyz minimising (d2, index) among those with
    d2 <= r2 -- the statement gf_nearest_point is held to, bit for bit.  float32 throughout: r2 = max_dist * max_dist,
    d2 = (dx dx + dy dy) + dz dz of d = query - point.  (-1, inf) with no candidate or for a query with a non-finite
    coordinate; a point with a non-finite coordinate is never a candidate.  Brute force, in chunks of queries."""
    q = _xyz3(query, "nearest_point_host: query")
    p = _xyz3(xyz, "nearest_point_host: xyz")
    md = np.float32(max_dist)
    if not (md > 0 and np.isfinite(md)):
        raise ValueError(f"nearest_point_host: max_dist must be positive and finite in float32, got {max_dist!r}")
    Q, n = q.shape[0], p.shape[0]
    idx = np.full(Q, -1, np.int32)
    out = np.full(Q, np.inf, np.float32)
    if Q == 0 or n == 0:
        return idx, out
    none = np.uint32(0xFFFFFFFF)
    with np.errstate(all="ignore"):
        r2 = md * md
        p_ok = np.isfinite(p).all(1)
        step = max(1, chunk_elems // n)
        for lo in range(0, Q, step):
            qs = q[lo:lo + step]
            d = qs[:, None, :] - p[None, :, :]
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            cand = (d2 <= r2) & p_ok[None, :] & np.isfinite(qs).all(1)[:, None]
            bits = np.where(cand, d2.view(np.uint32), none)  # d2 >= +0: the bit patterns ascend with the values
            j = bits.argmin(1)                               # the first minimum: the lowest index
            b = bits[np.arange(qs.shape[0]), j]
            hit = b != none
            idx[lo:lo + step] = np.where(hit, j, -1)
            out[lo:lo + step] = np.where(hit, b, np.uint32(0x7F800000)).astype(np.uint32).view(np.float32)
    return idx, out


def _parent(parent, n, who):
    if not torch.is_tensor(parent) or parent.dim() != 1 or parent.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{who}: parent: expected an int32 or int64 tensor [N]")
    if parent.numel() and int(parent.max()) >= n:
        raise ValueError(f"{who}: parent holds {int(parent.max())}, the source has {n} rows")
    return parent.long()


def expand_rows(rows, parent, fill=0):
    """out [N, C] (or [N]) = rows[parent] with `fill` where parent < 0: the rows [n, C] (or [n]) of a subsampled scene
    (or of another point set) on the N points whose parent is given -- grid_subsample's cell_of, nearest_point's idx.  A
    pure copy (one gather) on rows' device."""
    if not torch.is_tensor(rows) or rows.dim() not in (1, 2):
        raise ValueError("expand_rows: rows: expected a tensor [n, C] or [n]")
    p = _parent(parent, rows.shape[0], "expand_rows").to(rows.device)
    if rows.shape[0] == 0:
        return rows.new_full((p.shape[0], *rows.shape[1:]), fill)
    lost = p < 0
    return rows[p.clamp(min=0)].masked_fill_(lost if rows.dim() == 1 else lost[:, None], fill)


def expand_masks(masks, parent):
    """masks int32 [R, N] over the N points of a scan from masks [R, n] over its subsampled points: column g is column
    parent[g], zero where parent < 0.  A pure copy."""
    if not torch.is_tensor(masks) or masks.dim() != 2:
        raise ValueError("expand_masks: masks: expected a tensor [R, n]")
    p = _parent(parent, masks.shape[1], "expand_masks").to(masks.device)
    if masks.shape[1] == 0:
        return masks.new_zeros((masks.shape[0], p.shape[0]))
    return masks[:, p.clamp(min=0)].masked_fill_((p < 0)[None, :], 0)


def transfer(values, xyz_src, xyz_dst, max_dist, fill=0):
    """values [n, C] (or [n]) of the points xyz_src carried to the points xyz_dst [N, 3]: every destination takes the
    row of its nearest source point within max_dist (pointops.nearest_point; ties to the lower index) or `fill` without
    one.  Returns (out [N, C] or [N], idx int32 [N])."""
    from . import pointops

    if not torch.is_tensor(values) or values.shape[0] != xyz_src.shape[0]:
        raise ValueError(f"transfer: values: expected a tensor with one row per source point [{xyz_src.shape[0]}, ...]")
    idx, _ = pointops.nearest_point(xyz_dst, xyz_src, max_dist)
    return expand_rows(values, idx, fill), idx


# ---- 3D boxes of instances and the IoU of boxes (csrc/boxes.hip) ---------------------------------------------------------
BOX_SCENE_FIELDS = _abi.const("GF_BOX_SCENE_FIELDS")
BOX_FLOATS = _abi.const("GF_BOX_FLOATS")
BOX_IOU_FIELDS = _abi.const("GF_BOX_IOU_FIELDS")
BOX_FORMS = {"rows": _abi.const("GF_BOX_FORM_ROWS"), "ids": _abi.const("GF_BOX_FORM_IDS")}
BOX_MAX_ANGLES = 192    # gf_box_max_angles(): asserted against the library in pointops.box_limits()
BOX_MAX_GROUPS = 65535  # gf_box_max_groups()
BOX_ANGLES = 90         # headings over [0, 90 degrees): one per degree
_BOX_HOST_SLICE = 1 << 15  # members of a group taken at a time by the statement (bounds its [m, A] temporaries)


class Boxes(NamedTuple):
    """One upright box per group (numpy arrays, or tensors on the inputs' device).  size[:, 0] lies along (cos, sin),
    size[:, 1] along (-sin, cos), size[:, 2] along z; an empty group is all zeros."""
    center: object  # float64 [p, 3]
    size: object  # float64 [p, 3]
    cos: object  # float64 [p]: the fp32 table entry, widened
    sin: object  # float64 [p]
    yaw: object  # float64 [p]: radians about z, angle_index * (pi / 2) / angles
    angle_index: object  # int32 [p]
    count: object  # int32 [p]: points of the group
    rows: object = None  # float64 [p, BOX_FLOATS]: the packed rows as the kernels write and read them


def box_angle_table(angles=BOX_ANGLES):
    """fp32 [A, 2] = (cos, sin) of A equal steps over [0, 90 degrees), computed in float64 and rounded once."""
    A = int(angles)
    if not 1 <= A <= BOX_MAX_ANGLES or A != angles:
        raise ValueError(f"boxes: angles must be an integer in [1, {BOX_MAX_ANGLES}], got {angles!r}")
    th = np.arange(A, dtype=np.float64) * (np.pi / 2 / A)
    return np.stack([np.cos(th), np.sin(th)], axis=1).astype(np.float32)


_BOX = _columns("GfBox")


def _boxes_from_rows(rows, count, A):
    b = _BOX
    idx = rows[:, b.angle]
    i32 = idx.to(torch.int32) if torch.is_tensor(idx) else idx.astype(np.int32)
    return Boxes(rows[:, b.cx:b.cz + 1], rows[:, b.du:b.dz + 1], rows[:, b.c], rows[:, b.s], idx * (np.pi / 2 / A), i32,
                 count, rows)


def _box_rows_of(b):
    """float64 [p, BOX_FLOATS] of a Boxes (or of packed rows given as they are)."""
    if not isinstance(b, Boxes):
        return b
    if b.rows is not None:
        return b.rows
    if torch.is_tensor(b.center):
        rows = torch.empty((b.center.shape[0], BOX_FLOATS), dtype=torch.float64, device=b.center.device)
        center, size = b.center, b.size
    else:
        center, size = np.asarray(b.center, np.float64).reshape(-1, 3), np.asarray(b.size, np.float64).reshape(-1, 3)
        rows = np.empty((center.shape[0], BOX_FLOATS))
    c = _BOX
    rows[:, c.cx:c.cz + 1], rows[:, c.du:c.dz + 1] = center, size
    for at, v in ((c.c, b.cos), (c.s, b.sin), (c.angle, b.angle_index), (c.count, b.count)):
        rows[:, at] = v if torch.is_tensor(v) else np.asarray(v, dtype=np.float64).reshape(-1)
    return rows


def _float_keys(a):
    """fp32 -> uint32 whose integer order is the float order (gf_float_key: -0 below +0)."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def _float_unkeys(k):
    k = np.asarray(k, dtype=np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def _box_row(ulo, uhi, vlo, vhi, zlo, zhi, c, s, index, count):
    d = np.float64
    ulo, uhi, vlo, vhi, zlo, zhi, c, s = (d(v) for v in (ulo, uhi, vlo, vhi, zlo, zhi, c, s))
    lu, lv = (ulo + uhi) * d(0.5), (vlo + vhi) * d(0.5)
    row, b = np.empty(BOX_FLOATS), _BOX
    row[b.cx], row[b.cy], row[b.cz] = lu * c - lv * s, lu * s + lv * c, (zlo + zhi) * d(0.5)
    row[b.du], row[b.dv], row[b.dz] = uhi - ulo, vhi - vlo, zhi - zlo
    row[b.c], row[b.s], row[b.angle], row[b.count] = c, s, d(index), d(count)
    return row


def _box_rows_host(members, xyz, table):
    """(count int32 [p], aligned float64 [p, 10], oriented float64 [p, 10]) of the groups whose member indices are given:
    the statement of gf_instance_boxes_batched.  numpy rounds every ufunc on its own, in the kernel's order."""
    p, A = len(members), table.shape[0]
    c, s = np.ascontiguousarray(table[:, 0]), np.ascontiguousarray(table[:, 1])
    count = np.zeros(p, np.int32)
    aligned, oriented = np.zeros((p, BOX_FLOATS)), np.zeros((p, BOX_FLOATS))
    for r, idx in enumerate(members):
        m = count[r] = idx.shape[0]
        if m == 0:
            continue
        lo = np.full(2 * A + 3, 0xFFFFFFFF, np.uint32)  # keys of u [A], v [A], x, y, z
        hi = np.zeros(2 * A + 3, np.uint32)
        for b in range(0, m, _BOX_HOST_SLICE):
            q = xyz[idx[b:b + _BOX_HOST_SLICE]]
            x, y = q[:, 0:1], q[:, 1:2]
            u = x * c[None, :] + y * s[None, :]  # fp32: two products and a sum, each rounded
            v = y * c[None, :] - x * s[None, :]
            k = _float_keys(np.concatenate([u, v, q], axis=1))
            lo, hi = np.minimum(lo, k.min(0)), np.maximum(hi, k.max(0))
        lo, hi = _float_unkeys(lo), _float_unkeys(hi)
        area = (hi[:A] - lo[:A]) * (hi[A:2 * A] - lo[A:2 * A])  # fp32
        a = int(np.argmin(area))  # the first of the least
        z = (lo[2 * A + 2], hi[2 * A + 2])
        aligned[r] = _box_row(lo[2 * A], hi[2 * A], lo[2 * A + 1], hi[2 * A + 1], *z, np.float32(1), np.float32(0), 0, m)
        oriented[r] = _box_row(lo[a], hi[a], lo[A + a], hi[A + a], *z, c[a], s[a], a, m)
    return count, aligned, oriented


def _xyz_host(xyz):
    return np.ascontiguousarray(_np(xyz), dtype=np.float32).reshape(-1, 3)


def instance_boxes_host(masks, pick, xyz, angles=BOX_ANGLES):
    """The statement of the rows form: (count, aligned rows, oriented rows) of the groups masks[pick[r]] != 0 over xyz
    [N, 3].  A pick outside the masks is an empty group; masks may overlap."""
    table = box_angle_table(angles)
    xyz = _xyz_host(xyz)
    pick = np.asarray(_np(pick), dtype=np.int64).reshape(-1)
    masks = _np(masks)
    masks = masks.reshape(-1, xyz.shape[0]) if masks.size else np.zeros((0, xyz.shape[0]), np.int32)
    none = np.zeros(0, np.int64)
    return _box_rows_host([np.nonzero(masks[r])[0] if 0 <= r < masks.shape[0] else none for r in pick], xyz, table)


def id_boxes_host(group, n_groups, xyz, angles=BOX_ANGLES):
    """The statement of the ids form: the groups {i : group[i] == r} for r in [0, n_groups)."""
    table = box_angle_table(angles)
    xyz = _xyz_host(xyz)
    g = np.asarray(_np(group)).reshape(-1)
    if g.shape[0] != xyz.shape[0]:
        raise ValueError(f"id_boxes: group [{g.shape[0]}] against {xyz.shape[0]} points")
    order = np.argsort(g, kind="stable")
    cuts = np.searchsorted(g[order], np.arange(int(n_groups) + 1))
    return _box_rows_host([order[cuts[r]:cuts[r + 1]] for r in range(int(n_groups))], xyz, table)


def box_scene_table(forms, widths, ns, ps, group_ptrs, pick_ptrs, xyz_ptrs):
    """(int64 [S, BOX_SCENE_FIELDS] box scene table, sizes) for scenes of ps[b] groups over widths[b] points; forms[b]:
    "rows" (ns[b] masks, pick_ptrs[b]) or "ids".  sizes: the rows in total and the largest per-scene point / group
    counts of the launches."""
    N = np.asarray(widths, dtype=np.int64).reshape(-1)
    n = np.asarray(ns, dtype=np.int64).reshape(-1)
    p = np.asarray(ps, dtype=np.int64).reshape(-1)
    if (n < 0).any() or (N < 0).any() or (p < 0).any():
        raise ValueError("box_scene_table: negative size")
    if (p > BOX_MAX_GROUPS).any():
        raise ValueError(f"boxes: at most {BOX_MAX_GROUPS} groups per scene, got {int(p.max())}")
    S = N.shape[0]
    t, r = scene_table(S, BOX_SCENE_ROW)
    r["form"] = [BOX_FORMS[f] for f in forms]
    r["N"], r["n"], r["p"] = N, n, p
    r["group"] = np.asarray(group_ptrs, dtype=np.int64)
    r["pick"] = np.asarray(pick_ptrs, dtype=np.int64)
    r["xyz"] = np.asarray(xyz_ptrs, dtype=np.int64)
    r["row_off"] = _excl(p)
    sizes = {"rows": int(p.sum()), "max_points": int(N.max()) if S else 0, "max_groups": int(p.max()) if S else 0}
    return t, sizes


def box_iou_table(Ps, Gs):
    """(int64 [S, BOX_IOU_FIELDS] IoU table, sizes) for scenes of Ps[b] boxes against Gs[b]: offsets of each scene's rows
    in the packed arrays and of its [P, G] block."""
    P = np.asarray(Ps, dtype=np.int64).reshape(-1)
    G = np.asarray(Gs, dtype=np.int64).reshape(-1)
    if P.shape != G.shape or (P < 0).any() or (G < 0).any():
        raise ValueError("box_iou_table: one non-negative count per scene in both lists")
    S = P.shape[0]
    t, r = scene_table(S, BOX_IOU_ROW)
    r["P"], r["G"], r["a_off"], r["b_off"], r["out_off"] = P, G, _excl(P), _excl(G), _excl(P * G)
    sizes = {"a": int(P.sum()), "b": int(G.sum()), "out": int((P * G).sum()), "max_pairs": int((P * G).max()) if S else 0}
    return t, sizes


_box_tables_dev = {}


def _box_angles_dev(A, dev):
    t = _box_tables_dev.get((dev, A))
    if t is None:
        t = _box_tables_dev[dev, A] = torch.from_numpy(box_angle_table(A)).to(dev)
    return t


def _boxes_packed(specs, angles):
    """One gf_instance_boxes_batched call over scenes of either form: specs = ("rows", masks, pick, xyz) or ("ids",
    group, n_groups, xyz) per scene.  Returns (scene table (host), count int32 [rows], aligned, oriented float64
    [rows, BOX_FLOATS]) on the device."""
    from . import pointops

    box_angle_table(angles)  # (checks the range)
    dev = next((s[3].device for s in specs if torch.is_tensor(s[3])), None)
    if dev is None or dev.type != "cuda":
        raise RuntimeError("boxes: the kernels run on the GPU; instance_boxes / id_boxes have the numpy path")
    keep, forms, Ns, ns, ps, gp, pp, xp = [], [], [], [], [], [], [], []
    for form, g, pk, x in specs:
        x = torch.as_tensor(x, device=dev).to(torch.float32).reshape(-1, 3).contiguous()
        N = x.shape[0]
        if form == "rows":
            pk = torch.as_tensor(pk, device=dev).to(torch.int64).reshape(-1).contiguous()
            if torch.is_tensor(g) and g.numel():
                g = (g if g.dtype == torch.int32 else (g != 0).int()).to(dev).contiguous()
                if g.dim() != 2 or g.shape[1] != N:
                    raise ValueError(f"instance_boxes: masks {tuple(g.shape)} against {N} points")
                n, gptr = g.shape[0], g.data_ptr()
            else:
                n, gptr = 0, 0  # no masks: every pick is an empty group
            p, pptr = pk.shape[0], pk.data_ptr() if pk.shape[0] else 0
        elif form == "ids":
            g = torch.as_tensor(g, device=dev).to(torch.int32).reshape(-1).contiguous()
            if g.shape[0] != N:
                raise ValueError(f"id_boxes: group [{g.shape[0]}] against {N} points")
            n, p, gptr, pptr = 0, int(pk), g.data_ptr() if N else 0, 0
        else:
            raise ValueError(f"boxes: form must be 'rows' or 'ids', got {form!r}")
        keep += [g, pk, x]
        forms.append(form), Ns.append(N), ns.append(n), ps.append(p), gp.append(gptr), pp.append(pptr)
        xp.append(x.data_ptr() if N else 0)
    table, sizes = box_scene_table(forms, Ns, ns, ps, gp, pp, xp)
    out = pointops.instance_boxes_batched(pointops._table_dev(table, dev), sizes, _box_angles_dev(int(angles), dev))
    del keep  # (alive until the launches were queued on the current stream)
    return (table, *out)


def _split_boxes(table, count, rows, A):
    out = []
    for t in scene_rows(table, BOX_SCENE_ROW):
        p, o = int(t["p"]), int(t["row_off"])
        out.append(_boxes_from_rows(rows[o:o + p], count[o:o + p], A))
    return out


def _boxes_batched(specs, oriented, angles):
    A = int(angles) if oriented else 1
    box_angle_table(angles)
    table, count, aligned, orient = _boxes_packed(specs, A)
    return _split_boxes(table, count, orient if oriented else aligned, A)


def instance_boxes_batched(masks, picks, xyzs, *, oriented=False, angles=BOX_ANGLES):
    """instance_boxes of several scenes at once on the GPU: lists with one entry per scene ([] for the masks of a scene
    without proposals).  One table upload and one gf_instance_boxes_batched call for the whole batch; returns one Boxes
    per scene, on the device (views of the batch's buffers)."""
    if not len(masks) == len(picks) == len(xyzs):
        raise ValueError("instance_boxes_batched: one entry per scene in every list")
    return _boxes_batched([("rows", m, p, x) for m, p, x in zip(masks, picks, xyzs)], oriented, angles)


def id_boxes_batched(groups, n_groups, xyzs, *, oriented=False, angles=BOX_ANGLES):
    """id_boxes of several scenes at once on the GPU; lists with one entry per scene."""
    if not len(groups) == len(n_groups) == len(xyzs):
        raise ValueError("id_boxes_batched: one entry per scene in every list")
    return _boxes_batched([("ids", g, p, x) for g, p, x in zip(groups, n_groups, xyzs)], oriented, angles)


def instance_boxes(masks, pick, xyz, *, oriented=False, angles=BOX_ANGLES):
    """The 3D box of every picked mask of one scene: masks [n, N] (nonzero = member; they may overlap), pick [p] rows of
    masks (one outside [0, n) is an empty group), xyz [N, 3].  oriented=False: the axis-aligned box.  oriented=True: the
    upright box of least footprint among `angles` equal headings over [0, 90 degrees) (the lowest heading among equals).
    CUDA tensors take the kernels (csrc/boxes.hip) and the Boxes stays on the device; numpy arrays / CPU tensors take the
    statement instance_boxes_host, which the kernels match bit for bit."""
    if torch.is_tensor(xyz) and xyz.is_cuda:
        return instance_boxes_batched([masks], [pick], [xyz], oriented=oriented, angles=angles)[0]
    box_angle_table(angles)
    A = int(angles) if oriented else 1
    count, aligned, orient = instance_boxes_host(masks, pick, xyz, A)
    return _boxes_from_rows(orient if oriented else aligned, count, A)


def id_boxes(group, n_groups, xyz, *, oriented=False, angles=BOX_ANGLES):
    """The 3D box of every group of a per-point map: group int [N] with values in [-1, n_groups), -1 = no group (ground
    truth instances, label maps' owner).  Otherwise as instance_boxes."""
    if torch.is_tensor(xyz) and xyz.is_cuda:
        return id_boxes_batched([group], [n_groups], [xyz], oriented=oriented, angles=angles)[0]
    box_angle_table(angles)
    A = int(angles) if oriented else 1
    count, aligned, orient = id_boxes_host(group, n_groups, xyz, A)
    return _boxes_from_rows(orient if oriented else aligned, count, A)


def _overlap_1d(d, ha, hb):
    o = np.minimum(ha, d + hb) - np.maximum(-ha, d - hb)
    return np.where(o > 0.0, o, 0.0)


def _clip_host(pu, pv, m, axis, sign, h):
    """One pass of Sutherland-Hodgman over K polygons at once (pu, pv float64 [K, 8], m [K] vertices each) against
    sign * w >= -h, w the first (axis 0) or second coordinate: box_clip of csrc/boxes.hip, operation for operation."""
    K = pu.shape[0]
    rows = np.arange(K)
    k = -h if sign > 0 else h
    qu, qv, out = np.zeros_like(pu), np.zeros_like(pv), np.zeros(K, np.int64)
    pw, po = (pv, pu) if axis else (pu, pv)
    for i in range(8):
        act = i < m
        j = np.maximum(m - 1, 0) if i == 0 else np.full(K, i - 1)
        cw, co, lw, lo = pw[:, i], po[:, i], pw[rows, j], po[rows, j]
        cin, lin = (cw >= k, lw >= k) if sign > 0 else (cw <= k, lw <= k)
        with np.errstate(all="ignore"):
            tt = (k - lw) / (cw - lw)
            io = lo + tt * (co - lo)
        put = act & (cin != lin) & (out < 8)
        qu[rows[put], out[put]] = (io if axis else k)[put]
        qv[rows[put], out[put]] = (k if axis else io)[put]
        out[put] += 1
        put = act & cin & (out < 8)
        qu[rows[put], out[put]] = pu[put, i]
        qv[rows[put], out[put]] = pv[put, i]
        out[put] += 1
    return qu, qv, out


def box_iou_host(a, b):
    """float64 [P, G]: the 3D IoU of every box of a (Boxes or rows [P, BOX_FLOATS]) with every box of b -- the statement
    of gf_box_iou_batched (include/geoformer_hip.h gives the rules), numpy float64 ufuncs in the kernel's order."""
    A = np.asarray(_np(_box_rows_of(a)), dtype=np.float64).reshape(-1, BOX_FLOATS)
    B = np.asarray(_np(_box_rows_of(b)), dtype=np.float64).reshape(-1, BOX_FLOATS)
    P, G, k = A.shape[0], B.shape[0], _BOX
    if P == 0 or G == 0:
        return np.zeros((P, G))
    A, B = np.repeat(A, G, axis=0), np.tile(B, (P, 1))  # one row per pair
    hau, hav, haz = A[:, k.du] * 0.5, A[:, k.dv] * 0.5, A[:, k.dz] * 0.5
    hbu, hbv, hbz = B[:, k.du] * 0.5, B[:, k.dv] * 0.5, B[:, k.dz] * 0.5
    volA, volB = (A[:, k.du] * A[:, k.dv]) * A[:, k.dz], (B[:, k.du] * B[:, k.dv]) * B[:, k.dz]
    oz = _overlap_1d(B[:, k.cz] - A[:, k.cz], haz, hbz)
    area = _overlap_1d(B[:, k.cx] - A[:, k.cx], hau, hbu) * _overlap_1d(B[:, k.cy] - A[:, k.cy], hav, hbv)
    poly = np.nonzero((A[:, k.s] != 0.0) | (B[:, k.s] != 0.0))[0]
    if poly.shape[0]:
        a_, b_ = A[poly], B[poly]
        ca, sa, cb, sb = a_[:, k.c], a_[:, k.s], b_[:, k.c], b_[:, k.s]
        dx, dy = a_[:, k.cx] - b_[:, k.cx], a_[:, k.cy] - b_[:, k.cy]
        cu, cv = dx * cb + dy * sb, dy * cb - dx * sb
        cr, sr = ca * cb + sa * sb, sa * cb - ca * sb
        ux, uy, vx, vy = hau[poly] * cr, hau[poly] * sr, hav[poly] * sr, hav[poly] * cr
        K = poly.shape[0]
        pu, pv = np.zeros((K, 8)), np.zeros((K, 8))
        pu[:, 0], pv[:, 0] = (cu - ux) + vx, (cv - uy) - vy
        pu[:, 1], pv[:, 1] = (cu + ux) + vx, (cv + uy) - vy
        pu[:, 2], pv[:, 2] = (cu + ux) - vx, (cv + uy) + vy
        pu[:, 3], pv[:, 3] = (cu - ux) - vx, (cv - uy) + vy
        m = np.full(K, 4, np.int64)
        for axis, sign, h in ((0, 1, hbu[poly]), (0, -1, hbu[poly]), (1, 1, hbv[poly]), (1, -1, hbv[poly])):
            pu, pv, m = _clip_host(pu, pv, m, axis, sign, h)
        rows, acc = np.arange(K), np.zeros(K)
        for i in range(8):
            j = np.where(i + 1 == m, 0, min(i + 1, 7))
            term = pu[:, i] * pv[rows, j] - pu[rows, j] * pv[:, i]
            acc = np.where(i < m, acc + term, acc)
        area[poly] = np.where(m >= 3, np.abs(acc) * 0.5, 0.0)
    inter = np.where((volA > 0.0) & (volB > 0.0), area * oz, 0.0)
    den = (volA + volB) - inter
    with np.errstate(all="ignore"):
        return np.where(den > 0.0, inter / den, 0.0).reshape(P, G)


def box_iou_batched(a_list, b_list):
    """box_iou of several scenes in one launch on the GPU: a_list[b] (Boxes or rows) against b_list[b]; returns one
    float64 [P_b, G_b] tensor per scene, views of one packed buffer."""
    from . import pointops

    if len(a_list) != len(b_list):
        raise ValueError("box_iou_batched: one entry per scene in both lists")
    ra, rb = [_box_rows_of(a) for a in a_list], [_box_rows_of(b) for b in b_list]
    dev = next((r.device for r in ra + rb if torch.is_tensor(r)), None)
    if dev is None or dev.type != "cuda":
        raise RuntimeError("box_iou_batched: the kernel runs on the GPU; box_iou_host has the numpy path")
    rows = lambda r: torch.as_tensor(r, device=dev).to(torch.float64).reshape(-1, BOX_FLOATS)  # noqa: E731
    ra, rb = [rows(r) for r in ra], [rows(r) for r in rb]
    table, sizes = box_iou_table([r.shape[0] for r in ra], [r.shape[0] for r in rb])
    cat = lambda rs: (rs[0] if len(rs) == 1 else torch.cat(rs)).contiguous() if rs else torch.zeros((0, BOX_FLOATS), dtype=torch.float64, device=dev)  # noqa: E731
    out = pointops.box_iou_batched(pointops._table_dev(table, dev), sizes, cat(ra), cat(rb))
    return [out[o:o + P * G].view(P, G) for P, G, o in scene_rows(table, BOX_IOU_ROW)[["P", "G", "out_off"]].tolist()]


def box_iou(a, b):
    """float64 [P, G]: the 3D IoU of every box of a with every box of b (Boxes, or packed rows [., BOX_FLOATS]): upright
    boxes, exact rectangle clipping in float64.  CUDA tensors take gf_box_iou_batched and the result stays on the
    device; numpy arrays take box_iou_host, which the kernel matches bit for bit."""
    ra, rb = _box_rows_of(a), _box_rows_of(b)
    if any(torch.is_tensor(r) and r.is_cuda for r in (ra, rb)):
        return box_iou_batched([ra], [rb])[0]
    return box_iou_host(ra, rb)
