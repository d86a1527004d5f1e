"""Thin wrappers of csrc/view_merge.hip: the five launches that join the instances of a scan's views and the mean of
the views' semantic scores (the statements are postprocess.merge_views_host and mean_views_host; postprocess.merge_views
and mean_views are the callers).  Every wrapper checks dtype, contiguity, device, shapes and the caps and raises
RuntimeError before anything is launched.

A module of its own, not a section of pointops: pointops is imported by every forward, and what it defines is paid by
processes that never join views (DESIGN.md section 19 on what a process that never stitches pays)."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream_ptr
from .pointops import TILE_SCENE_FIELDS, TILE_SCORE_FIELDS, TILE_STITCH_MAX_CLASSES, _f32c, _i32c
from .postprocess import VIEW_MAX_VIEWS  # gf_view_merge_max_views(): asserted against the library in view_limits()

VIEW_MAX_ROWS = 4096  # gf_view_merge_max_rows(): asserted against the library in view_limits()
VIEW_MAX_POINTS = (1 << 31) - 2


def view_limits():
    """(most rows in all, most views) of the view merge, from the library."""
    lib = _lib.load()
    lim = lib.gf_view_merge_max_rows(), lib.gf_view_merge_max_views()
    if lim != (VIEW_MAX_ROWS, VIEW_MAX_VIEWS):
        raise RuntimeError(f"view merge: the library's limits {lim} are not {(VIEW_MAX_ROWS, VIEW_MAX_VIEWS)}")
    return lim


def view_check_caps(table_host, N=None):
    """The caps of the view merge on a host view table (postprocess.view_scene_table), before any launch: P."""
    t = np.asarray(table_host)
    if t.ndim != 2 or t.shape[1] != TILE_SCENE_FIELDS or t.dtype != np.int64:
        raise RuntimeError(f"view table: expected int64 [V, {TILE_SCENE_FIELDS}], got {t.dtype} {t.shape}")
    from . import postprocess

    if not 1 <= t.shape[0] <= VIEW_MAX_VIEWS:
        raise RuntimeError(f"view merge: {t.shape[0]} views (1 to {VIEW_MAX_VIEWS})")
    P = int(postprocess.scene_rows(t, postprocess.TILE_ROW)["p_s"].sum())
    if P > VIEW_MAX_ROWS:
        raise RuntimeError(f"view merge: {P} picked rows over {t.shape[0]} views (at most {VIEW_MAX_ROWS})")
    if N is not None and not 0 <= N <= VIEW_MAX_POINTS:
        raise RuntimeError(f"view merge: N = {N} points (at most {VIEW_MAX_POINTS})")
    return P


def _view_sizes(P, V, name):
    if not 0 <= P <= VIEW_MAX_ROWS:
        raise RuntimeError(f"{name}: {P} rows (at most {VIEW_MAX_ROWS})")
    if not 1 <= V <= VIEW_MAX_VIEWS:
        raise RuntimeError(f"{name}: {V} views (1 to {VIEW_MAX_VIEWS})")


def view_pack(table, table_host, N):
    """(bits int32 [P, ceil(N / 32)], cnt int32 [P]): every picked row of every view as a bitset over the scan's N points
    and its number of points (gf_view_pack; table / table_host: postprocess.view_scene_table on the device and on the
    host).  One memset and one launch on the current stream."""
    N = int(N)
    P = view_check_caps(table_host, N)
    table_host = np.ascontiguousarray(table_host)
    if not (table.is_cuda and table.dtype == torch.int64 and table.is_contiguous()
            and tuple(table.shape) == table_host.shape):
        raise RuntimeError(f"view_pack: table: expected a contiguous int64 tensor {table_host.shape} on the GPU")
    bits = torch.empty((P, (N + 31) // 32), dtype=torch.int32, device=table.device)
    cnt = torch.empty(P, dtype=torch.int32, device=table.device)
    check(_lib.load().gf_view_pack(ptr(table), table_host.ctypes.data, table_host.shape[0], P, N, ptr(bits), ptr(cnt),
                                   stream_ptr()), "gf_view_pack")
    return bits, cnt


def view_overlaps(bits, N, out=None):
    """inter int32 [P, P]: the points two rows share, from view_pack's bitsets (gf_view_overlaps: one launch, every cell
    written).  out: an int32 [P, P] tensor to write into."""
    _i32c(bits, "bits")
    P, N = bits.shape[0], int(N)
    _view_sizes(P, 1, "view_overlaps")
    if bits.dim() != 2 or bits.shape[1] != (N + 31) // 32 or not 0 <= N <= VIEW_MAX_POINTS:
        raise RuntimeError(f"view_overlaps: expected bits [P, {(N + 31) // 32}] for N = {N}, got {tuple(bits.shape)}")
    inter = torch.empty((P, P), dtype=torch.int32, device=bits.device) if out is None else _i32c(out, "out")
    if inter.shape != (P, P):
        raise RuntimeError(f"view_overlaps: out: expected [{P}, {P}], got {tuple(inter.shape)}")
    check(_lib.load().gf_view_overlaps(ptr(bits), P, N, ptr(inter), stream_ptr()), "gf_view_overlaps")
    return inter


def view_best(inter, cnt, cls, row_view, view_first):
    """best int32 [P, V]: every row's partner of the largest IoU in every other view, exact, the smaller row on ties, -1
    without one (gf_view_best, one launch).  cls int64 [P], row_view int32 [P], view_first int32 [V + 1]."""
    _i32c(inter, "inter"); _i32c(cnt, "cnt"); _i32c(row_view, "row_view"); _i32c(view_first, "view_first")
    P, V = cnt.shape[0], view_first.shape[0] - 1
    _view_sizes(P, V, "view_best")
    if not (cls.is_cuda and cls.dtype == torch.int64 and cls.is_contiguous()):
        raise RuntimeError("view_best: cls: expected a contiguous int64 tensor on the GPU")
    if inter.shape != (P, P) or cls.shape != (P,) or row_view.shape != (P,):
        raise RuntimeError(f"view_best: expected inter [{P}, {P}], cls [{P}] and row_view [{P}], got "
                           f"{tuple(inter.shape)}, {tuple(cls.shape)}, {tuple(row_view.shape)}")
    best = torch.empty((P, V), dtype=torch.int32, device=inter.device)
    check(_lib.load().gf_view_best(ptr(inter), ptr(cnt), ptr(cls), ptr(row_view), ptr(view_first), P, V, ptr(best),
                                   stream_ptr()), "gf_view_best")
    return best


def view_merge(inter, cnt, best, cls, scores, row_view, iou, min_views):
    """dict of comp int32 [P], members int32 [P] (global id or -1), G int32 [1], cls int64 [P], scores fp32 [P],
    support int32 [P] (the first G of the last three are the instances'), first int32 [P + 1] and rows int32 [P] (the
    member lists): the components of postprocess.merge_views_host's mutual-best edges, one launch of one workgroup
    (gf_view_merge)."""
    _i32c(inter, "inter"); _i32c(cnt, "cnt"); _i32c(best, "best"); _f32c(scores, "scores"); _i32c(row_view, "row_view")
    P, V = scores.shape[0], best.shape[1] if best.dim() == 2 else 0
    _view_sizes(P, V, "view_merge")
    if not (cls.is_cuda and cls.dtype == torch.int64 and cls.is_contiguous()):
        raise RuntimeError("view_merge: cls: expected a contiguous int64 tensor on the GPU")
    if inter.shape != (P, P) or cnt.shape != (P,) or best.shape != (P, V) or cls.shape != (P,) or row_view.shape != (P,):
        raise RuntimeError(f"view_merge: expected inter [{P}, {P}], cnt [{P}], best [{P}, V], cls [{P}] and row_view "
                           f"[{P}], got {tuple(inter.shape)}, {tuple(cnt.shape)}, {tuple(best.shape)}, "
                           f"{tuple(cls.shape)}, {tuple(row_view.shape)}")
    if not 1 <= int(min_views) <= V:
        raise RuntimeError(f"view_merge: min_views = {min_views} (1 to V = {V})")
    dev = scores.device
    ints = torch.empty((5, P + 1), dtype=torch.int32, device=dev)
    d_G = torch.empty(1, dtype=torch.int32, device=dev)
    inst_cls = torch.empty(max(P, 1), dtype=torch.int64, device=dev)
    inst_scores = torch.empty(max(P, 1), dtype=torch.float32, device=dev)
    check(_lib.load().gf_view_merge(ptr(inter), ptr(cnt), ptr(best), ptr(cls), ptr(scores), ptr(row_view), P, V,
                                    float(iou), int(min_views), ptr(ints[0]), ptr(ints[1]), ptr(d_G), ptr(inst_cls),
                                    ptr(inst_scores), ptr(ints[2]), ptr(ints[3]), ptr(ints[4]), stream_ptr()),
          "gf_view_merge")
    return dict(comp=ints[0, :P], members=ints[1, :P], G=d_G, cls=inst_cls[:P], scores=inst_scores[:P],
                support=ints[2, :P], first=ints[3], rows=ints[4, :P])


def view_assemble(bits, merged, row_view, G, N, vote, out=None):
    """(masks int32 [G, N], count int32 [G]): every instance's per-point vote over its member rows (gf_view_assemble: one
    memset of count and one launch on the current stream; every cell of masks is written).  merged: view_merge's dict;
    out: an int32 [G, N] tensor to write into."""
    _i32c(bits, "bits"); _i32c(row_view, "row_view")
    P, N, G = bits.shape[0], int(N), int(G)
    _view_sizes(P, 1, "view_assemble")
    if bits.dim() != 2 or bits.shape[1] != (N + 31) // 32 or not 0 <= N <= VIEW_MAX_POINTS or not 0 <= G <= P:
        raise RuntimeError(f"view_assemble: expected bits [P, {(N + 31) // 32}] for N = {N} and 0 <= G <= P, got "
                           f"{tuple(bits.shape)}, G = {G}")
    if not 0.0 < float(vote) <= 1.0:
        raise RuntimeError(f"view_assemble: vote = {vote} (in (0, 1])")
    if row_view.shape != (P,) or merged["rows"].shape != (P,) or merged["first"].shape != (P + 1,):
        raise RuntimeError(f"view_assemble: expected row_view [{P}] and view_merge's lists of {P} rows")
    masks = torch.empty((G, N), dtype=torch.int32, device=bits.device) if out is None else _i32c(out, "out")
    if masks.shape != (G, N):
        raise RuntimeError(f"view_assemble: out: expected [{G}, {N}], got {tuple(masks.shape)}")
    count = torch.empty(G, dtype=torch.int32, device=bits.device)
    check(_lib.load().gf_view_assemble(ptr(bits), ptr(merged["first"]), ptr(merged["rows"]), ptr(row_view),
                                       ptr(merged["support"]), P, G, N, float(vote), ptr(masks), ptr(count),
                                       stream_ptr()), "gf_view_assemble")
    return masks, count


def view_mean_scores(table, table_host, N, C, out=None):
    """out fp32 [N, C]: the mean of the V views' scores, summed in view order and divided by V (gf_view_mean_scores, the
    statement is postprocess.mean_views_host): one launch on the current stream, no atomics, nothing read back.  table /
    table_host: int64 [V, GF_TILE_SCORE_FIELDS] (postprocess.tile_score_table of the views' tensors) on the device and
    on the host.  V or C above the caps raise before anything is launched."""
    t = np.asarray(table_host)
    if t.ndim != 2 or t.shape[1] != TILE_SCORE_FIELDS or t.dtype != np.int64:
        raise RuntimeError(f"view_mean_scores: table_host: expected int64 [V, {TILE_SCORE_FIELDS}], got {t.dtype} {t.shape}")
    table_host = np.ascontiguousarray(t)
    N, C = int(N), int(C)
    _view_sizes(0, table_host.shape[0], "view_mean_scores")
    if not 1 <= C <= TILE_STITCH_MAX_CLASSES:
        raise RuntimeError(f"view_mean_scores: C = {C} classes (1 to {TILE_STITCH_MAX_CLASSES})")
    if not 0 <= N <= VIEW_MAX_POINTS:
        raise RuntimeError(f"view_mean_scores: N = {N} points (at most {VIEW_MAX_POINTS})")
    if not (table.is_cuda and table.dtype == torch.int64 and table.is_contiguous()
            and tuple(table.shape) == table_host.shape):
        raise RuntimeError(f"view_mean_scores: table: expected a contiguous int64 tensor {table_host.shape} on the GPU")
    res = torch.empty((N, C), dtype=torch.float32, device=table.device) if out is None else _f32c(out, "out")
    if res.shape != (N, C):
        raise RuntimeError(f"view_mean_scores: out: expected [{N}, {C}], got {tuple(res.shape)}")
    check(_lib.load().gf_view_mean_scores(ptr(table), table_host.ctypes.data, table_host.shape[0], N, C, ptr(res),
                                          stream_ptr()), "gf_view_mean_scores")
    return res
