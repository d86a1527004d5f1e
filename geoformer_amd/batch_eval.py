"""Evaluation of the val set several scenes per forward (test.py:40-150 with batches of B scenes instead of one).

    for name, cls, scores, masks, pick in predict_batches(model, [(name, raw), ...], batch_size=4):
        ...                                   # masks int32 [n, N] over the scene's points, pick: the NMS result
    ap, avgs = evaluate(model, [(name, raw), ...], batch_size=4)
    print(evaluation.format_results(avgs))
    ev = evaluation.SemanticEvaluator(train_fold=model.cfg.train_fold)
    ap, avgs = evaluate(model, [(name, raw), ...], batch_size=4, semantic=ev)    # AP and mIoU from one pass
    res = evaluate_semantic(model, [(name, raw), ...], batch_size=4)             # backbone + semantic head only
    print(evaluation.format_semantic_results(res))
    res = evaluate_boxes(model, [(name, raw), ...], batch_size=4, kind="oriented")   # box mAP@0.25 / mAP@0.5
    print(evaluation.format_box_results(res))
    for name, labels in label_batches(model, [(name, raw), ...], batch_size=4):
        ...                                   # labels.ids / .owner [N], labels.table: one row per instance (host)
    for name, labels, pan in panoptic_batches(model, [(name, raw), ...], batch_size=4):
        ...                                   # pan [N]: instance ids, 1000 wall, 2000 floor, 0 unlabelled (host)
    res = evaluate_panoptic(model, [(name, raw), ...], batch_size=4)             # PQ / SQ / RQ
    print(evaluation.format_panoptic_results(res))
    for name, cls, scores, masks, pick in predict_batches(model, [(name, raw), ...], batch_size=4, tiles=Tiling(tile=4.0)):
        ...                                   # a large scan runs as overlapping tiles; masks int32 [G, N], merged
    ap, avgs = evaluate(model, [(name, raw), ...], batch_size=4, tiles=Tiling(tile=4.0), stitch="core", semantic=ev)
    res = evaluate_panoptic(model, [(name, raw), ...], batch_size=4, tiles=Tiling(tile=4.0), stitch="core")
                                              # the tiles' semantic scores stitched per scan: "core" or "mean"
    for name, cls, scores, masks, pick in predict_batches(model, [(name, raw), ...], batch_size=4, density=Density()):
        ...                                   # a dense scan runs on one point per 2 cm cell; masks still int32 [n, N]
    for name, cls, scores, masks, pick in predict_batches(model, [(name, raw), ...], batch_size=4, views=Views(rotations=4)):
        ...                                   # every scene under 4 rotations; masks int32 [G, N]: the views' instances
                                              # paired by mutual best IoU, masks by per-point vote, scores the views' mean
    ap, avgs = evaluate(model, [(name, raw), ...], batch_size=4, views=Views(rotations=8), semantic=ev)
                                              # ... and mIoU from the mean of the views' semantic scores

A batch of raw scenes ([N, 8] = xyz, rgb, semantic label, instance label, as prepare_data_inst.py stores them) is
collated on the host (scene.collate_raw), uploaded and voxelised on the GPU one batch ahead (feeder.DeviceFeeder), and
run through ONE eval forward with ``all_scenes=True``: every scene of the batch gets its proposals (the reference's
forward keeps scene 0's only).  Matrix NMS of all scenes of the batch is one postprocess.matrix_nms_batched call, on the
benchmark label ids of test.py:65-68 with final_score_thresh 0.5 (test.py:88-93).  ``nms="greedy"`` takes the reference's
other post-process instead (test.py:78-86): class-agnostic greedy NMS at ``cfg.TEST_NMS_THRESH``, one
postprocess.greedy_nms_batched call per batch.  A scene without proposals is left out of the evaluation, as test.py's
``continue`` does.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from . import evaluation, postprocess, scene
from .feeder import DeviceFeeder

NMS_FINAL_SCORE = 0.5  # test.py:92


def scene_dict(raw):
    """scene.collate_raw's per-scene dict of a raw [N, 8] scene."""
    r = raw.detach().cpu().numpy() if torch.is_tensor(raw) else np.asarray(raw)
    return {"xyz": r[:, :3].astype(np.float32), "rgb": r[:, 3:6].astype(np.float32),
            "label": r[:, 6].astype(np.int64), "instance": r[:, 7].astype(np.int64)}


class GeometricSegments:
    """``segments=GeometricSegments(radius=0.06)`` (or ``segments="geometric"`` for the defaults): the over-segments are
    not looked up by scene name but computed from each scene's points (pointops.oversegment; keywords k, radius,
    normal_deg, offset, flatness, min_points as postprocess.oversegment_host).  predict_batches computes them on the
    device, per scene of the batch, from the batch's ``locs_float``; collate_batches on host batches computes them on the
    host."""

    def __init__(self, **params):
        unknown = sorted(set(params) - set(postprocess.OVERSEGMENT_DEFAULTS))
        if unknown:
            raise TypeError(f"GeometricSegments: unknown parameter(s) {', '.join(unknown)}; known: "
                            f"{', '.join(postprocess.OVERSEGMENT_DEFAULTS)}")
        self.params = dict(postprocess.OVERSEGMENT_DEFAULTS, **params)

    def __repr__(self):
        return f"GeometricSegments({', '.join(f'{k}={v!r}' for k, v in self.params.items())})"

    def of_batch(self, locs_float, offsets_host):
        """int32 [N] ids of a batch's points: one pointops.oversegment per scene (scene-local ids), on locs_float's device
        and the current stream."""
        from . import pointops

        off = [int(o) for o in offsets_host]
        parts = [pointops.oversegment(locs_float[off[b]:off[b + 1]].contiguous(), **self.params)
                 for b in range(len(off) - 1)]
        return torch.cat(parts) if parts else torch.empty(0, dtype=torch.int32, device=locs_float.device)


def _geometric(segments):
    """The GeometricSegments `segments` stands for, or None where it is a mapping (or None)."""
    if isinstance(segments, str):
        if segments != "geometric":
            raise ValueError(f"segments: a mapping scene name -> ids, a GeometricSegments or 'geometric', got "
                             f"{segments!r}")
        return GeometricSegments()
    return segments if isinstance(segments, GeometricSegments) else None


class MaskSplit:
    """``split=MaskSplit(radius=0.08, min_points=100, mode="split")`` (or ``split="largest"`` / ``split="split"`` for the
    defaults of that mode): every scene's picked masks are split into spatially connected clusters after the NMS
    (postprocess.split_masks; keywords radius, k, min_samples, min_points, mode)."""

    def __init__(self, **params):
        unknown = sorted(set(params) - set(postprocess.SPLIT_DEFAULTS))
        if unknown:
            raise TypeError(f"MaskSplit: unknown parameter(s) {', '.join(unknown)}; known: "
                            f"{', '.join(postprocess.SPLIT_DEFAULTS)}")
        self.params = dict(postprocess.SPLIT_DEFAULTS, **params)
        if self.params["mode"] not in postprocess.SPLIT_MODES:
            raise ValueError(f"MaskSplit: mode must be one of {postprocess.SPLIT_MODES}, got {self.params['mode']!r}")

    def __repr__(self):
        return f"MaskSplit({', '.join(f'{k}={v!r}' for k, v in self.params.items())})"

    def of_scene(self, cls, scores, masks, pick, xyz):
        """(cls', scores', masks', pick') of one scene: postprocess.split_masks on the tensors' device and the current
        stream."""
        return postprocess.split_masks(masks, scores, cls, pick, xyz, **self.params)


def _mask_split(split):
    """The MaskSplit `split` stands for, or None."""
    if split is None or isinstance(split, MaskSplit):
        return split
    if isinstance(split, str) and split in postprocess.SPLIT_MODES:
        return MaskSplit(mode=split)
    raise ValueError(f"split: None, a MaskSplit or one of {postprocess.SPLIT_MODES}, got {split!r}")


class Tiling:
    """``tiles=Tiling(tile=4.0, halo=0.5, max_points=400_000, iom=0.5, min_shared=20)``: every scene with more than
    max_points points is run as the overlapping tiles of scene.tile_plan(xyz, tile, halo), and the picked instances of
    its tiles are joined by postprocess.merge_tiles(iom, min_shared).  max_points is a starting point with no
    measurement behind it."""

    DEFAULTS = dict(tile=4.0, halo=0.5, max_points=400_000, **postprocess.TILE_DEFAULTS)

    def __init__(self, **params):
        unknown = sorted(set(params) - set(self.DEFAULTS))
        if unknown:
            raise TypeError(f"Tiling: unknown parameter(s) {', '.join(unknown)}; known: {', '.join(self.DEFAULTS)}")
        self.params = dict(self.DEFAULTS, **params)
        if not self.params["tile"] > 0 or not self.params["halo"] >= 0 or self.params["max_points"] < 0:
            raise ValueError(f"Tiling: tile > 0, halo >= 0 and max_points >= 0, got {self!r}")

    def __repr__(self):
        return f"Tiling({', '.join(f'{k}={v!r}' for k, v in self.params.items())})"

    def plan_of(self, raw):
        """The scene.TilePlan of a raw [N, 8] scene, or None when it has at most max_points points."""
        r = raw.detach().cpu().numpy() if torch.is_tensor(raw) else np.asarray(raw)
        if r.shape[0] <= self.params["max_points"]:
            return None
        return scene.tile_plan(r[:, :3], self.params["tile"], self.params["halo"])

    def merge(self, plan, per_tile):
        """(cls, scores, masks [G, N], pick) of a scan from its tiles' results (postprocess.merge_tiles); a scan none
        of whose tiles picked anything is a scene without proposals."""
        cls, scores, masks, pick, _ = postprocess.merge_tiles(plan, per_tile, iom=self.params["iom"],
                                                              min_shared=self.params["min_shared"])
        if len(pick) == 0:
            return [], [], [], pick
        return cls, scores, masks, pick


class TileName(tuple):
    """(scene name, tile id): the name of a tile in tile_items' expanded list."""
    __slots__ = ()

    def __new__(cls, name, tile):
        return super().__new__(cls, (name, int(tile)))


def tile_items(items, tiling):
    """(expanded items, plans): every (name, raw) whose scene has more than tiling's max_points points is replaced, in
    place, by its non-empty tiles (TileName(name, tile id), the raw rows gathered through plan.index); plans: scene
    name -> scene.TilePlan of the tiled scenes.  The other scenes pass through."""
    out, plans = [], {}
    for name, raw in items:
        plan = tiling.plan_of(raw)
        if plan is None:
            out.append((name, raw))
            continue
        if name in plans:
            raise ValueError(f"tile_items: two scenes are named {name!r}")
        plans[name] = plan
        r = raw.detach().cpu().numpy() if torch.is_tensor(raw) else np.asarray(raw)
        out.extend((TileName(name, s), r[plan.points(s)]) for s in range(plan.T) if plan.offsets[s + 1] > plan.offsets[s])
    return out, plans


def _tiling(tiles):
    if tiles is None or isinstance(tiles, Tiling):
        return tiles
    raise ValueError(f"tiles: None or a Tiling, got {tiles!r}")


def _stitching(stitch, tiling, who):
    """The checks of the stitch= keyword, before anything touches the model or the GPU."""
    if stitch is not None and stitch not in postprocess.STITCH_MODES:
        raise ValueError(f"{who}: stitch must be None or one of {postprocess.STITCH_MODES}, got {stitch!r}")
    if stitch is not None and tiling is None:
        raise ValueError(f"{who}: stitch= goes with tiles=")
    return stitch


def _tiled_raws(items, plans):
    """{name: raw} of the tiled scenes, whose kept scores and labels go by name: a tiled scene that shares its name with
    another scene of the list would be counted against the wrong labels, so that is a ValueError."""
    names = [n for n, _ in items]
    twice = sorted({str(n) for n in plans if names.count(n) > 1})
    if twice:
        raise ValueError(f"stitch=: the tiled scene(s) {', '.join(twice)} share their name with another scene")
    return {n: r for n, r in items if n in plans}


class _TileSemantics:
    """Stands where predict_batches / semantic_batches take a SemanticEvaluator when scans run as tiles: a scene that is
    no tile of a planned scan is handed on to `inner` at once, as a batch of one scene; the scores of a scan's tiles
    are kept on the device (copies: nothing says that the next forward does not write the same buffer) until the scan's last
    non-empty tile is in, then stitched (postprocess.stitch_tiles, one launch) and handed on once, under the scan's own
    name with the scan's own labels (the raw scene's column 6).  A scan holds 4 * C * (the points of all its tiles)
    bytes until then.  Nothing is read back."""

    def __init__(self, inner, plans, raws, stitch):
        self.inner, self.plans, self.raws, self.stitch = inner, plans, raws, stitch
        self.left = {n: int((np.diff(p.offsets) > 0).sum()) for n, p in plans.items()}
        self.kept = {}

    def add_batch(self, scores, labels, offsets, names, offsets_host=None):
        off = [int(o) for o in (offsets if offsets_host is None else offsets_host)]
        for i, name in enumerate(names):
            part = scores[off[i]:off[i + 1]]
            if not (isinstance(name, TileName) and name[0] in self.plans):
                _hand_on(self.inner, part, labels[off[i]:off[i + 1]], name)
                continue
            scan, s = name
            plan = self.plans[scan]
            self.kept.setdefault(scan, [None] * plan.T)[s] = part.clone(memory_format=torch.contiguous_format)
            self.left[scan] -= 1
            if self.left[scan] == 0:
                stitched = postprocess.stitch_tiles(plan, self.kept.pop(scan), self.stitch)
                lab = torch.from_numpy(scene_dict(self.raws[scan])["label"]).to(scores.device, non_blocking=True)
                _hand_on(self.inner, stitched, lab, scan)


def _predict_tiled(model, raw_scenes, batch_size, tiling, stitch, kw):
    """The loop of predict_batches over tile_items' expanded list; a tiled scene is yielded once, merged, when its last
    tile has come out.  With stitch the semantic evaluator is given every tiled scene once too, stitched
    (_TileSemantics), in the batch of the scene's last tile: before that batch's NMS and before the scene is yielded."""
    if kw.get("semantic") is not None and stitch is None:
        raise ValueError('predict_batches: semantic= is not supported with tiles yet without stitch="core" or "mean"')
    raw_scenes = list(raw_scenes)
    items, plans = tile_items(raw_scenes, tiling)
    if kw.get("semantic") is not None:
        kw = dict(kw, semantic=_TileSemantics(kw["semantic"], plans, _tiled_raws(raw_scenes, plans), stitch))
    segments = kw.get("segments")
    if plans and segments is not None and _geometric(segments) is None:
        # a mapping: a tiled scene's ids are sliced through the plan, per tile
        sliced = {n: s for n, s in segments.items() if n not in plans}
        for name, _ in items:
            if isinstance(name, TileName) and name[0] in plans and segments.get(name[0]) is not None:
                seg = segments[name[0]]
                seg = seg.detach().cpu().numpy() if torch.is_tensor(seg) else np.asarray(seg)
                if seg.shape != (plans[name[0]].N,):
                    raise ValueError(f"segments[{name[0]!r}]: expected one id per point [{plans[name[0]].N}], got "
                                     f"{seg.shape}")
                sliced[name] = seg[plans[name[0]].points(name[1])]
        kw = dict(kw, segments=sliced)
    left = {n: int((np.diff(p.offsets) > 0).sum()) for n, p in plans.items()}
    got = {n: {} for n in plans}
    for name, cls, sc, masks, pick in predict_batches(model, items, batch_size, **kw):
        if not (isinstance(name, TileName) and name[0] in plans):
            yield name, cls, sc, masks, pick
            continue
        scan, s = name
        got[scan][s] = (cls, sc, masks, pick)
        left[scan] -= 1
        if left[scan] == 0:
            none = ([], [], [], torch.empty(0, dtype=torch.int64))
            per_tile = [got[scan].get(t, none) for t in range(plans[scan].T)]
            del got[scan]
            yield (scan, *tiling.merge(plans[scan], per_tile))


class Views:
    """``views=Views(rotations=4, flip=False, matrices=None, iou=0.5, min_views=None, vote=0.5)``: test-time
    augmentation -- every scene is run under V views of the same points and the views' picked instances are joined by
    postprocess.merge_views(iou, min_views, vote).  View k is the rotation about z by 360 * k / rotations degrees
    (headings that are multiples of 90 degrees have exact 0 / +-1 entries); with flip every rotation is followed by its
    x-mirrored twin (V = 2 * rotations); view 0 is always the identity.  matrices: explicit float64 [V, 3, 3] matrices
    instead (rotations and flip are then unused): each orthogonal to 1e-9, the first the identity.  1 <= V <= 32.
    min_views=None stands for (V + 1) // 2.  iou, vote and min_views are chosen by reasoning; no measurement stands
    behind them."""

    DEFAULTS = dict(rotations=4, flip=False, matrices=None, **postprocess.VIEW_DEFAULTS)

    def __init__(self, **params):
        unknown = sorted(set(params) - set(self.DEFAULTS))
        if unknown:
            raise TypeError(f"Views: unknown parameter(s) {', '.join(unknown)}; known: {', '.join(self.DEFAULTS)}")
        self.params = p = dict(self.DEFAULTS, **params)
        if p["matrices"] is not None:
            m = np.array(p["matrices"], dtype=np.float64)
            if m.ndim != 3 or m.shape[1:] != (3, 3) or not 1 <= m.shape[0] <= postprocess.VIEW_MAX_VIEWS:
                raise ValueError(f"Views: matrices: expected [V, 3, 3] with 1 <= V <= {postprocess.VIEW_MAX_VIEWS}, "
                                 f"got {m.shape}")
            if not np.all(np.isfinite(m)) or np.abs(m @ m.transpose(0, 2, 1) - np.eye(3)).max() > 1e-9:
                raise ValueError("Views: matrices: every matrix must be orthogonal (to 1e-9)")
            if not np.array_equal(m[0], np.eye(3)):
                raise ValueError("Views: matrices: the first matrix must be the identity")
        else:
            rot = p["rotations"]
            if isinstance(rot, bool) or not isinstance(rot, (int, np.integer)) or rot < 1 \
                    or rot * (2 if p["flip"] else 1) > postprocess.VIEW_MAX_VIEWS:
                raise ValueError(f"Views: rotations: an integer >= 1 with at most {postprocess.VIEW_MAX_VIEWS} views "
                                 f"in all, got {self!r}")
            quarter = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))
            ms = []
            for k in range(int(rot)):
                if (4 * k) % rot == 0:
                    c, s = quarter[(4 * k // rot) % 4]  # exact: cos(pi / 2) is not 0
                else:
                    c, s = np.cos(2 * np.pi * k / rot), np.sin(2 * np.pi * k / rot)
                ms.append([[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]])  # xyz @ m turns the points by the angle
                if p["flip"]:
                    ms.append([[-c + 0.0, s, 0.0], [s + 0.0, c, 0.0], [0.0, 0.0, 1.0]])  # ... then x -> -x
            m = np.array(ms, dtype=np.float64)
        self.matrices = m
        self.V = int(m.shape[0])
        if not (0.0 <= p["iou"] <= 1.0) or not (0.0 < p["vote"] <= 1.0):
            raise ValueError(f"Views: 0 <= iou <= 1 and 0 < vote <= 1, got {self!r}")
        mv = p["min_views"]
        if mv is not None and (isinstance(mv, bool) or not isinstance(mv, (int, np.integer)) or not 1 <= mv <= self.V):
            raise ValueError(f"Views: min_views: None or an integer in 1 .. V = {self.V}, got {mv!r}")

    def __repr__(self):
        return f"Views({', '.join(f'{k}={v!r}' for k, v in self.params.items())})"

    @property
    def min_views(self):
        return (self.V + 1) // 2 if self.params["min_views"] is None else int(self.params["min_views"])

    def of_scene(self, raw, k):
        """View k of a raw [N, 8] scene: xyz @ matrices[k] in float64, columns 3..7, the points and their order
        unchanged; view 0 is the scene itself."""
        if k == 0:
            return raw
        r = np.array(raw.detach().cpu().numpy() if torch.is_tensor(raw) else raw)
        r[:, :3] = (r[:, :3].astype(np.float64) @ self.matrices[k]).astype(r.dtype)
        return r

    def merge(self, N, per_view):
        """(cls, scores, masks [G, N], pick) of a scene from its views' results (postprocess.merge_views); a scene
        without a kept instance is a scene without proposals."""
        cls, scores, masks, pick, _ = postprocess.merge_views(per_view, N, iou=self.params["iou"],
                                                              min_views=self.min_views, vote=self.params["vote"])
        if len(pick) == 0:
            return [], [], [], torch.as_tensor(pick)
        return cls, scores, masks, pick


class ViewName(tuple):
    """(scene name, view): the name of a view in view_items' expanded list."""
    __slots__ = ()

    def __new__(cls, name, view):
        return super().__new__(cls, (name, int(view)))


def view_items(items, views):
    """The expanded items: every (name, raw) is replaced, in place, by its V views (ViewName(name, k),
    views.of_scene(raw, k)) for k = 0 .. V-1."""
    return [(ViewName(name, k), views.of_scene(raw, k)) for name, raw in items for k in range(views.V)]


def _views(views):
    if views is None or isinstance(views, Views):
        return views
    raise ValueError(f"views: None or a Views, got {views!r}")


def _viewed_names(items, who):
    """With semantic= the views' scores of a scene are kept by its name: two scenes of one name are a ValueError."""
    names = [n for n, _ in items]
    twice = sorted({str(n) for n in names if names.count(n) > 1})
    if twice:
        raise ValueError(f"{who}: views= with semantic=: the scene(s) {', '.join(twice)} share their name with another scene")


class _ViewSemantics:
    """Stands where predict_batches / semantic_batches take a SemanticEvaluator when scenes run under V views: a scene
    that is no view is handed on to `inner` at once; the [N, C] scores of a scene's views are kept on the device (copies:
    the next forward may write the same buffer) until the last view is in, then averaged (postprocess.mean_views, one
    launch) and handed on once, under the scene's own name against view 0's labels.  A scene holds 4 * C * N * V bytes
    until then.  Nothing is read back.  With tiles, _TileSemantics stands in front and this object is given every
    view's stitched scan."""

    def __init__(self, inner, V):
        self.inner, self.V = inner, V
        self.kept, self.labels = {}, {}

    def add_batch(self, scores, labels, offsets, names, offsets_host=None):
        off = [int(o) for o in (offsets if offsets_host is None else offsets_host)]
        for i, name in enumerate(names):
            part, lab = scores[off[i]:off[i + 1]], labels[off[i]:off[i + 1]]
            if not isinstance(name, ViewName):
                _hand_on(self.inner, part, lab, name)
                continue
            scan, k = name
            got = self.kept.setdefault(scan, [None] * self.V)
            got[k] = part.clone(memory_format=torch.contiguous_format)
            if k == 0:
                self.labels[scan] = lab.clone()
            if all(x is not None for x in got):
                del self.kept[scan]
                _hand_on(self.inner, postprocess.mean_views(got), self.labels.pop(scan), scan)


def _view_segments(segments, items, V):
    """The segments= mapping of view_items' expanded list: the ids of a scene, given under the scene's name, serve every
    one of its V views (the points and their order are the same in all of them).  A GeometricSegments (or None) passes
    through: the ids are then computed per view."""
    if segments is None or _geometric(segments) is not None:
        return segments
    out = dict(segments)
    out.update({ViewName(n, k): segments[n] for n, _ in items if n in segments for k in range(V)})
    return out


def _predict_views(model, raw_scenes, batch_size, views, kw):
    """The loop of predict_batches over view_items' expanded list (tiles= / stitch=, segments= and split= apply to every
    view); a scene is yielded once, joined, under its own name when its last view has come out.  predict_batches has
    checked the names (_viewed_names) before anything else ran."""
    items = list(raw_scenes)
    kw = dict(kw, segments=_view_segments(kw.get("segments"), items, views.V))
    if kw.get("semantic") is not None:
        kw["semantic"] = _ViewSemantics(kw["semantic"], views.V)
    sizes = [(name, int(np.asarray(raw).shape[0]) if not torch.is_tensor(raw) else int(raw.shape[0])) for name, raw in items]
    at, got = 0, []
    for name, cls, sc, masks, pick in predict_batches(model, view_items(items, views), batch_size, **kw):
        scan, N = sizes[at]
        if not (isinstance(name, ViewName) and name == (scan, len(got))):
            raise RuntimeError(f"predict_batches: views=: expected view {len(got)} of {scan!r}, got {name!r}")
        got.append((cls, sc, masks, pick))
        if len(got) == views.V:
            yield (scan, *views.merge(N, got))
            at, got = at + 1, []


class Density:
    """``density=Density(cell=0.02, mode="center")``: every scene is run on one representative point per occupied cell of
    a grid of `cell` metres (pointops.grid_subsample; mode "center": the point nearest the cell's centre, "first": the
    cell's first point) and every result is put back on the scene's own points.  cell=None: 1 / scale of the collate,
    0.02 m -- one representative per voxel-sized cell."""

    DEFAULTS = dict(cell=None, mode="center")

    def __init__(self, **params):
        unknown = sorted(set(params) - set(self.DEFAULTS))
        if unknown:
            raise TypeError(f"Density: unknown parameter(s) {', '.join(unknown)}; known: {', '.join(self.DEFAULTS)}")
        self.params = dict(self.DEFAULTS, **params)
        if self.params["cell"] is not None and not (self.params["cell"] > 0 and np.isfinite(self.params["cell"])):
            raise ValueError(f"Density: cell > 0 (or None), got {self!r}")
        if self.params["mode"] not in postprocess.GRID_MODES:
            raise ValueError(f"Density: mode must be one of {postprocess.GRID_MODES}, got {self.params['mode']!r}")

    def __repr__(self):
        return f"Density({', '.join(f'{k}={v!r}' for k, v in self.params.items())})"

    def cell(self, scale=50):
        """The cell in metres: the parameter, or 1 / scale of the collate."""
        return 1.0 / scale if self.params["cell"] is None else float(self.params["cell"])


class DensityMap(NamedTuple):
    """A subsampled scene's way back: rep int64 [n] (host) -- the scene's rows that were kept, in order -- and cell_of
    int32 [N] (device) -- for every point of the scene the row of the subsampled scene that stands for it."""
    rep: np.ndarray
    cell_of: torch.Tensor


def _density(density):
    if density is None or isinstance(density, Density):
        return density
    raise ValueError(f"density: None or a Density, got {density!r}")


def density_items(items, density, device):
    """(subsampled items, maps): every (name, raw) becomes (name, raw[rep]) with (rep, cell_of, _) =
    pointops.grid_subsample of its xyz on `device` (one launch sequence and one two-word read-back per scene); maps:
    scene name -> DensityMap.  A scene that keeps every point (M == N) passes through with no map.  A subsampled scene
    that shares its name with another scene of the list is a ValueError (its map goes by its name)."""
    from . import pointops

    items = list(items)
    dev = torch.device(device)
    out, maps = [], {}
    for name, raw in items:
        r = raw.detach().cpu().numpy() if torch.is_tensor(raw) else np.asarray(raw)
        xyz = torch.from_numpy(np.ascontiguousarray(r[:, :3], dtype=np.float32)).to(dev)
        rep, cell_of, _ = pointops.grid_subsample(xyz, density.cell(), density.params["mode"])
        if rep.shape[0] == r.shape[0]:
            out.append((name, raw))
            continue
        if name in maps:
            raise ValueError(f"density=: two scenes are named {name!r}")
        rep = rep.cpu().numpy().astype(np.int64)
        maps[name] = DensityMap(rep, cell_of)
        out.append((name, r[rep]))
    names = [n for n, _ in items]
    twice = sorted({str(n) for n in maps if names.count(n) > 1})
    if twice:
        raise ValueError(f"density=: the subsampled scene(s) {', '.join(twice)} share their name with another scene")
    return out, maps


def _hand_on(inner, scores, labels, name):
    """One scene to a semantic evaluator, as a batch of one."""
    off = torch.tensor([0, scores.shape[0]], dtype=torch.int32)
    return inner.add_batch(scores, labels, off.to(scores.device, non_blocking=True), [name], offsets_host=off)


class _DensitySemantics:
    """Stands where the loops take a SemanticEvaluator when scenes run subsampled: every scene is handed on to `inner` as
    a batch of one -- a subsampled scene with its scores put back on the scene's own points through cell_of (a copy of
    rows: every point takes its representative's scores) and with the scene's own labels (the raw scene's column 6), any
    other scene as it came.  With tiles, _TileSemantics stands in front and this object is given the stitched scan."""

    def __init__(self, inner, maps, raws):
        self.inner, self.maps, self.raws = inner, maps, raws

    def add_batch(self, scores, labels, offsets, names, offsets_host=None):
        off = [int(o) for o in (offsets if offsets_host is None else offsets_host)]
        for i, name in enumerate(names):
            part, lab = scores[off[i]:off[i + 1]], labels[off[i]:off[i + 1]]
            if not isinstance(name, TileName) and name in self.maps:
                part = postprocess.expand_rows(part, self.maps[name].cell_of)
                lab = torch.from_numpy(scene_dict(self.raws[name])["label"]).to(scores.device, non_blocking=True)
            _hand_on(self.inner, part.contiguous(), lab, name)


def _density_segments(segments, maps):
    """The segments= mapping of the subsampled list: a subsampled scene's ids gathered through rep."""
    if segments is None or _geometric(segments) is not None:
        return segments
    out = dict(segments)
    for name, m in maps.items():
        if segments.get(name) is not None:
            seg = segments[name]
            seg = seg.detach().cpu().numpy() if torch.is_tensor(seg) else np.asarray(seg)
            if seg.shape != (m.cell_of.shape[0],):
                raise ValueError(f"segments[{name!r}]: expected one id per point [{m.cell_of.shape[0]}], got "
                                 f"{seg.shape}")
            out[name] = seg[m.rep]
    return out


def _predict_dense(model, raw_scenes, batch_size, density, kw):
    """The loop of predict_batches over density_items' subsampled list: everything else (segments=, split=, tiles= /
    stitch=, views=) sees the subsampled scenes, and the masks of a subsampled scene are put back on its own points
    last."""
    items = list(raw_scenes)
    dev = torch.device(kw["device"]) if kw.get("device") is not None else next(model.parameters()).device
    sub, maps = density_items(items, density, dev)
    kw = dict(kw, segments=_density_segments(kw.get("segments"), maps))
    if kw.get("semantic") is not None and maps:
        kw["semantic"] = _DensitySemantics(kw["semantic"], maps, {n: r for n, r in items if n in maps})
    views = kw.pop("views", None)  # (checked by predict_batches, names included)
    inner = predict_batches(model, sub, batch_size, **kw) if views is None else \
        _predict_views(model, sub, batch_size, views, kw)
    for name, cls, sc, masks, pick in inner:
        if name in maps and torch.is_tensor(masks):
            masks = postprocess.expand_masks(masks, maps[name].cell_of)
        yield name, cls, sc, masks, pick


def _scene_segments(segments, name, n):
    """int32 [n] over-segment ids of scene `name` from the mapping (range-checked), -1 everywhere when it has none."""
    seg = segments.get(name)
    if seg is None:
        return np.full(n, -1, np.int32)
    seg = seg.detach().cpu().numpy() if torch.is_tensor(seg) else np.asarray(seg)
    if seg.shape != (n,) or not np.issubdtype(seg.dtype, np.integer):
        raise ValueError(f"segments[{name!r}]: expected an integer array [{n}], one id per point, got {seg.dtype} "
                         f"{seg.shape}")
    if n and (int(seg.max()) > np.iinfo(np.int32).max or int(seg.min()) < np.iinfo(np.int32).min):
        raise ValueError(f"segments[{name!r}]: ids must fit int32 (at most 2^31 - 1), got {int(seg.min())} .. "
                         f"{int(seg.max())}")
    return seg.astype(np.int32)


def collate_batches(raw_scenes, batch_size, spatial_shape=None, scale=50, full_scale_min=128, segments=None):
    """(chunks of (name, raw), host batch dicts): the scenes in order, batch_size per batch (the last may be short).
    spatial_shape: a lower bound on every batch's voxel grid (a scene's results depend on the grid it runs on: a
    stride-2 convolution drops the voxels at an odd extent's edge).  segments: a mapping scene name -> integer array
    [N] of over-segment ids (scene-local, negative = none); given, every batch dict carries "segments" (int32 [N] over
    the batch's points, -1 for a scene the mapping does not name) and the eval forward pools its mask logits over
    them.  A GeometricSegments (or "geometric"): the ids are computed here, on the host, from the batch's locs_float
    (predict_batches computes them on the device instead)."""
    geo = _geometric(segments)
    items = list(raw_scenes)
    if batch_size < 1:
        raise ValueError("batch_size >= 1")
    chunks = [items[i:i + batch_size] for i in range(0, len(items), batch_size)]
    batches = []
    for chunk in chunks:
        b = scene.collate_raw([scene_dict(r) for _, r in chunk], scale, full_scale_min)
        if spatial_shape is not None:
            b["spatial_shape"] = np.maximum(b["spatial_shape"], np.asarray(spatial_shape, dtype=b["spatial_shape"].dtype))
        if geo is not None:
            b["segments"] = geo.of_batch(b["locs_float"], b["offsets"])
        elif segments is not None:
            b["segments"] = torch.from_numpy(np.concatenate(
                [_scene_segments(segments, name, np.asarray(r).shape[0]) for name, r in chunk]))
        batches.append(b)
    return chunks, batches


@torch.no_grad()
def predict_batches(model, raw_scenes, batch_size, *, epoch=300, spatial_shape=None, nms_kernel="gaussian",
                    sigma=2.0, final_score_thresh=NMS_FINAL_SCORE, cvfold=None, reserve=True, device=None,
                    semantic=None, nms="matrix", nms_thresh=None, segments=None, split=None, tiles=None, stitch=None,
                    density=None, views=None):
    """Yields (name, cls_final, scores_final, masks_final, pick) per scene, in input order.  raw_scenes: iterable of
    (name, raw [N, 8]).  The NMS categories are the benchmark label ids of the classes (evaluation.benchmark_label_ids
    with cvfold, default model.cfg.cvfold).  A scene without proposals yields ([], [], [], empty pick).  reserve: size
    the allocator for the largest batch first (GeoFormer.reserve_for with the batch's total points).  semantic: an
    evaluation.SemanticEvaluator that is given every batch's semantic scores, labels, offsets and scene names (one
    launch on the forward's stream before the NMS, nothing read back); None: nothing is added to the loop.  nms:
    "matrix" (matrix NMS with nms_kernel / sigma / final_score_thresh) or "greedy" (class-agnostic greedy NMS at
    nms_thresh, default model.cfg.TEST_NMS_THRESH; pick in pick order).  segments: collate_batches' mapping of
    over-segment ids; the forward pools the mask logits over them (every mask is then constant over a segment's
    foreground points); None: nothing is added to the loop.  A GeometricSegments (or "geometric"): the ids of every
    batch are computed on the device from its locs_float once the feeder has delivered it (one pointops.oversegment per
    scene, on the forward's stream, nothing read back) and stored as the batch's "segments".  split: "largest", "split"
    or a MaskSplit -- every scene's picked masks are split into spatially connected clusters after the NMS
    (postprocess.split_masks on the forward's stream, with the scene's xyz from the batch's locs_float): "largest" keeps
    the largest cluster of every picked mask (same shapes, nothing read back), "split" yields one row per kept cluster
    (pick = arange; one read-back per scene); None: nothing is added to the loop.  tiles: a Tiling -- every scene with
    more than its max_points points is replaced in the item list by its non-empty tiles (tile_items), the loop runs over
    the expanded list (same feeder, same batches of batch_size, segments= sliced or computed per tile, split= applied
    per tile), and when a scene's last tile has come out postprocess.merge_tiles joins the tiles' picked instances: the
    scene is yielded once, in input order, with masks int32 [G, N] over the whole scan holding the G merged instances
    only, and pick their score order (one read-back per tiled scene); None: nothing is added to the loop.  stitch:
    "core" or "mean", with tiles only -- how `semantic` is given a tiled scene: its tiles' scores are kept on the
    device until the scene's last tile is in, stitched into one [N, C] (postprocess.stitch_tiles: each point's row from
    its core tile, or the mean over the tiles that hold it) and counted once, under the scene's own name against the
    scene's own labels, before the scene is yielded; there is no default because neither rule's effect on mIoU has been
    measured.  With semantic=None there is nothing to stitch: stitch is checked and otherwise unused.  semantic= with
    tiles and stitch=None is a ValueError; stitch without tiles is one too; so is, with semantic= and stitch, a tiled
    scene whose name another scene of the list carries (the scores and labels of a scan are kept by its name).
    density: a Density -- subsample first: every scene is replaced by one representative point per occupied cell
    (density_items; pointops.grid_subsample on the device, one two-word read-back per scene), everything above --
    segments= (a mapping's ids gathered through the representatives), split=, tiles= / stitch= -- sees the subsampled
    scene, and expansion comes last: the scene is yielded once under its own name with masks int32 [R, N] over its own
    points (every point takes its representative's column) and `semantic` is given its scores on all N points against
    its own labels.  A scene that keeps every point runs exactly as without density=; a subsampled scene whose name
    another scene carries is a ValueError; None: nothing is added to the loop.  What subsampling does to AP or mIoU has
    not been measured.
    views: a Views -- test-time augmentation: every scene is replaced in the item list by its V views (view_items: the
    same points in the same order, rotated about z and optionally mirrored; view 0 is the scene itself), the loop runs
    over the expanded list (density= comes first, so the views are views of the subsampled scene; tiles= / stitch=,
    segments= and split= apply to every view: a large view is tiled and comes out merged as [G_v, N], a segments=
    mapping serves every view of a scene under the scene's name, "geometric" segments are computed per view), and when
    a scene's last view has come out postprocess.merge_views joins the views' picked instances: rows pair one to one
    by mutual best IoU, the mask is a per-point vote of the views, the score the views' mean with 0 for a view that
    missed the instance.  The scene is yielded once, in input order, under its own name, with masks int32 [G, N] (0 / 1)
    holding the G joined instances only and pick their score order (one read-back per scene); `semantic` is given the
    scene once, its scores the views' mean (postprocess.mean_views) against view 0's labels, before the scene is
    yielded, and two scenes of one name are then a ValueError.  Views(rotations=1) runs the join over the one view: it
    yields the picked rows that hold a point, as 0 / 1 masks with their own scores, in pick order -- a filter and a
    re-ordering.  None: nothing is added to the loop.  What the views do to AP or mIoU has not been measured."""
    _stitching(stitch, _tiling(tiles), "predict_batches")
    if _views(views) is not None and semantic is not None:
        raw_scenes = list(raw_scenes)
        _viewed_names(raw_scenes, "predict_batches")
    if _density(density) is not None:
        yield from _predict_dense(model, raw_scenes, batch_size, density, dict(
            epoch=epoch, spatial_shape=spatial_shape, nms_kernel=nms_kernel, sigma=sigma,
            final_score_thresh=final_score_thresh, cvfold=cvfold, reserve=reserve, device=device, semantic=semantic,
            nms=nms, nms_thresh=nms_thresh, segments=segments, split=split, tiles=tiles, stitch=stitch, views=views))
        return
    if views is not None:
        yield from _predict_views(model, raw_scenes, batch_size, views, dict(
            epoch=epoch, spatial_shape=spatial_shape, nms_kernel=nms_kernel, sigma=sigma,
            final_score_thresh=final_score_thresh, cvfold=cvfold, reserve=reserve, device=device, semantic=semantic,
            nms=nms, nms_thresh=nms_thresh, segments=segments, split=split, tiles=tiles, stitch=stitch))
        return
    if tiles is not None:
        yield from _predict_tiled(model, raw_scenes, batch_size, tiles, stitch, dict(
            epoch=epoch, spatial_shape=spatial_shape, nms_kernel=nms_kernel, sigma=sigma,
            final_score_thresh=final_score_thresh, cvfold=cvfold, reserve=reserve, device=device, semantic=semantic,
            nms=nms, nms_thresh=nms_thresh, segments=segments, split=split))
        return
    geo = _geometric(segments)
    splitter = _mask_split(split)
    if nms not in ("matrix", "greedy"):
        raise ValueError(f"predict_batches: nms must be 'matrix' or 'greedy', got {nms!r}")
    if nms == "greedy" and nms_thresh is None:
        nms_thresh = model.cfg.TEST_NMS_THRESH
    cvfold = model.cfg.cvfold if cvfold is None else cvfold
    dev = torch.device(device) if device is not None else next(model.parameters()).device
    model.eval()
    chunks, batches = collate_batches(raw_scenes, batch_size, spatial_shape, segments=None if geo else segments)
    if not batches:
        return
    most = max(int(b["offsets"][-1]) for b in batches)
    if reserve:
        model.reserve_for(most)
    for chunk, host, batch in zip(chunks, batches, DeviceFeeder(batches, dev, reserve_points=most)):
        if geo is not None:
            batch["segments"] = geo.of_batch(batch["locs_float"], host["offsets"])
        out = model(batch, epoch, training=False, all_scenes=True)
        if semantic is not None:
            semantic.add_batch(out["semantic_scores"], batch["labels"], batch["offsets"], [n for n, _ in chunk],
                               offsets_host=host["offsets"])
        per = out.get("proposal_scores_per_scene") or [([], [], []) for _ in chunk]
        if nms == "greedy":
            picks = postprocess.greedy_nms_batched([m for _, _, m in per], [s for _, s, _ in per], nms_thresh)
        else:
            labels = [evaluation.benchmark_label_ids(c, cvfold) if torch.is_tensor(c) else [] for c, _, _ in per]
            picks = postprocess.matrix_nms_batched([m for _, _, m in per], [s for _, s, _ in per], labels,
                                                   kernel=nms_kernel, sigma=sigma,
                                                   final_score_thresh=final_score_thresh)
        if splitter is not None:
            per, picks = list(per), list(picks)
            off = [int(o) for o in host["offsets"]]
            for b, ((cls, sc, masks), pick) in enumerate(zip(per, picks)):
                if torch.is_tensor(masks):
                    cls, sc, masks, picks[b] = splitter.of_scene(cls, sc, masks, pick,
                                                                 batch["locs_float"][off[b]:off[b + 1]].contiguous())
                    per[b] = (cls, sc, masks)
        for (name, _), (cls, sc, masks), pick in zip(chunk, per, picks):
            yield name, cls, sc, masks, pick


class _SemanticTap:
    """Stands where predict_batches takes a SemanticEvaluator: keeps every batch's semantic classes (int32, device) per
    scene name, and hands the batch on to the caller's own evaluator when there is one."""

    def __init__(self, inner=None):
        self.inner = inner
        self.preds = {}

    def add_batch(self, scores, labels, offsets, names, offsets_host=None):
        from . import pointops

        if self.inner is not None:
            preds = self.inner.add_batch(scores, labels, offsets, names, offsets_host=offsets_host)
        else:
            preds = pointops.semantic_confusion(scores.contiguous(), None, None, None)
        off = offsets_host.tolist()
        for i, n in enumerate(names):
            self.preds[n] = preds[off[i]:off[i + 1]]
        return preds


def _label_batches(model, raw_scenes, batch_size, min_score, keep_masks, panoptic, count_gt, kw):
    """The loop of label_batches; yields (name, SceneLabels, pan).  panoptic: None (pan is None and nothing is added to
    the loop) or an evaluation.PanopticEvaluator, whose class tables make the panoptic ids; with count_gt the
    batch is also counted against the ground truth of the raw scenes' columns 6 / 7."""
    items = list(raw_scenes)
    raws = dict(items)
    dev = torch.device(kw["device"]) if kw.get("device") is not None else next(model.parameters()).device
    pending = []
    tap = None
    if panoptic is not None:
        kw = dict(kw)
        tap = kw["semantic"] = _SemanticTap(kw.get("semantic"))

    def flush():
        cvfold = model.cfg.cvfold if kw.get("cvfold") is None else kw["cvfold"]
        ids = [evaluation.benchmark_label_ids(c, cvfold) if torch.is_tensor(c) else [] for _, c, *_ in pending]
        xyzs = [torch.as_tensor(np.asarray(raws[n])[:, :3].astype(np.float32)).to(dev, non_blocking=True)
                for n, *_ in pending]
        table, packed = postprocess._label_batch_packed([m for *_, m, _ in pending], [s for _, _, s, _, _ in pending],
                                                        ids, [p for *_, p in pending], xyzs, min_score)
        pans = [None] * len(pending)
        if panoptic is not None:
            pans = _panoptic_of_batch(panoptic, count_gt, [n for n, *_ in pending], raws, table, packed, tap, dev)
        # the batch's maps and tables cross in three copies, whatever the number of scenes
        out = postprocess._split_labels(table, *[b.cpu().numpy() for b in packed])
        for (name, _, _, masks, pick), lab, pan in zip(pending, out, pans):
            if keep_masks:
                m = masks[pick].cpu().numpy() if torch.is_tensor(masks) else np.zeros((0, lab.owner.shape[0]), np.int32)
                lab = lab._replace(masks=m)
            yield name, lab, pan
        pending.clear()

    for rec in predict_batches(model, items, batch_size, **kw):
        pending.append(rec)
        if len(pending) == batch_size:
            yield from flush()
    if pending:
        yield from flush()


def _panoptic_of_batch(ev, count_gt, names, raws, table, packed, tap, dev):
    """Host panoptic ids of one labelled batch (one more copy); with count_gt the batch's tables go to `ev`."""
    from . import pointops

    pts, ti, _ = packed
    sem = torch.cat([tap.preds.pop(n) for n in names]).contiguous()
    rows = postprocess.scene_rows(table, postprocess.LBL_ROW)
    off_h = torch.from_numpy(np.concatenate([[0], np.cumsum(rows["N"])]).astype(np.int32))
    P = int(rows["p"].max()) if len(rows) else 0
    if count_gt:
        gts = []
        for n in names:
            r = torch.as_tensor(np.asarray(raws[n])[:, 6:8], device=dev)
            gts.append(evaluation.gt_ids_from_labels(r[:, 0].long(), r[:, 1].long()))
        ti_h = ti.cpu().numpy()
        label_ids = [ti_h[o:o + p, postprocess._LBL_I.label_id] for o, p in rows[["row_off", "p"]].tolist()]
        pan = ev.add_batch(pts[0], pts[1], sem, torch.cat(gts), off_h.to(dev), label_ids, names, offsets_host=off_h)
    else:
        cls, st, sos = ev.device_tables(dev)
        pan = pointops.panoptic_points(pts[0].contiguous(), pts[1].contiguous(), sem, off_h.to(dev), cls, st, sos,
                                       ev.n_stuff, P)
    pan = pan.cpu().numpy()
    off = off_h.tolist()
    return [pan[off[i]:off[i + 1]] for i in range(len(names))]


@torch.no_grad()
def label_batches(model, raw_scenes, batch_size, *, min_score=postprocess.MIN_SCORE, keep_masks=False, **kw):
    """Yields (name, SceneLabels) per scene, in input order, with the results on the host: the loop of predict_batches
    with postprocess.label_points_batched once per batch of scenes.  Per scene the per-point maps (ids, owner) and the
    instance table cross to the host; the picked masks [p, N] (rank order, SceneLabels.masks) only with keep_masks=True.
    Keywords go to predict_batches."""
    for name, lab, _ in _label_batches(model, raw_scenes, batch_size, min_score, keep_masks, None, False, kw):
        yield name, lab


@torch.no_grad()
def panoptic_batches(model, raw_scenes, batch_size, *, min_score=postprocess.MIN_SCORE, keep_masks=False, classes=None,
                     stuff=evaluation.DEFAULT_STUFF_IDS, stuff_of_sem=None, evaluator=None, **kw):
    """Yields (name, SceneLabels, pan) per scene, in input order, on the host: the loop of label_batches plus the
    batch's semantic classes, joined by gf_panoptic_overlaps.  pan int32 [N]: the label map's id where a picked instance
    owns the point, stuff id * 1000 (1000 wall, 2000 floor) where the semantic head says so, 0 elsewhere.  classes: the
    thing classes (default: the model's cvfold); evaluator: an evaluation.PanopticEvaluator that also counts every
    batch against the ground truth of the raw scenes' columns 6 / 7 (its class tables are used).  Other keywords go to
    predict_batches."""
    ev = evaluator
    if ev is None:
        ev = evaluation.PanopticEvaluator(model.cfg.cvfold if classes is None else classes, stuff, stuff_of_sem)
    yield from _label_batches(model, raw_scenes, batch_size, min_score, keep_masks, ev, evaluator is not None, kw)


@torch.no_grad()
def evaluate_panoptic(model, scenes_with_gt, batch_size, classes=0, **kw):
    """PQ / SQ / RQ of the model's panoptic labelling over (name, raw [N, 8]) scenes whose columns 6 / 7 are the ground
    truth (evaluation.gt_ids_from_labels): evaluation.PanopticEvaluator.evaluate's dict.  Keywords go to
    panoptic_batches."""
    ev = kw.pop("evaluator", None)
    if ev is None:
        ev = evaluation.PanopticEvaluator(classes, kw.pop("stuff", evaluation.DEFAULT_STUFF_IDS),
                                          kw.pop("stuff_of_sem", None))
    for _ in panoptic_batches(model, scenes_with_gt, batch_size, evaluator=ev, **kw):
        pass
    return ev.evaluate()


@torch.no_grad()
def evaluate(model, scenes_with_gt, batch_size, classes=0, *, cvfold=None, boxes=None, **kw):
    """ScanNet AP / AP50 / AP25 of the model over (name, raw [N, 8]) scenes whose labels are the ground truth
    (evaluation.gt_ids_from_labels): (ap [C, n_overlaps], averages), as evaluation.InstanceEvaluator.evaluate.
    boxes: an evaluation.BoxEvaluator that is given every scene of the same pass with the scene's own xyz (box AP from
    the pass that gives AP); None: nothing is added to the loop.  Other keywords go to predict_batches."""
    cvfold = model.cfg.cvfold if cvfold is None else cvfold
    items = list(scenes_with_gt)
    raws = dict(items)
    ev = evaluation.InstanceEvaluator(classes=classes)
    dev = next(model.parameters()).device
    for name, cls, sc, masks, pick in predict_batches(model, items, batch_size, cvfold=cvfold, **kw):
        if not torch.is_tensor(cls):
            continue  # test.py: a scene without proposals is skipped
        r = torch.as_tensor(np.asarray(raws[name]), device=dev)
        gt = evaluation.gt_ids_from_labels(r[:, 6].long(), r[:, 7].long())
        labels = evaluation.benchmark_label_ids(cls, cvfold)
        ev.add_scene(name, gt, labels, sc, masks, pick)
        if boxes is not None:
            boxes.add_scene(name, gt, labels, sc, masks, pick, r[:, :3].to(torch.float32).contiguous())
    return ev.evaluate()


@torch.no_grad()
def evaluate_boxes(model, scenes_with_gt, batch_size, classes=0, kind="aligned", *, cvfold=None, evaluator=None, **kw):
    """Box AP (detection mAP@0.25 / mAP@0.5 over the 3D boxes of the picked masks) of the model over (name, raw [N, 8])
    scenes whose columns 6 / 7 are the ground truth: evaluation.BoxEvaluator.evaluate's dict.  kind: "aligned" or
    "oriented"; evaluator: a BoxEvaluator of the caller's (classes and kind are then its own); overlaps, angles and
    min_points go to the BoxEvaluator, other keywords to predict_batches.  Per scene: the two native calls of
    BoxEvaluator.add_scene on the forward's device and one small copy.  A scene without proposals is left out, as in
    evaluate.  A tiled or subsampled scan (tiles=, density=) comes out of predict_batches over its own points and is
    boxed on the raw scan's xyz."""
    cvfold = model.cfg.cvfold if cvfold is None else cvfold
    ev = evaluator
    if ev is None:
        ev = evaluation.BoxEvaluator(classes, kind, **{k: kw.pop(k) for k in ("overlaps", "angles", "min_points") if k in kw})
    items = list(scenes_with_gt)
    raws = dict(items)
    dev = next(model.parameters()).device
    for name, cls, sc, masks, pick in predict_batches(model, items, batch_size, cvfold=cvfold, **kw):
        if not torch.is_tensor(cls):
            continue
        r = torch.as_tensor(np.asarray(raws[name]), device=dev)
        gt = evaluation.gt_ids_from_labels(r[:, 6].long(), r[:, 7].long())
        ev.add_scene(name, gt, evaluation.benchmark_label_ids(cls, cvfold), sc, masks, pick,
                     r[:, :3].to(torch.float32).contiguous())
    return ev.evaluate()


def _semantic_forwards(model, raw_scenes, batch_size, spatial_shape, reserve, device):
    """The forwards of semantic_batches: yields (chunk, host batch, device batch, scores fp32 [N, C] contiguous) per
    batch."""
    dev = torch.device(device) if device is not None else next(model.parameters()).device
    model.eval()
    chunks, batches = collate_batches(raw_scenes, batch_size, spatial_shape)
    if not batches:
        return
    most = max(int(b["offsets"][-1]) for b in batches)
    if reserve:
        model.reserve_for(most)
    for chunk, host, batch in zip(chunks, batches, DeviceFeeder(batches, dev, reserve_points=most)):
        _, scores, _ = model.forward_backbone(batch, len(chunk), want_preds=False)
        yield chunk, host, batch, scores.contiguous()


@torch.no_grad()
def semantic_batches(model, raw_scenes, batch_size, *, spatial_shape=None, reserve=True, device=None, evaluator=None,
                     tiles=None, stitch=None, density=None, views=None):
    """Yields (name, preds) per scene, in input order: preds int32 [N] on the device, a view of the batch's buffer -- the
    semantic head's class of every point (the first maximal score, the rule of the forward's foreground selection).
    Only the backbone and the semantic head run (forward_backbone with the fused voxel-row head; no arg-max by the
    framework, no instance stage): the loop of the first ``prepare_epochs``.  evaluator: an evaluation.SemanticEvaluator
    that counts every batch against its labels in the same launch.  tiles: a Tiling, with stitch "core" or "mean" (both
    or neither: ValueError) -- every scene with more than max_points points runs as its non-empty tiles (tile_items), the
    tiles' scores are kept on the device until the scene is complete and stitched (postprocess.stitch_tiles), and the
    scene is counted and yielded once, under its own name, with preds int32 [N] over the whole scan.  density: a Density
    -- every scene runs subsampled (density_items; tiles= then cuts the subsampled scene), its scores -- stitched, when
    tiled -- are put back on its own points through cell_of, and it is counted against its own labels and yielded with
    preds int32 [N].  views: a Views -- every scene (subsampled first, with density=) runs under its V views (view_items;
    tiles= then cuts every view), the views' scores -- stitched, when tiled -- are kept on the device until the last view
    is in, averaged (postprocess.mean_views) and counted once against view 0's labels; two scenes of one name are a
    ValueError."""
    from . import pointops

    tiling = _tiling(tiles)
    _stitching(stitch, tiling, "semantic_batches")
    if tiling is not None and stitch is None:
        raise ValueError('semantic_batches: tiles= needs stitch="core" or "mean"')
    if _views(views) is not None:
        raw_scenes = list(raw_scenes)
        _viewed_names(raw_scenes, "semantic_batches")
    if tiling is not None or _density(density) is not None or views is not None:
        items = list(raw_scenes)
        sem = tap = _SemanticTap(evaluator)
        plans = {}
        if density is not None:
            dev = torch.device(device) if device is not None else next(model.parameters()).device
            raws = items
            items, maps = density_items(raws, density, dev)
            sem = _DensitySemantics(tap, maps, {n: r for n, r in raws if n in maps})
        if views is not None:
            items = view_items(items, views)
            sem = _ViewSemantics(sem, views.V)
        expanded = items
        if tiling is not None:
            expanded, plans = tile_items(items, tiling)
            sem = _TileSemantics(sem, plans, _tiled_raws(items, plans), stitch)
        for chunk, host, batch, scores in _semantic_forwards(model, expanded, batch_size, spatial_shape, reserve, device):
            sem.add_batch(scores, batch["labels"], batch["offsets"], [n for n, _ in chunk], offsets_host=host["offsets"])
            for name, _ in chunk:
                # a scan is complete with its last tile, and is yielded in that tile's place
                name = name[0] if isinstance(name, TileName) and name[0] in plans else name
                name = name[0] if isinstance(name, ViewName) else name  # ... and a scene with its last view
                if name in tap.preds:
                    yield name, tap.preds.pop(name)
        return
    for chunk, host, batch, scores in _semantic_forwards(model, raw_scenes, batch_size, spatial_shape, reserve, device):
        if evaluator is not None:
            preds = evaluator.add_batch(scores, batch["labels"], batch["offsets"], [n for n, _ in chunk],
                                        offsets_host=host["offsets"])
        else:
            preds = pointops.semantic_confusion(scores, None, None, None)
        off = host["offsets"].tolist()
        for i, (name, _) in enumerate(chunk):
            yield name, preds[off[i]:off[i + 1]]


@torch.no_grad()
def evaluate_semantic(model, scenes_with_gt, batch_size, **kw):
    """mIoU / accuracy / foreground-filter quality of the semantic head over (name, raw [N, 8]) scenes whose column 6 is
    the ground truth (raw dataset labels): evaluation.SemanticEvaluator.evaluate's dict, with the class count and the
    train fold of model.cfg.  Keywords go to semantic_batches."""
    ev = kw.pop("evaluator", None)
    if ev is None:
        ev = evaluation.SemanticEvaluator(n_classes=model.cfg.classes, train_fold=model.cfg.train_fold)
    for _ in semantic_batches(model, scenes_with_gt, batch_size, evaluator=ev, **kw):
        pass
    return ev.evaluate()
