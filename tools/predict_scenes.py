"""Label maps and ScanNet benchmark files of scenes: the eval forward, matrix NMS (or, with --nms greedy, the reference's
greedy NMS) and the scene labelling of batch_eval.label_batches, written with geoformer_amd.export.

    python tools/predict_scenes.py --out out scene0011_00_inst_nostuff.npy ...      # [N, 8] as prepare_data_inst.py stores them
    python tools/predict_scenes.py --out out --synthetic 8 --points 150000 --batch-size 4
    python tools/predict_scenes.py --synthetic 8 --no-write                          # only the timing
    python tools/predict_scenes.py --out out --semantic scene0011_00_inst_nostuff.npy   # + out/semantic/<name>.txt, mIoU
    python tools/predict_scenes.py --out out --panoptic scene0011_00_inst_nostuff.npy   # + `panoptic` in the .npz, PQ
    python tools/predict_scenes.py --out out --segments segs scene0011_00_inst_nostuff.npy  # masks pooled over segs/<name>*.segs.json
    python tools/predict_scenes.py --out out --geometric-segments scene0011_00_inst_nostuff.npy  # ... over segments made from the points
    python tools/predict_scenes.py --out out --split-masks largest scene0011_00_inst_nostuff.npy  # picked masks cut to their largest connected cluster
    python tools/predict_scenes.py --out out --tile 4 --halo 0.5 floor3.npy               # a large scan as overlapping 4 m tiles, instances joined
    python tools/predict_scenes.py --out out --tile 4 --tile-stitch core --panoptic floor3.npy  # ... and the tiles' semantics stitched: PQ of the scan
    python tools/predict_scenes.py --out out --render turntable:4 scene0011_00_inst_nostuff.npy  # + out/render/<name>_instance_pred_<view>.png
    python tools/predict_scenes.py --out out --density 0.02 laser_scan.npy                 # a dense scan on one point per 2 cm cell, labels on every point
    python tools/predict_scenes.py --out out --boxes oriented scene0011_00_inst_nostuff.npy  # + out/boxes/<name>.txt, one 3D box per instance
    python tools/predict_scenes.py --out out --views 4 scene0011_00_inst_nostuff.npy         # 4 rotated views per scene, instances joined by vote

Per scene <out>/<name>.npz (ids, owner, instance table: export.load_labels) and, with --scannet, <out>/<name>.txt plus
<out>/predicted_masks/ (exclusive masks; --full-masks writes the picked masks as they are).  Without --checkpoint the
benchmark's synthetic model (bench.build_model) runs.  Prints one JSON line with the scenes per second of the
label_batches loop, results on the host, for keep_masks off and on, beside the bare predict_batches loop (wall clock,
host collate included, files not).  --semantic (or the yaml's save_semantic) adds one pass of
batch_eval.semantic_batches: <out>/semantic/<name>.txt, the ScanNet semantic benchmark's file (one label id per point),
and, when the scenes carry labels, the mIoU table of evaluation.SemanticEvaluator before the JSON line.  --panoptic
takes the label maps from batch_eval.panoptic_batches instead: <out>/<name>.npz also holds `panoptic` (the instance id,
1000 wall, 2000 floor, 0 unlabelled per point), and, when the scenes carry labels, the PQ / SQ / RQ table of
evaluation.PanopticEvaluator is printed before the JSON line.  --segments DIR pools every scene's mask logits over its
over-segmentation before the proposals (csrc/segment_pool.hip): <DIR>/<name>*.segs.json (ScanNet's, field segIndices)
or <DIR>/<name>.segs.npy, one id per point; for the --synthetic scenes scene.grid_segments stands in (DIR is not read).
--geometric-segments (instead of --segments) computes the over-segmentation on the GPU from every scene's points
(pointops.oversegment with its defaults, csrc/oversegment.hip), for given and synthetic scenes alike.
The JSON line's `segment_pooling` says whether the pooling ran, `geometric_segments` where the segments came from.
--split-masks largest|split splits every picked mask into spatially connected clusters after the NMS (DBSCAN per mask,
batch_eval.MaskSplit with its defaults, csrc/mask_split.hip): `largest` keeps each mask's largest cluster, `split` makes
every kept cluster an instance of its own.  The JSON line's `mask_split` names the mode (null without the flag).
--tile M runs every scene of more than --tile-max-points points as overlapping tiles of about M metres in x / y (halo
--halo M on every side) and joins the instances of the tiles (batch_eval.Tiling, csrc/tile_merge.hip).  --tile-stitch
core|mean also stitches the tiles' semantic scores per scan (batch_eval's stitch=, csrc/tile_stitch.hip): each point's
scores from its core tile, or the mean over the tiles that hold it; --panoptic goes with --tile only then, and the
--semantic pass then runs over the tiles too (without it that pass runs every scan whole).  The JSON line's `tiling`
holds the parameters and `stitch` (null without --tile).
--render top|turntable:K draws every scene on the GPU (geoformer_amd.render, csrc/render.hip) from above or from K views
around it, --render-size WxH pixels, in the colours of --render-task (input, semantic_gt, semantic_pred, instance_gt,
instance_pred; semantic_pred takes the classes of the --semantic pass, which it switches on):
<out>/render/<name>_<task>_<view>.png, 8-bit RGB.
--density CELL runs every scene on one representative point per occupied CELL-metre cell (batch_eval.Density,
csrc/resample.hip; --density-mode center: the point nearest the cell's centre, first: the cell's first point) and puts
every result back on the scene's own points; tiles, segments and the mask split then see the subsampled scene.  The
JSON line's `density` holds the parameters (null without the flag).
--boxes aligned|oriented writes <out>/boxes/<name>.txt: one line per kept instance of the label map that owns a point,
``cx cy cz du dv dz yaw label_id score`` (export.write_boxes), the box of the points the instance owns
(postprocess.id_boxes over the map's owner column on the GPU, csrc/boxes.hip): axis-aligned, or the upright box of least
footprint among 90 headings.  The JSON line's `boxes` names the kind (null without the flag) and `boxes_written` the
count.
--views K runs every scene under K views -- rotations about z by 360 / K degrees, with --view-flip each followed by its
x-mirrored twin (2 K views) -- and joins the views' picked instances (batch_eval.Views, csrc/view_merge.hip): rows pair
one to one by mutual best IoU of at least --view-iou (0.5), an instance needs members in --view-min views (default: half
of them, rounded up), a point belongs to it when at least --view-vote (0.5) of its views say so, and its score is the
views' mean, 0 for a view that missed it.  The --semantic pass then averages the views' scores.  Tiles, segments and the
mask split apply to every view; --density comes first.  The three thresholds are chosen by reasoning, not measured.
The JSON line's `views` holds the parameters (null without the flag).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_views(text):
    """top -> ("top", 1); turntable:K -> ("turntable", K)."""
    if text == "top":
        return ("top", 1)
    kind, _, k = text.partition(":")
    if kind != "turntable" or not k.isdigit() or int(k) < 1:
        raise argparse.ArgumentTypeError(f"expected top or turntable:K with K >= 1, got {text!r}")
    return ("turntable", int(k))


def parse_size(text):
    w, _, h = text.lower().partition("x")
    if not (w.isdigit() and h.isdigit() and int(w) >= 1 and int(h) >= 1):
        raise argparse.ArgumentTypeError(f"expected WxH, got {text!r}")
    return (int(w), int(h))


RENDER_TASKS = ("input", "semantic_gt", "semantic_pred", "instance_gt", "instance_pred")


def cameras_of(views, xyz, size):
    from geoformer_amd import render

    bounds = render.bounds_of(xyz)
    return [render.top_down(bounds, size)] if views[0] == "top" else render.turntable(bounds, views[1], 30.0, size)


def write_renders(out_dir, results, raws, views, size, task, semantic=None, device="cuda"):
    """<out_dir>/render/<name>_<task>_<view>.png of every (name, SceneLabels) of results, drawn on the device with
    render.render's defaults; raws: name -> raw [N, 8]; semantic: name -> classes [N] (for semantic_pred).  Returns the
    paths."""
    from geoformer_amd import export, render

    os.makedirs(os.path.join(out_dir, "render"), exist_ok=True)
    paths = []
    for name, lab in results:
        raw = np.asarray(raws[name])
        xyz = torch.as_tensor(raw[:, :3].astype(np.float32), device=device)
        rgb, ids, keep = render.colors_for(task, raw_scene=raw, labels=lab, semantic=(semantic or {}).get(name),
                                           device=device)
        image, _ = render.render(xyz, rgb, cameras_of(views, xyz, size), size, ids=ids, keep=keep)
        for v, im in enumerate(image.cpu().numpy()):
            paths.append(export.write_png(os.path.join(out_dir, "render", f"{name}_{task}_{v}.png"), im))
    return paths


def write_boxes(out_dir, results, raws, kind, device="cuda"):
    """<out_dir>/boxes/<name>.txt of every (name, SceneLabels) of results: the box of the points every kept instance
    owns, computed on the device; raws: name -> raw [N, 8].  Returns the number of boxes written."""
    from geoformer_amd import export, postprocess

    written = 0
    for name, lab in results:
        xyz = torch.as_tensor(np.asarray(raws[name])[:, :3].astype(np.float32), device=device)
        p = int(lab.table.count.shape[0])
        b = postprocess.id_boxes(torch.as_tensor(lab.owner, device=device), p, xyz, oriented=kind == "oriented")
        rows = b.rows.cpu().numpy()
        count = rows[:, postprocess._BOX.count]
        on = count > 0  # (an instance that is not kept, or that lost every point to better ones, owns nothing)
        b = postprocess._boxes_from_rows(rows[on], count[on].astype(np.int32), postprocess.BOX_ANGLES if kind == "oriented" else 1)
        export.write_boxes(os.path.join(out_dir, "boxes", f"{name}.txt"), b, np.asarray(lab.table.label_id)[on],
                           np.asarray(lab.table.score)[on])
        written += int(on.sum())
    return written


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("scenes", nargs="*", help="scene .npy files, [N, 8] = xyz, rgb, semantic label, instance label")
    ap.add_argument("--synthetic", type=int, default=0, metavar="K", help="K synthetic scenes (scene.make_raw_scene)")
    ap.add_argument("--points", type=int, default=150_000, help="points per synthetic scene")
    ap.add_argument("--out", default="predictions")
    ap.add_argument("--batch-size", type=int, default=4)
    ap.add_argument("--min-score", type=float, default=None, help="default: postprocess.MIN_SCORE (0.09)")
    ap.add_argument("--nms-score", type=float, default=None, help="final_score_thresh of the matrix NMS (default 0.5)")
    ap.add_argument("--nms", choices=("matrix", "greedy"), default="matrix",
                    help="matrix NMS (test.py:88-93) or class-agnostic greedy NMS at the yaml's TEST_NMS_THRESH (test.py:78-86)")
    ap.add_argument("--checkpoint", default=None, help="state dict (torch.save) of a GeoFormer of --config")
    ap.add_argument("--config", default="test_geoformer_scannet.yaml")
    ap.add_argument("--scannet", action="store_true", help="also write the benchmark's .txt files")
    ap.add_argument("--full-masks", action="store_true", help="benchmark files hold the picked masks, not the exclusive ones")
    ap.add_argument("--semantic", action="store_true", help="also write <out>/semantic/<name>.txt and print the mIoU table")
    ap.add_argument("--panoptic", action="store_true",
                    help="also store the panoptic ids (things + wall / floor) in <out>/<name>.npz and print the PQ table")
    seg_from = ap.add_mutually_exclusive_group()
    seg_from.add_argument("--geometric-segments", action="store_true",
                          help="pool the mask logits over a geometric over-segmentation computed on the GPU from each "
                               "scene's points (batch_eval.GeometricSegments with its defaults)")
    seg_from.add_argument("--segments", default=None, metavar="DIR",
                          help="pool the mask logits over each scene's over-segmentation: DIR/<name>*.segs.json or "
                               "DIR/<name>.segs.npy (synthetic scenes: scene.grid_segments)")
    ap.add_argument("--split-masks", choices=("largest", "split"), default=None,
                    help="split every picked mask into spatially connected clusters after the NMS (batch_eval.MaskSplit "
                         "with its defaults): keep the largest cluster, or make every kept cluster an instance")
    ap.add_argument("--tile", type=float, default=None, metavar="M",
                    help="run scenes of more than --tile-max-points points as overlapping tiles of about M metres and "
                         "join the instances of the tiles (batch_eval.Tiling)")
    ap.add_argument("--halo", type=float, default=None, metavar="M", help="overlap of the tiles on every side (default 0.5)")
    ap.add_argument("--tile-max-points", type=int, default=None, metavar="N",
                    help="scenes with at most N points run whole (default 400000)")
    ap.add_argument("--tile-stitch", choices=("core", "mean"), default=None,
                    help="with --tile: stitch the tiles' semantic scores per scan, each point from its core tile or the "
                         "mean over the tiles that hold it (batch_eval's stitch=); needed for --tile --panoptic")
    ap.add_argument("--density", type=float, default=None, metavar="CELL",
                    help="run every scene on one point per occupied CELL-metre cell and put the results back on its own "
                         "points (batch_eval.Density)")
    ap.add_argument("--density-mode", choices=("first", "center"), default=None,
                    help="with --density: the cell's representative (default center)")
    ap.add_argument("--render", type=parse_views, default=None, metavar="top|turntable:K",
                    help="draw every scene on the GPU from above, or from K views around it: <out>/render/*.png")
    ap.add_argument("--render-size", type=parse_size, default=(1024, 768), metavar="WxH")
    ap.add_argument("--render-task", choices=RENDER_TASKS, default="instance_pred", help="what the colours show")
    ap.add_argument("--boxes", choices=("aligned", "oriented"), default=None,
                    help="also write <out>/boxes/<name>.txt: one 3D box per kept instance (postprocess.id_boxes)")
    ap.add_argument("--views", type=int, default=None, metavar="K",
                    help="run every scene under K views rotated about z by 360 / K degrees and join the views' "
                         "instances by mutual best IoU, a per-point vote and the mean score (batch_eval.Views)")
    ap.add_argument("--view-flip", action="store_true", help="with --views: follow every rotation by its x-mirrored twin")
    ap.add_argument("--view-iou", type=float, default=None, metavar="X",
                    help="with --views: least IoU of two rows that join (default 0.5, not measured)")
    ap.add_argument("--view-min", type=int, default=None, metavar="N",
                    help="with --views: least number of views with a member (default: half the views, rounded up)")
    ap.add_argument("--view-vote", type=float, default=None, metavar="X",
                    help="with --views: least share of an instance's views that must hold a point (default 0.5, not measured)")
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--reps", type=int, default=3, help="timed passes per keep_masks setting")
    return ap


def main():
    ap = build_parser()
    args = ap.parse_args()

    import geoformer_amd

    geoformer_amd.configure_runtime()
    import bench
    from geoformer_amd import batch_eval, export, postprocess, scene
    from geoformer_amd.model import GeoFormer, load_config

    items = [(os.path.splitext(os.path.basename(p))[0], np.load(p)) for p in args.scenes]
    items += [(f"synthetic{i:04d}", scene.make_raw_scene(args.points, 500 + i)) for i in range(args.synthetic)]
    if not items:
        ap.error("no scenes: give .npy files or --synthetic K")
    for name, raw in items:
        if raw.ndim != 2 or raw.shape[1] != 8:
            ap.error(f"{name}: expected [N, 8], got {raw.shape}")
    dev = torch.device("cuda")
    if args.checkpoint:
        model = GeoFormer(load_config(args.config))
        sd = torch.load(args.checkpoint, map_location="cpu")
        model.load_state_dict(sd.get("state_dict", sd) if isinstance(sd, dict) else sd)
        model.to(dev)
        model.eval()
    else:
        probe = scene.make_batch([batch_eval.scene_dict(items[0][1])])
        model = bench.build_model(dev, probe_batch=bench.to_device(probe, dev), cfg_name=args.config)
    kw = {"min_score": postprocess.MIN_SCORE if args.min_score is None else args.min_score}
    if args.segments is not None:
        import glob

        segs = {}
        for i, (name, raw) in enumerate(items):
            if i >= len(args.scenes):  # a synthetic scene
                segs[name] = scene.grid_segments(raw)
                continue
            npy = os.path.join(args.segments, f"{name}.segs.npy")
            found = sorted(glob.glob(os.path.join(glob.escape(args.segments), glob.escape(name) + "*.segs.json")))
            if os.path.exists(npy):
                segs[name] = np.load(npy)
            elif found:
                segs[name] = export.load_scannet_segments(found[0])
            else:
                ap.error(f"--segments: neither {npy} nor {name}*.segs.json in {args.segments}")
            if segs[name].shape != (raw.shape[0],):
                ap.error(f"--segments: {name}: {segs[name].shape[0]} ids for {raw.shape[0]} points")
        kw["segments"] = segs
    if args.geometric_segments:
        kw["segments"] = batch_eval.GeometricSegments()
    if args.nms_score is not None:
        kw["final_score_thresh"] = args.nms_score
    if args.nms != "matrix":
        kw["nms"] = args.nms
    if args.split_masks is not None:
        kw["split"] = args.split_masks
    tiling = None
    if args.tile is not None:
        if args.panoptic and args.tile_stitch is None:
            ap.error("--tile: --panoptic is not supported with tiles yet without --tile-stitch core|mean")
        more = {k: v for k, v in (("halo", args.halo), ("max_points", args.tile_max_points)) if v is not None}
        tiling = kw["tiles"] = batch_eval.Tiling(tile=args.tile, **more)
        if args.tile_stitch is not None:
            kw["stitch"] = args.tile_stitch
    elif args.halo is not None or args.tile_max_points is not None or args.tile_stitch is not None:
        ap.error("--halo, --tile-max-points and --tile-stitch go with --tile")

    density = None
    if args.density is not None:
        if not args.density > 0:
            ap.error("--density: CELL > 0")
        density = kw["density"] = batch_eval.Density(cell=args.density, mode=args.density_mode or "center")
    elif args.density_mode is not None:
        ap.error("--density-mode goes with --density")

    views = None
    if args.views is not None:
        more = {k: v for k, v in (("iou", args.view_iou), ("min_views", args.view_min), ("vote", args.view_vote))
                if v is not None}
        try:
            views = kw["views"] = batch_eval.Views(rotations=args.views, flip=args.view_flip, **more)
        except ValueError as e:
            ap.error(f"--views: {e}")
    elif args.view_flip or args.view_iou is not None or args.view_min is not None or args.view_vote is not None:
        ap.error("--view-flip, --view-iou, --view-min and --view-vote go with --views")

    def run(keep_masks):
        np.random.seed(0)
        return list(batch_eval.label_batches(model, items, args.batch_size, keep_masks=keep_masks, **kw))

    pans, pq = {}, None
    if args.panoptic:
        from geoformer_amd import evaluation

        np.random.seed(0)
        pq = evaluation.PanopticEvaluator(classes=model.cfg.cvfold)
        results = []
        for name, lab, pan in batch_eval.panoptic_batches(model, items, args.batch_size, keep_masks=args.full_masks,
                                                          evaluator=pq, **kw):
            results.append((name, lab))
            pans[name] = pan
    else:
        results = run(args.full_masks)
    if not args.no_write:
        os.makedirs(args.out, exist_ok=True)
        for name, lab in results:
            export.save_labels(os.path.join(args.out, f"{name}.npz"), lab._replace(masks=None), pans.get(name))
            if args.scannet:
                export.write_scannet_predictions(args.out, name, lab, lab.masks if args.full_masks else None)
    boxes_written = 0
    if args.boxes is not None and not args.no_write:
        boxes_written = write_boxes(args.out, results, dict(items), args.boxes, dev)
    sem_preds = {}
    if args.semantic or getattr(model.cfg, "save_semantic", False) or (args.render and args.render_task == "semantic_pred"):
        from geoformer_amd import evaluation

        ev = evaluation.SemanticEvaluator(n_classes=model.cfg.classes, train_fold=model.cfg.train_fold)
        skw = {"tiles": tiling, "stitch": args.tile_stitch} if args.tile_stitch is not None else {}
        if density is not None:
            skw["density"] = density
        if views is not None:
            skw["views"] = views
        for name, preds in batch_eval.semantic_batches(model, items, args.batch_size, evaluator=ev, **skw):
            if not args.no_write:
                export.write_scannet_semantic(os.path.join(args.out, "semantic"), name, preds, model.cfg.train_fold)
            if args.render and args.render_task == "semantic_pred":
                sem_preds[name] = preds.clone()  # (a view of the batch's buffer)
        if any((raw[:, 6] != evaluation.IGNORE_LABEL).any() for _, raw in items):
            print(ev.format_results())
    if pq is not None and any((raw[:, 6] != -100).any() for _, raw in items):
        print(pq.format_results())
    if args.render and not args.no_write:
        write_renders(args.out, results, dict(items), args.render, args.render_size, args.render_task, sem_preds, dev)
    pkw = {k: v for k, v in kw.items() if k != "min_score"}

    def predict_only():  # the loop without the labelling and without any copy of a result, for comparison
        np.random.seed(0)
        n = sum(int(pick.numel()) for *_, pick in batch_eval.predict_batches(model, items, args.batch_size, **pkw))
        torch.cuda.synchronize()
        return n

    rates = {}
    for key, fn in (("predict_batches_only", predict_only), ("labels_only", lambda: run(False)),
                    ("keep_masks", lambda: run(True))):
        fn()  # (warm: allocator, launch plans)
        best = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            best.append(len(items) / (time.perf_counter() - t))
        rates[key] = [round(x, 2) for x in sorted(best)]
    kept = sum(int(np.sum(lab.table.kept)) for _, lab in results)
    print(json.dumps({"scenes": len(items), "batch_size": args.batch_size, "min_score": kw["min_score"],
                      "points": int(sum(r.shape[0] for _, r in items)),
                      "picked": sum(len(lab.table.kept) for _, lab in results), "kept": kept,
                      "labelled_points": sum(int((lab.owner >= 0).sum()) for _, lab in results),
                      "segment_pooling": "segments" in kw, "geometric_segments": args.geometric_segments,
                      "mask_split": args.split_masks, "tiling": dict(tiling.params, stitch=args.tile_stitch) if tiling else None,
                      "density": density.params if density else None, "views": views.params if views else None,
                      "boxes": args.boxes,
                      "boxes_written": boxes_written, "scenes_per_s": rates, "out": None if args.no_write else args.out}))


if __name__ == "__main__":
    main()
