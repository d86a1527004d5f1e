"""Instance labels for posed depth frames: the frames are fused into one scene on the GPU (geoformer_amd.frames,
csrc/frames.hip), the scene goes through batch_eval.label_batches, and the labels come back to every frame through the
pixel-to-point map -- exactly, with no projection or occlusion guess.

    python tools/predict_frames.py --frames scan.npz --out out
    python tools/predict_frames.py --frames scan.npz --cell 0.03 --stride 2 --far 5 --edge 0.05 --min-obs 2 --out out

scan.npz holds depth uint16 (millimetres; --depth-shift for another unit) or float32 [F, H, W], K [4] or [F, 4] =
(fx, fy, cx, cy), pose [F, 4, 4] camera to world (camera axes x right, y down, z forward) and optionally color uint8
[F, H, W, 3].  Written: <out>/<name>.ply (the fused points, export.write_ply), <out>/<name>.npz (export.save_labels) and
per frame <out>/frames/<name>_<f>.npy (int32 [Hs, Ws]: the label id of every sampled pixel, 0 without an instance, -1
where the pixel has no point) and <out>/frames/<name>_<f>.png in render.instance_colors (white: no point).  Without
--checkpoint the benchmark's synthetic model runs.  Prints one JSON line.

    python tools/predict_frames.py --frames scan.npz --chunk-frames 8 --out out

With --chunk-frames K the frames go through a frames.Fuser (csrc/frames_stream.hip) K at a time, so that only one
chunk's images are on the device at a time; the grid's origin is then the first chunk's minimum minus 64 m, not the
minimum of all points, which moves the cell borders and nothing else.  Without the flag nothing changes.

    python tools/predict_frames.py --frames scan.npz --labels --label-ignore 0 --out out

With --labels, scan.npz also holds label and instance, uint8, uint16 or int32 [F, H, W]: per pixel the class in the
coding the scene is to carry (the scores below expect the dataset's 0..19) and an instance id that is consistent across
the frames; --label-ignore is the value of unannotated pixels, which do not vote (0 in ScanNet's label-filt and
instance-filt images as shipped; whatever the remapping to 0..19 left for them otherwise).  They are lifted onto the fused points by vote (frames.lift_scene, csrc/frames_vote.hip), the scene
is written with its labels as <out>/<name>_scene.npy (float64 [n, 8], what batch_eval.* and augment.train_merge take),
and it is scored: batch_eval.evaluate (AP) and evaluation.SemanticEvaluator (mIoU), under "lifted" in the JSON line.
With --chunk-frames K and --labels together, the label and instance images go through two frames.Voter
(csrc/frames_vote_stream.hip) K frames at a time beside the Fuser and the labelled scene comes from
frames.lift_scene_stream: the same bytes, with one chunk of images on the device at a time ("voter" in the JSON line).

    python tools/predict_frames.py --frames scan.npz --chunk-frames 8 --track --track-every 2 --out out

With --track (only with --chunk-frames) the model also runs on the Fuser's snapshot after every J-th chunk (--track-every,
default 1) and after the last one, and a frames.Tracker (csrc/frames_track.hip) carries the instance ids from run to run
(--track-iou, --track-max-misses: its parameters).  The per-frame .npy then hold the track id of every pixel (-1 without
a track or a point) and the .png its colour in render.instance_colors; <out>/tracks.npz holds the track table and
"track" in the JSON line the counts.  Without --track the output is what it was.

    python tools/predict_frames.py --frames scan.npz --chunk-frames 8 --carve --out out

With --carve (only with --chunk-frames) a frames.Carver (csrc/frames_carve.hip) observes every chunk after it is added:
a cell that later frames look through loses score, and cells at or below --carve-drop (default -2) are left out of the
scene, of the lifted labels and of the tracker's points (--carve-band: the tolerance in metres, default three cells).
"carve" under "stream" in the JSON line holds the counts.  Without --carve the output is what it was.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", required=True, metavar="FILE.npz", help="depth, K, pose and optionally color")
    ap.add_argument("--out", default="predictions")
    ap.add_argument("--cell", type=float, default=0.02, help="metres: one fused point per cell")
    ap.add_argument("--stride", type=int, default=1, help="every stride-th pixel of every stride-th row")
    ap.add_argument("--near", type=float, default=0.1)
    ap.add_argument("--far", type=float, default=10.0)
    ap.add_argument("--edge", type=float, default=None, help="drop pixels at relative depth jumps above this (off)")
    ap.add_argument("--min-obs", type=int, default=1, help="drop cells seen by fewer pixels")
    ap.add_argument("--depth-shift", type=float, default=None, help="depth units per metre (1000 for uint16, 1 for float32)")
    ap.add_argument("--chunk-frames", type=int, default=0, metavar="K",
                    help="fuse the frames K at a time through a frames.Fuser: one chunk on the device at a time")
    ap.add_argument("--checkpoint", default=None, help="state dict (torch.save) of a GeoFormer of --config")
    ap.add_argument("--config", default="test_geoformer_scannet.yaml")
    ap.add_argument("--labels", action="store_true",
                    help="lift the npz's per-pixel `label` and `instance` images onto the fused points and score the scene")
    ap.add_argument("--label-ignore", type=int, default=None, metavar="V",
                    help='the value of "unannotated" pixels, which do not vote (0 for ScanNet\'s label-filt / instance-filt)')
    ap.add_argument("--min-votes", type=int, default=1, help="pixels an instance label needs on a point")
    ap.add_argument("--min-share", type=float, default=None, help="share of a point's votes its instance label needs")
    ap.add_argument("--track", action="store_true",
                    help="with --chunk-frames: run the model while the frames arrive and keep instance ids over the runs")
    ap.add_argument("--track-every", type=int, default=1, metavar="J", help="run the model after every J-th chunk (and the last)")
    ap.add_argument("--track-iou", type=float, default=0.3, help="frames.Tracker's iou")
    ap.add_argument("--track-max-misses", type=int, default=2, help="frames.Tracker's max_misses")
    ap.add_argument("--carve", action="store_true",
                    help="with --chunk-frames: observe every chunk and drop the cells that later frames look through")
    ap.add_argument("--carve-band", type=float, default=None, metavar="B", help="frames.Carver's band in metres (three cells)")
    ap.add_argument("--carve-drop", type=int, default=-2, metavar="D", help="drop cells whose score is at or below D")
    return ap


def lifted_labels(fused, label, instance, ignore, stride, min_votes=1, min_share=None):
    """(semantic, instance) int32 [n] of frames.lift_scene for images of the depth's shape (read at the stride)."""
    from geoformer_amd import frames

    if tuple(fused.point_of.shape) == tuple(label.shape):
        stride = None
    return frames.lift_scene(fused, label, instance, ignore=ignore, stride=stride, min_votes=min_votes, min_share=min_share)


def fuse_in_chunks(depth, K, pose, color, shift, args, label=None, instance=None, after_chunk=None):
    """(Fused, {"chunk_frames", "adds", "cells", "table_slots", "rehashes"}, voters, keep): the frames through a frames.Fuser,
    --chunk-frames at a time.  Only one chunk's depth and colour are on the device at a time: the arrays stay in host
    memory (as np.load gave them) and are sliced per add.  The Fused is the one frames.fuse would return for all frames
    with origin=the Fuser's, so everything after it is the same.  With label and instance images, each chunk's go
    through two frames.Voter (csrc/frames_vote_stream.hip) beside the Fuser, one chunk of images on the device at a
    time; voters = (the Fuser, the semantic Voter, the instance Voter), what frames.lift_scene_stream takes (else None).
    after_chunk(fu, cells so far, chunk number, last): called after every add (--track).  With --carve a frames.Carver
    observes every chunk after its add; its keep() goes to after_chunk as keep=, restricts the snapshot and is returned
    (what lift_scene_stream takes as keep=; None without --carve)."""
    from geoformer_amd import frames

    F, step = int(depth.shape[0]), int(args.chunk_frames)
    if step < 1:
        raise ValueError(f"--chunk-frames {step} (>= 1)")
    K = np.asarray(K)
    fu = frames.Fuser(args.cell, args.stride, args.near, args.far, args.edge)
    voters = None
    if label is not None:
        voters = (fu, frames.Voter(args.label_ignore), frames.Voter(args.label_ignore))
    cells = []
    carver = frames.Carver(fu, band=args.carve_band, drop=args.carve_drop) if getattr(args, "carve", False) else None
    for a in range(0, F, step):
        b = min(F, a + step)
        part = frames.make(depth[a:b], K if K.ndim == 1 else K[a:b], pose[a:b], None if color is None else color[a:b], shift)
        cells.append(fu.add(part))
        if carver is not None:
            carver.observe(part)
        if voters is not None:
            stride = None if tuple(cells[-1].shape) == tuple(label[a:b].shape) else args.stride
            voters[1].add(cells[-1], label[a:b], stride)
            voters[2].add(cells[-1], instance[a:b], stride)
        if after_chunk is not None:
            after_chunk(fu, cells, len(cells), b == F, **({} if carver is None else {"keep": carver.keep()}))
    stream = {"chunk_frames": step, "adds": len(cells), "cells": fu.cells, "table_slots": fu.slots, "rehashes": fu.rehashes}
    if carver is None:
        return fu.snapshot(args.min_obs, torch.cat(cells)), stream, voters, None
    keep = carver.keep()
    stream["carve"] = {"observed": carver.cells, "dropped": int((~keep).sum()), "band": carver.band,
                       "drop": args.carve_drop}
    return fu.snapshot(args.min_obs, torch.cat(cells), keep=keep), stream, voters, keep


def score(model, name, raw, config_classes=0):
    """{"ap", "ap50", "ap25", "miou", "labelled_points"} of one labelled scene: batch_eval.evaluate and a
    SemanticEvaluator over batch_eval.evaluate_semantic."""
    from geoformer_amd import batch_eval, evaluation

    np.random.seed(0)
    _, avgs = batch_eval.evaluate(model, [(name, raw)], 1, classes=config_classes)
    ev = evaluation.SemanticEvaluator(n_classes=model.cfg.classes, train_fold=model.cfg.train_fold)
    res = batch_eval.evaluate_semantic(model, [(name, raw)], 1, evaluator=ev)
    num = lambda v: None if np.isnan(v) else float(v)  # noqa: E731
    return {"ap": num(avgs["all_ap"]), "ap50": num(avgs["all_ap_50%"]), "ap25": num(avgs["all_ap_25%"]),
            "miou": num(res["miou"]), "labelled_points": int(res["points"])}


def make_model(args, raw, dev):
    """The GeoFormer of --config with --checkpoint's weights, or the benchmark's synthetic model probed with `raw`."""
    import bench
    from geoformer_amd import batch_eval, scene
    from geoformer_amd.model import GeoFormer, load_config

    if args.checkpoint:
        model = GeoFormer(load_config(args.config))
        sd = torch.load(args.checkpoint, map_location="cpu")
        model.load_state_dict(sd.get("state_dict", sd) if isinstance(sd, dict) else sd)
        model.to(dev)
        model.eval()
        return model
    probe = scene.make_batch([batch_eval.scene_dict(raw)])
    return bench.build_model(dev, probe_batch=bench.to_device(probe, dev), cfg_name=args.config)


class Tracking:
    """--track: the model on the snapshot after every J-th chunk and a frames.Tracker updated with its labels."""

    def __init__(self, args, name):
        from geoformer_amd import frames

        self.args, self.name, self.model, self.runs, self.ms, self.keep = args, name, None, 0, 0.0, None
        self.tracker = frames.Tracker(iou=args.track_iou, max_misses=args.track_max_misses)

    def __call__(self, fu, cells, number, last, keep=None):
        from geoformer_amd import batch_eval, frames

        self.fu, self.keep = fu, keep
        if not last and number % self.args.track_every:
            return
        raw, _ = fu.snapshot(self.args.min_obs, torch.cat(cells), keep=keep).raw_scene()
        if raw.shape[0] == 0:
            return
        if self.model is None:
            self.model = make_model(self.args, raw, torch.device("cuda"))
        np.random.seed(0)
        (_, labels), = batch_eval.label_batches(self.model, [(self.name, raw)], 1)
        t = time.perf_counter()
        frames.track_scene(self.tracker, fu, labels, self.args.min_obs, keep=keep)
        torch.cuda.synchronize()
        self.ms += (time.perf_counter() - t) * 1e3
        self.runs += 1

    def frame_outputs(self, fused):
        """frame_outputs with the track id in place of the label id and the owner."""
        from geoformer_amd import frames, render

        ids = self.tracker.labels(self.fu.kept(self.args.min_obs, self.keep))
        return frames.gather(fused, ids, fill=-1), frames.gather(fused, render.instance_colors(ids), fill=255)


def frame_outputs(fused, labels):
    """(ids int32 [F, Hs, Ws], -1 where a pixel has no point; image uint8 [F, Hs, Ws, 3]) of a Fused and its labels."""
    from geoformer_amd import frames, render

    dev = fused.point_of.device
    ids = frames.gather(fused, torch.as_tensor(np.asarray(labels.ids), dtype=torch.int32), fill=-1)
    owner = torch.as_tensor(np.asarray(labels.owner), dtype=torch.int32, device=dev)
    image = frames.gather(fused, render.instance_colors(owner), fill=255)
    return ids, image


def main():
    ap = build_parser()
    args = ap.parse_args()

    import geoformer_amd

    geoformer_amd.configure_runtime()
    from geoformer_amd import batch_eval, export, frames

    if args.track and not args.chunk_frames:
        ap.error("--track needs --chunk-frames")
    if args.carve and not args.chunk_frames:
        ap.error("--carve needs --chunk-frames")
    if args.track_every < 1:
        ap.error(f"--track-every {args.track_every} (>= 1)")
    name = os.path.splitext(os.path.basename(args.frames))[0]
    with np.load(args.frames) as z:
        missing = [k for k in ("depth", "K", "pose") if k not in z.files]
        if missing:
            ap.error(f"{args.frames}: no {', '.join(missing)}")
        depth, K, pose = z["depth"], z["K"], z["pose"]
        color = z["color"] if "color" in z.files else None
        label = instance = None
        if args.labels:
            missing = [k for k in ("label", "instance") if k not in z.files]
            if missing:
                ap.error(f"{args.frames}: --labels, but no {', '.join(missing)}")
            label, instance = z["label"], z["instance"]
    shift = args.depth_shift if args.depth_shift is not None else (1000.0 if depth.dtype == np.uint16 else 1.0)
    try:
        if args.chunk_frames:
            t = time.perf_counter()
            tracking = Tracking(args, name) if args.track else None
            fused, stream, voters, keep = fuse_in_chunks(depth, K, pose, color, shift, args, label, instance, tracking)
        else:
            fr = frames.make(depth, K, pose, color, shift)
            t = time.perf_counter()
            fused = frames.fuse(fr, args.cell, args.stride, args.near, args.far, args.edge, args.min_obs)
        torch.cuda.synchronize()
        fuse_s = time.perf_counter() - t
    except ValueError as e:
        ap.error(str(e))
    n = int(fused.xyz.shape[0])
    if n == 0:
        ap.error("no pixel of the frames is valid: check --near, --far and the depth unit")
    sem = ins = None
    if label is not None:
        try:
            t = time.perf_counter()
            if args.chunk_frames:  # the votes are in: only the snapshot and the scene's tail are left
                sem, ins = frames.lift_scene_stream(*voters, args.min_obs, args.min_votes, args.min_share, keep=keep)
            else:
                sem, ins = lifted_labels(fused, label, instance, args.label_ignore, args.stride, args.min_votes, args.min_share)
            torch.cuda.synchronize()
            lift_s = time.perf_counter() - t
        except ValueError as e:
            ap.error(str(e))
    raw, _ = fused.raw_scene(semantic=sem, instance=ins)
    dev = torch.device("cuda")
    model = tracking.model if args.track and tracking.model is not None else make_model(args, raw, dev)
    np.random.seed(0)
    (_, labels), = batch_eval.label_batches(model, [(name, raw)], 1)
    os.makedirs(os.path.join(args.out, "frames"), exist_ok=True)
    export.write_ply(os.path.join(args.out, f"{name}.ply"), fused.xyz, fused.rgb)
    export.save_labels(os.path.join(args.out, f"{name}.npz"), labels)
    ids, image = frame_outputs(fused, labels) if not args.track else tracking.frame_outputs(fused)
    ids, image = ids.cpu().numpy(), image.cpu().numpy()
    for f in range(ids.shape[0]):
        np.save(os.path.join(args.out, "frames", f"{name}_{f:04d}.npy"), ids[f])
        export.write_png(os.path.join(args.out, "frames", f"{name}_{f:04d}.png"), image[f])
    out = {"frames": int(ids.shape[0]), "sampled_pixels": int(ids.size), "pixels_with_a_point": int((ids >= 0).sum()),
           "fused_points": n, "fuse_ms": round(fuse_s * 1e3, 2), "picked": int(len(labels.table.kept)),
           "kept": int(np.sum(labels.table.kept)), "labelled_points": int((np.asarray(labels.owner) >= 0).sum()),
           "out": args.out}  # (with --track: pixels_with_a_point counts the pixels with a track, fuse_ms includes the model runs)
    if args.track:
        tr = tracking.tracker
        np.savez(os.path.join(args.out, "tracks.npz"), **{f: c.cpu().numpy() for f, c in zip(tr.table()._fields, tr.table())})
        out["track"] = {"runs": tracking.runs, "tracks": tr.tracks, "live": tr.live, "update_ms": round(tracking.ms, 2),
                        "retries": tr.retries, "tracked_pixels": int((ids >= 0).sum())}
    if args.chunk_frames:
        out["stream"] = stream  # (fuse_ms then includes the upload of every chunk)
    if sem is not None:
        np.save(os.path.join(args.out, f"{name}_scene.npy"), raw)  # the fused scene with its lifted labels, [n, 8]
        out["lifted"] = {"lift_ms": round(lift_s * 1e3, 2), "points_with_a_class": int((sem >= 0).sum()),
                         "points_with_an_instance": int((ins >= 0).sum()), "instances": max(int(ins.max()), -1) + 1,
                         **score(model, name, raw)}
        if args.chunk_frames:
            out["voter"] = {"pairs": [v.pairs for v in voters[1:]], "table_slots": [v.slots for v in voters[1:]],
                            "rehashes": sum(v.rehashes for v in voters[1:]), "retries": sum(v.retries for v in voters[1:])}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
