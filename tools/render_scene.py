"""Pictures of a scene and of its predictions, drawn on the GPU without a display: what util/visualize.py shows in a
viewer, as PNG files (geoformer_amd.render, csrc/render.hip).

    python tools/render_scene.py scene0011_00_inst_nostuff.npy                                   # the input colours, 4 views around
    python tools/render_scene.py scene0011_00_inst_nostuff.npy --task semantic_gt --views top
    python tools/render_scene.py scene0011_00_inst_nostuff.npy --task instance_pred --predictions out
    python tools/render_scene.py scene0011_00_inst_nostuff.npy --task semantic_pred --predictions out/semantic --ply

The scene is the [N, 8] array of prepare_data_inst.py (xyz, rgb in [-1, 1], semantic label, instance label).
--predictions DIR is what tools/predict_scenes.py (geoformer_amd.export) wrote for the scene of the same name:
  instance_pred  DIR/<name>.npz (export.load_labels) or, without it, the benchmark files DIR/<name>.txt with
                 DIR/predicted_masks/ (export.read_scannet_predictions): the instances of score >= --min-score (0.09, the
                 viewer's cut) in file order, a later one drawn over an earlier one
  semantic_pred  DIR/<name>.txt of export.write_scannet_semantic: one benchmark label id per point, coloured by id
Output: <out>/<name>_<task>_<view>.png, and with --ply <out>/<name>_<task>.ply, the coloured points for a viewer.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def build_parser():
    from predict_scenes import RENDER_TASKS, parse_size, parse_views

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("scene", help="scene .npy, [N, 8]")
    ap.add_argument("--task", choices=RENDER_TASKS, default="input")
    ap.add_argument("--predictions", default=None, metavar="DIR", help="for the *_pred tasks")
    ap.add_argument("--min-score", type=float, default=None, help="default: postprocess.MIN_SCORE (0.09)")
    ap.add_argument("--views", type=parse_views, default=("turntable", 4), metavar="top|turntable:K")
    ap.add_argument("--elevation", type=float, default=30.0, help="degrees above the horizon of the turntable")
    ap.add_argument("--ortho", action="store_true", help="orthographic turntable views")
    ap.add_argument("--size", type=parse_size, default=(1024, 768), metavar="WxH")
    ap.add_argument("--supersample", type=int, default=2)
    ap.add_argument("--radius", type=int, default=2, help="disc radius in sub-pixels")
    ap.add_argument("--no-shade", action="store_true")
    ap.add_argument("--out", default="render")
    ap.add_argument("--ply", action="store_true", help="also write the coloured points as a PLY file")
    return ap


def predicted_labels(pred_dir, name, n_points, min_score):
    """SceneLabels-like owner of the scene's instance predictions: the .npz when there is one, else the benchmark files."""
    from geoformer_amd import export, postprocess

    npz = os.path.join(pred_dir, f"{name}.npz")
    if os.path.exists(npz):
        return export.load_labels(npz)
    _, scores, masks = export.read_scannet_predictions(pred_dir, name)
    owner = np.full(n_points, -1, np.int32)
    for r in np.nonzero(scores >= np.float32(min_score))[0]:
        if masks[r].shape[0] != n_points:
            raise SystemExit(f"{name}: a mask of {masks[r].shape[0]} points for a scene of {n_points}")
        owner[masks[r] != 0] = r
    return postprocess.SceneLabels(owner, owner, None)


def main():
    ap = build_parser()
    args = ap.parse_args()
    import torch

    import geoformer_amd

    geoformer_amd.configure_runtime()
    from geoformer_amd import export, postprocess, render

    raw = np.load(args.scene)
    if raw.ndim != 2 or raw.shape[1] != 8:
        ap.error(f"{args.scene}: expected [N, 8], got {raw.shape}")
    name = os.path.splitext(os.path.basename(args.scene))[0]
    labels = semantic = None
    if args.task.endswith("_pred"):
        if args.predictions is None:
            ap.error(f"--task {args.task} needs --predictions DIR")
        if args.task == "instance_pred":
            labels = predicted_labels(args.predictions, name, raw.shape[0],
                                      postprocess.MIN_SCORE if args.min_score is None else args.min_score)
        else:
            semantic = export.read_scannet_semantic(args.predictions, name)
            if semantic.shape != (raw.shape[0],):
                ap.error(f"{name}: {semantic.shape[0]} labels for {raw.shape[0]} points")
    dev = torch.device("cuda")
    xyz = torch.as_tensor(raw[:, :3].astype(np.float32), device=dev)
    rgb, ids, keep = render.colors_for(args.task, raw_scene=raw, labels=labels, semantic=semantic, device=dev)
    bounds = render.bounds_of(raw[:, :3])
    if args.views[0] == "top":
        cams = [render.top_down(bounds, args.size)]
    else:
        cams = render.turntable(bounds, args.views[1], args.elevation, args.size, kind="ortho" if args.ortho else "persp")
    image, _ = render.render(xyz, rgb, cams, args.size, supersample=args.supersample, radius=args.radius, ids=ids,
                             keep=keep, shade=None if args.no_shade else render.Shade())
    os.makedirs(args.out, exist_ok=True)
    for v, im in enumerate(image.cpu().numpy()):
        print(export.write_png(os.path.join(args.out, f"{name}_{args.task}_{v}.png"), im))
    if args.ply:
        sel = slice(None) if keep is None else keep.cpu().numpy() != 0
        print(export.write_ply(os.path.join(args.out, f"{name}_{args.task}.ply"), raw[sel, :3], rgb.cpu().numpy()[sel]))


if __name__ == "__main__":
    main()
