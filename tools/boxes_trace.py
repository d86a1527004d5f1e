"""One 150k-point scene with ~50 picked instances through the box kernels (csrc/boxes.hip) -- the boxes of the picked
masks and of the ground-truth instances, both kinds, then the IoU block -- next to the numpy statements on the same
input, for a kernel trace:

    rocprofv3 --kernel-trace --stats -d artifacts/boxes -- python tools/boxes_trace.py

Prints the times from device events (median of --reps) and the wall clock of the statements, one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def scene_case(rng, points, instances, proposals):
    """xyz, an instance id per point (-1: none) and `proposals` masks, each a noisy copy of an instance."""
    centres = rng.random((instances, 3)) * np.array([8.0, 8.0, 2.0])
    inst = rng.integers(-1, instances, points)
    xyz = (np.where(inst[:, None] >= 0, centres[np.maximum(inst, 0)], 4.0) + rng.standard_normal((points, 3)) * 0.4)
    of = rng.integers(0, instances, proposals)
    masks = ((inst[None, :] == of[:, None]) & (rng.random((proposals, points)) < 0.85)).astype(np.int32)
    return xyz.astype(np.float32), inst.astype(np.int32), masks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=150_000)
    ap.add_argument("--instances", type=int, default=40)
    ap.add_argument("--proposals", type=int, default=67)  # pick = the first three quarters: 50 masks
    ap.add_argument("--angles", type=int, default=90)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()

    import geoformer_amd

    geoformer_amd.configure_runtime()
    from geoformer_amd import postprocess

    xyz, inst, masks = scene_case(np.random.default_rng(11), args.points, args.instances, args.proposals)
    pick = np.arange(3 * args.proposals // 4, dtype=np.int64)
    d_xyz, d_inst, d_masks, d_pick = [torch.from_numpy(a).cuda() for a in (xyz, inst, masks, pick)]
    specs = [("rows", d_masks, d_pick, d_xyz), ("ids", d_inst, args.instances, d_xyz)]
    P = pick.shape[0]
    out = {"points": args.points, "picked": int(P), "instances": args.instances, "angles": args.angles}
    for kind, A in (("aligned", 1), ("oriented", args.angles)):
        box, iou = [], []
        for i in range(args.reps + 3):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record()
            _, count, aligned, oriented = postprocess._boxes_packed(specs, A)
            e[1].record()
            rows = oriented if kind == "oriented" else aligned
            block = postprocess.box_iou_batched([rows[:P]], [rows[P:]])[0]
            e[2].record()
            torch.cuda.synchronize()
            if i >= 3:
                box.append(e[0].elapsed_time(e[1]) * 1e3), iou.append(e[1].elapsed_time(e[2]) * 1e3)
        t = time.perf_counter()
        hp = postprocess.instance_boxes_host(masks, pick, xyz, A)
        hg = postprocess.id_boxes_host(inst, args.instances, xyz, A)
        t1 = time.perf_counter()
        k = 2 if kind == "oriented" else 1
        hi = postprocess.box_iou_host(hp[k], hg[k])
        t2 = time.perf_counter()
        same = bool(np.array_equal(block.cpu().numpy(), hi) and np.array_equal(rows.cpu().numpy(), np.concatenate([hp[k], hg[k]])))
        med = lambda v: round(float(np.median(v)), 1)  # noqa: E731
        out[kind] = {"boxes_us_events": med(box), "iou_us_events": med(iou), "boxes_numpy_us": round((t1 - t) * 1e6, 1),
                     "iou_numpy_us": round((t2 - t1) * 1e6, 1), "equal_to_numpy": same}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
