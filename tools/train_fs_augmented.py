#!/usr/bin/env python3
"""Cost of few-shot training episodes built on the GPU (geoformer_amd/augment.py train_merge_fs / FSTrainFeeder) at
the FS yaml's batch 8, ~150k points per scene.

    python tools/train_fs_augmented.py [--steps 6] [--warmup 2] [--points 150000] [--batch-size 8] [--scenes 12]

Prints one JSON line:
  episode_gpu_ms.device / .reference: GPU time of one train_merge_fs (8 augmented queries + 8 supports) between two
      events, median over the timed episodes (the reference mode includes its per-scene read-backs and host draws);
  feeder_host_ms: consumer-thread time of one FSTrainFeeder hand-over (next(feeder)), mean over the timed steps;
  step_ms.prebuilt: the few-shot training step (GeoFormerFS forward, FSInstSetCriterion, backward, Adam over the
      42 706 trainable parameters) over K distinct episodes built beforehand by train_merge_fs (rng="device");
  step_ms.feeder: the same loop fed by FSTrainFeeder with the same seed, i.e. the same episodes.
Scenes are resident on the device; every class of fold 0 lists several scenes (each scene carries three of its classes).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import geoformer_amd  # noqa: E402

geoformer_amd.configure_runtime()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--points", type=int, default=150_000)
    ap.add_argument("--batch-size", type=int, default=8)
    ap.add_argument("--scenes", type=int, default=12)
    args = ap.parse_args()
    from geoformer_amd import augment, scene
    from geoformer_amd.model import GeoFormerFS, load_config
    from geoformer_amd.model.criterion_fs import FSInstSetCriterion
    from tests.util import synthetic_state_dict

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    B, K = args.batch_size, args.warmup + args.steps
    fold = augment.FOLD[0]
    raws = {}
    for i in range(args.scenes):
        r = scene.make_raw_scene(int(args.points * (0.8 + 0.4 * ((i * 7) % 11) / 10)), 1200 + i)
        ins = r[:, 7]
        for j, b in enumerate(np.unique(ins[ins >= 0])):
            r[(ins == b) & (r[:, 6] != -100), 6] = fold[(3 * i + j % 3) % len(fold)]
        raws[f"scene{i:04d}_00"] = r
    index = augment.FSIndex.build(raws)
    resident = {k: torch.from_numpy(v).to(dev) for k, v in raws.items()}
    for r in resident.values():
        augment._radius(r)  # (the extents of a resident scene are read once)

    cfg = load_config("geoformer_fs_scannet.yaml", batch_size=B, dec_dropout=0.0)
    torch.manual_seed(0)
    m = GeoFormerFS(cfg)
    m.load_state_dict(synthetic_state_dict(m.state_dict(), 4))
    with torch.no_grad():
        m.semantic_linear.bias[4:] += 1.0  # train fold == cv fold: foreground = classes >= 4
    m.to(dev)
    m.train()
    crit = FSInstSetCriterion(cfg)
    params = [p for p in m.parameters() if p.requires_grad]
    opt = torch.optim.Adam(params, lr=1e-3, fused=True)

    def step(ep):
        sup, q, _ = ep
        np.random.seed(5)
        o = m(sup, q, training=True)
        loss, _ = crit(o, q, 5)
        opt.zero_grad()
        loss.backward()
        opt.step()

    res = {"batch_size": B, "points_per_scene": args.points, "steps": args.steps,
           "trainable_parameters": int(sum(p.numel() for p in params))}
    gpu = {}
    for mode in ("device", "reference"):
        ts = []
        for i in range(K):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            if mode == "device":
                augment.train_merge_fs(resident, index, B, rng="device", seed=1, batch_index=i, device=dev)
            else:
                np.random.seed(i)
                augment.train_merge_fs(resident, index, B, rng="reference", device=dev)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        gpu[mode] = float(np.median(ts[args.warmup:]))
    res["episode_gpu_ms"] = gpu

    prebuilt = [augment.train_merge_fs(resident, index, B, rng="device", seed=7, batch_index=i, device=dev)
                for i in range(K)]
    res["points"] = [int(prebuilt[0][1]["locs"].shape[0]), int(prebuilt[0][0]["locs"].shape[0])]
    torch.cuda.synchronize()
    for i in range(args.warmup):
        step(prebuilt[i])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.warmup, K):
        step(prebuilt[i])
    torch.cuda.synchronize()
    res_prebuilt = (time.perf_counter() - t0) * 1e3 / args.steps
    del prebuilt

    feeder = augment.FSTrainFeeder(resident, index, batch_size=B, seed=7, device=dev)
    host = []
    for i in range(args.warmup):
        step(next(feeder))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        h0 = time.perf_counter()
        ep = next(feeder)
        host.append(time.perf_counter() - h0)
        step(ep)
    torch.cuda.synchronize()
    res_feeder = (time.perf_counter() - t0) * 1e3 / args.steps
    res["feeder_host_ms"] = float(np.mean(host) * 1e3)
    res["step_ms"] = {"prebuilt": res_prebuilt, "feeder": res_feeder}
    res["feeder_over_prebuilt"] = res_feeder / res_prebuilt
    print(json.dumps(res))


if __name__ == "__main__":
    main()
