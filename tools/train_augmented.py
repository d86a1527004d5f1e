#!/usr/bin/env python3
"""Cost of freshly augmented training batches (geoformer_amd/augment.py) at batch 4, ~150k points per scene.

    python tools/train_augmented.py [--steps 8] [--warmup 2] [--points 150000] [--batch-size 4]

Prints one JSON line:
  merge_gpu_ms.device / .reference: GPU time of one train_merge per batch between two events (the reference mode
      includes its per-scene read-backs and host draws);
  feeder_host_ms: consumer-thread time of one TrainFeeder hand-over (next(feeder)), mean over the timed steps;
  step_ms.distinct: training step (forward, criterion, backward, Adam) over K pre-built DISTINCT batches (host-collated
      by scene.make_batch, resident on the device: fresh sizes every step, no augmentation);
  step_ms.feeder: the same loop fed by TrainFeeder (rng="device", scenes resident on the device).
Both loops use the same model, the same scenes and the same sizes before augmentation.
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
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--points", type=int, default=150_000)
    ap.add_argument("--batch-size", type=int, default=4)
    args = ap.parse_args()
    from geoformer_amd import augment, scene
    from geoformer_amd.model import GeoFormer, InstSetCriterion, load_config
    from tests.util import synthetic_state_dict

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    B, K = args.batch_size, args.warmup + args.steps
    cfg = load_config("geoformer_scannet.yaml", batch_size=B, dec_dropout=0.0, prepare_epochs=1)
    torch.manual_seed(0)
    m = GeoFormer(cfg)
    m.load_state_dict(synthetic_state_dict(m.state_dict(), 1))
    m.to(dev)
    m.train()
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    crit = InstSetCriterion(cfg)
    opt = torch.optim.Adam(m.parameters(), lr=1e-4)

    n_scenes = B * K
    raws = [scene.make_raw_scene(int(args.points * (0.8 + 0.4 * ((i * 7) % 11) / 10)), 900 + i) for i in range(n_scenes)]
    resident = [torch.from_numpy(r).to(dev) for r in raws]
    for r in resident:
        augment._radius(r)  # (the extents of a resident scene are read once)

    def step(batch):
        np.random.seed(3)
        out = m(batch, 1)
        loss, _ = crit(out, batch, 1)
        opt.zero_grad()
        loss.backward()
        opt.step()
        return loss

    # GPU time of train_merge per batch, both modes
    res = {"batch_size": B, "points_per_scene": args.points, "steps": args.steps}
    merge = {}
    for mode in ("device", "reference"):
        ts = []
        for i in range(K):
            sc = resident[i * B:(i + 1) * B]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            if mode == "device":
                augment.train_merge(sc, rng="device", seed=1, batch_index=i, device=dev)
            else:
                np.random.seed(i)
                augment.train_merge(sc, rng="reference", device=dev)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        merge[mode] = float(np.median(ts[args.warmup:]))
    res["merge_gpu_ms"] = merge

    # loop over K distinct pre-built batches (no augmentation)
    def to_dev(b):
        return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in b.items()}

    distinct = []
    for i in range(K):
        sc = []
        for r in raws[i * B:(i + 1) * B]:
            sc.append({"xyz": r[:, :3].astype(np.float32), "rgb": r[:, 3:6].astype(np.float32),
                       "label": np.where(r[:, 6] > 1, 4, np.maximum(r[:, 6], 0)).astype(np.int64),
                       "instance": r[:, 7].astype(np.int64)})
        distinct.append(to_dev(scene.make_batch(sc)))
    torch.cuda.synchronize()
    for i in range(args.warmup):
        step(distinct[i])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.warmup, K):
        step(distinct[i])
    torch.cuda.synchronize()
    res_distinct = (time.perf_counter() - t0) * 1e3 / args.steps
    del distinct

    # the same loop fed by TrainFeeder
    feeder = augment.TrainFeeder(resident, batch_size=B, seed=7, device=dev)
    host = []
    for i in range(args.warmup):
        step(next(feeder))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        h0 = time.perf_counter()
        b = next(feeder)
        host.append(time.perf_counter() - h0)
        step(b)
    torch.cuda.synchronize()
    res_feeder = (time.perf_counter() - t0) * 1e3 / args.steps
    res["feeder_host_ms"] = float(np.mean(host) * 1e3)
    res["step_ms"] = {"distinct": res_distinct, "feeder": res_feeder}
    res["feeder_over_distinct"] = res_feeder / res_distinct
    print(json.dumps(res))


if __name__ == "__main__":
    main()
