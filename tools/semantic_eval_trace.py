"""The semantic evaluation's kernel beside the framework statement of the same work, for a kernel trace:

    rocprofv3 --kernel-trace --stats --memory-copy-trace -d artifacts/semantic -- python tools/semantic_eval_trace.py --what kernel
    rocprofv3 --kernel-trace --stats -d artifacts/semantic_torch -- python tools/semantic_eval_trace.py --what torch
    python tools/semantic_eval_trace.py --what loops --scenes 8                 # scenes/s of the loops, profiler off

--what kernel: --reps calls of pointops.semantic_confusion on one scene's scores [N, C] and raw labels (one launch each;
k_semantic_confusion in the stats), then --reps SemanticEvaluator.add_batch calls between two marks the memory-copy
trace can be read against: none of them may be followed by a device-to-host copy.
--what torch: the same tensors through scores.max(1)[1], the table look-up, and bincount of row * C + pred (every kernel
of the stats but the fills of the set-up belongs to it).
--what loops: batch_eval.evaluate at --batch-size with and without semantic=, and batch_eval.semantic_batches, on
--scenes synthetic 150k-point scenes with the benchmark's model; wall clock of whole passes, host collate included.
Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=("kernel", "torch", "loops"), default="kernel")
    ap.add_argument("--points", type=int, default=150_269)
    ap.add_argument("--classes", type=int, default=13)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--scenes", type=int, default=8)
    ap.add_argument("--batch-size", type=int, default=4)
    args = ap.parse_args()

    import geoformer_amd

    geoformer_amd.configure_runtime()
    from geoformer_amd import batch_eval, evaluation, pointops, scene

    N, C = args.points, args.classes
    out = {"what": args.what, "points": N, "classes": C}
    if args.what in ("kernel", "torch"):
        rng = np.random.default_rng(1)
        scores = torch.from_numpy(rng.standard_normal((N, C)).astype(np.float32)).cuda()
        raw = np.array([-100] + list(range(20)), np.int64)[rng.integers(0, 21, N)]
        labels = torch.from_numpy(raw).cuda()
        lut_h, mi, mo = evaluation.semantic_label_lut(0)
        offsets = torch.tensor([0, N], dtype=torch.int32).cuda()
        want = evaluation.semantic_confusion_host(scores.cpu().numpy(), raw, None, lut=lut_h, map_ignore=mi, map_other=mo)[1][0]
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if args.what == "kernel":
        lut = torch.from_numpy(lut_h).cuda()
        conf = torch.zeros((1, C + 1, C), dtype=torch.int64, device="cuda")
        for i in range(args.reps + 5):
            if i == 5:
                torch.cuda.synchronize()
                conf.zero_()
                ev0.record()
            pointops.semantic_confusion(scores, labels, offsets, conf, lut=lut, map_ignore=mi, map_other=mo)
        ev1.record()
        torch.cuda.synchronize()
        assert (conf[0].cpu().numpy() == args.reps * want).all()
        out["call_us_events"] = round(ev0.elapsed_time(ev1) * 1e3 / args.reps, 2)  # back-to-back calls, host included
        ev = evaluation.SemanticEvaluator(n_classes=C, train_fold=0)
        ev.add_batch(scores, labels, offsets, ["warm"])
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")  # a synchronising call (a read-back is one) raises from here on
        for i in range(args.reps):
            ev.add_batch(scores, labels, offsets, [f"s{i}"])
        torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        assert (ev.confusion() == (args.reps + 1) * want).all()
        out["add_batch_calls_without_a_synchronising_call"] = args.reps
    elif args.what == "torch":
        table = torch.full((121,), mo, dtype=torch.int64, device="cuda")  # index = label + 100: -100 -> 0
        table[100:120] = torch.from_numpy(lut_h).cuda().long()
        table[0] = mi
        for i in range(args.reps + 5):
            if i == 5:
                torch.cuda.synchronize()
                ev0.record()
            pred = scores.max(1)[1]
            row = table[labels + 100]
            conf = torch.bincount(row * C + pred, minlength=(C + 1) * C)
        ev1.record()
        torch.cuda.synchronize()
        assert (conf.view(C + 1, C).cpu().numpy() == want).all()
        out["call_us_events"] = round(ev0.elapsed_time(ev1) * 1e3 / args.reps, 2)
    else:
        import bench

        items = [(f"synthetic{i:04d}", scene.make_raw_scene(args.points, 500 + i)) for i in range(args.scenes)]
        dev = torch.device("cuda")
        probe = scene.make_batch([batch_eval.scene_dict(items[0][1])])
        model = bench.build_model(dev, probe_batch=bench.to_device(probe, dev), cfg_name="test_geoformer_scannet.yaml")
        new = lambda: evaluation.SemanticEvaluator(n_classes=model.cfg.classes, train_fold=model.cfg.train_fold)  # noqa: E731

        def timed(fn):
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return round(len(items) / (time.perf_counter() - t), 2)

        legs = {"evaluate": lambda: batch_eval.evaluate(model, items, args.batch_size, final_score_thresh=0.0),
                "evaluate_semantic=": lambda: batch_eval.evaluate(model, items, args.batch_size, final_score_thresh=0.0,
                                                                  semantic=new()),
                "semantic_batches": lambda: batch_eval.evaluate_semantic(model, items, args.batch_size)}
        rates = {k: [] for k in legs}
        for rep in range(4):  # (alternating; the first round warms every shape and is dropped)
            for k, fn in legs.items():
                np.random.seed(0)
                r = timed(fn)
                if rep:
                    rates[k].append(r)
        out.update({"scenes": len(items), "batch_size": args.batch_size, "scenes_per_s": rates})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
