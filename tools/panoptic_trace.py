"""The panoptic kernel family beside the framework statement of the same table, for a kernel trace:

    rocprofv3 --kernel-trace --stats -d artifacts/panoptic -- python tools/panoptic_trace.py --what kernel
    rocprofv3 --kernel-trace --stats -d artifacts/panoptic_torch -- python tools/panoptic_trace.py --what torch

One scene of --points points with --picks picked instances and about --segments ground-truth segments, laid out in
spatially coherent runs as a scene's labels are.
--what kernel: --reps calls of pointops.panoptic_overlaps_packed (the presence memset, k_pan_keys, k_pan_slots and
k_pan_count in the stats; nothing is read back between the calls).  --lds-bins 0 takes the global-atomic regime.
--what torch: the same tensors through torch.unique on the keys (sorted, with the inverse) and bincount of
row * (G + 1) + col (every kernel of the stats but the fills of the set-up belongs to it).
Both check their table against evaluation.panoptic_overlaps_host once and print one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=("kernel", "torch"), default="kernel")
    ap.add_argument("--points", type=int, default=150_269)
    ap.add_argument("--picks", type=int, default=51)
    ap.add_argument("--segments", type=int, default=60)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--lds-bins", type=int, default=-1)
    args = ap.parse_args()

    import geoformer_amd

    geoformer_amd.configure_runtime()
    from geoformer_amd import _lib, evaluation, pointops

    N, P = args.points, args.picks
    ev = evaluation.PanopticEvaluator(classes=0)
    things = ev.class_ids[~ev.is_stuff]
    rng = np.random.default_rng(1)
    run = lambda values: np.repeat(values, 97)[:N]  # noqa: E731  (runs of 97 points share a label)
    k = -(-N // 97)
    owner = run(rng.integers(-1, P, k)).astype(np.int32)
    sem = run(rng.integers(0, 13, k)).astype(np.int32)
    pool = np.concatenate([[0, 1001, 2001], (things[rng.integers(0, len(things), args.segments - 2)] * 1000
                                             + np.arange(1, args.segments - 1))])
    gt = run(pool[rng.integers(0, len(pool), k)]).astype(np.int64)
    ids = np.where(owner >= 0, things[np.maximum(owner, 0) % len(things)] * 1000 + owner + 1, 0).astype(np.int32)
    _, Gs, gt_id, want = evaluation.panoptic_overlaps_host(owner, sem, gt, class_ids=ev.class_ids, is_stuff=ev.is_stuff,
                                                           stuff_of_sem=ev.stuff_of_sem, P=P)
    G, R = int(Gs[0]), P + ev.n_stuff + 1
    out = {"what": args.what, "points": N, "picks": P, "segments": G, "bins": R * (G + 1)}
    d = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    owner_d, ids_d, sem_d, gt_d = d(owner), d(ids), d(sem), d(gt)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if args.what == "kernel":
        _lib.check(_lib.load().gf_dev_panoptic_lds_bins(args.lds_bins), "gf_dev_panoptic_lds_bins")
        cls, st, sos = ev.device_tables(torch.device("cuda", torch.cuda.current_device()))
        off = torch.tensor([0, N], dtype=torch.int32).cuda()
        for i in range(args.reps + 5):
            if i == 5:
                torch.cuda.synchronize()
                ev0.record()
            _, buf, lay = pointops.panoptic_overlaps_packed(owner_d, ids_d, sem_d, gt_d, off, cls, st, sos, ev.n_stuff, P,
                                                            max_gt=256)
        ev1.record()
        torch.cuda.synchronize()
        g, gid, inter = pointops.panoptic_unpack(buf.cpu().numpy(), lay, 1, R, 256)
        assert int(g[0]) == G and (gid[0, :G] == gt_id[0]).all()
        assert (inter[0, :, :G] == want[0, :, :G]).all() and (inter[0, :, 256] == want[0, :, G]).all()
        out["lds_bins"] = args.lds_bins
    else:
        # rows and keys as the kernel defines them, prepared once: the timed part is the table alone
        st_of = torch.full((13,), -1, dtype=torch.int64, device="cuda")
        st_of[0], st_of[1] = 0, 1
        srow = st_of[sem_d.long()]
        row = torch.where(owner_d >= 0, owner_d.long(), torch.where(srow >= 0, P + srow, R - 1))
        q = gt_d // 1000
        cls_sorted = torch.from_numpy(np.sort(ev.class_ids)).cuda()
        pos = torch.searchsorted(cls_sorted, q).clamp(max=len(cls_sorted) - 1)
        valid = cls_sorted[pos] == q
        stuff_q = (q == 1) | (q == 2)
        key = torch.where(valid, pos * 1000 + torch.where(stuff_q, 0, gt_d - q * 1000), 64000)  # void sorts last
        for i in range(args.reps + 5):
            if i == 5:
                torch.cuda.synchronize()
                ev0.record()
            uniq, col = torch.unique(key, sorted=True, return_inverse=True)
            table = torch.bincount(row * uniq.shape[0] + col, minlength=R * uniq.shape[0])
        ev1.record()
        torch.cuda.synchronize()
        assert uniq.shape[0] == G + 1 and (table.view(R, G + 1).cpu().numpy() == want[0]).all()
    out["call_us_events"] = round(ev0.elapsed_time(ev1) * 1e3 / args.reps, 2)  # back-to-back calls, host included
    print(json.dumps(out))


if __name__ == "__main__":
    main()
