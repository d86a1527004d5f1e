"""Posed depth frames of a synthetic room through csrc/frames.hip -- back-projection, the grid of cells, the cell means,
the pixel-to-point map -- next to the numpy statement on the same input, for a kernel trace:

    python tools/frames_trace.py                                   # 64 frames of 640 x 480, stride 1, 2 cm cells
    rocprofv3 --kernel-trace --stats -d artifacts/frames -- python tools/frames_trace.py --no-host

The depth images are ray casts of the inside of a 6 x 5 x 3 m room from cameras on a circle (uint16 millimetres, with
colours).  Prints one JSON line: the time of every entry point from device events (median of --reps, buffers allocated
ahead), the cell sums with and without the aggregation of equal cells among adjacent lanes, the whole frames.fuse (wall
clock, the uploads of the frames not included), the numpy statement frames.fuse_host (wall clock) and whether the two
agree bit for bit, and the share of the HBM peak the back-projection reaches on its algorithmic bytes (depth and colour
read; points, colours and the two maps written).  Under "vote": gf_frames_vote (csrc/frames_vote.hip) lifting a label
image -- the 1 m block every pixel's own point lies in -- onto the fused points, as uint8, uint16 and int32, at the
default and at the proven table size, with and without the aggregation of equal pairs among adjacent lanes; the numpy
statement frames.vote_host on the same input and whether the two agree; the share of the HBM peak on point_of's 4 bytes
plus the label's 1, 2 or 4 per pixel.

    python tools/frames_trace.py --no-host --stream 8               # ... and the same frames 8 at a time

Under "stream_vote" (with --stream K): frames.Voter (csrc/frames_vote_stream.hip) fed the label image K frames per add
beside the Fuser, next to one gf_frames_vote over everything; see voter_leg.
Under "stream" (with --stream K): frames.Fuser (csrc/frames_stream.hip) fed K frames per add, next to the one-shot
frames.fuse on the same input in the same process; see stream_leg.

    python tools/frames_trace.py --no-host --track 8                # ... and a tracker updated after every 8 frames

Under "track" (with --track K): frames.Tracker (csrc/frames_track.hip) updated on the Fuser's snapshot after every chunk of
K frames, with synthetic owners (the 50 blocks of 1.2 x 1 x 1.5 m a point lies in); see track_leg.

    python tools/frames_trace.py --no-host --carve 8 --carve-host   # ... and a carver that observes every 8 frames

Under "carve" (with --carve K): frames.Carver (csrc/frames_carve.hip) observing every chunk of K frames after the Fuser
added it, in both launch shapes; see carve_leg.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12  # bytes per second, MI355X (specification)


def room_frames(F, W, H, seed=0):
    """(depth uint16 [F, H, W] in millimetres, color uint8 [F, H, W, 3], K [4], pose [F, 4, 4]): the inside of the box
    [0, 6] x [0, 5] x [0, 3] m seen from F cameras on a circle of 1 m around its centre, each looking outwards and a
    little down; the depth of a pixel is the camera-z of its ray's exit from the box."""
    from geoformer_amd import render

    lo, hi = np.zeros(3), np.array([6.0, 5.0, 3.0])
    f = 0.9 * W
    K = np.array([f, f, W / 2.0, H / 2.0])
    i, j = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    rays = np.stack([(i - K[2]) / f, (j - K[3]) / f, np.ones_like(i)], axis=-1)  # camera z = 1: t is the depth
    depth = np.empty((F, H, W), np.uint16)
    color = np.empty((F, H, W, 3), np.uint8)
    pose = np.tile(np.eye(4), (F, 1, 1))
    rng = np.random.default_rng(seed)
    for k in range(F):
        az = 2 * np.pi * k / F
        eye = (lo + hi) / 2 + np.array([np.cos(az), np.sin(az), 0.2 * np.sin(3 * az)])
        R = render.look_at(eye, eye + np.array([np.cos(az), np.sin(az), -0.25]))
        pose[k, :3, :3], pose[k, :3, 3] = R.T, eye
        d = rays @ R  # world directions
        with np.errstate(divide="ignore"):
            t = np.where(d > 0, (hi - eye) / d, np.where(d < 0, (lo - eye) / d, np.inf)).min(-1)
        depth[k] = np.rint((t + rng.standard_normal(t.shape) * 0.002) * 1000).astype(np.uint16)
        p = eye + d * t[..., None]
        color[k] = (np.floor(p * 4).astype(np.int64) * np.array([37, 91, 53]) % 200 + 40).astype(np.uint8)
    return depth, color, K, pose


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--size", default="640x480")
    ap.add_argument("--stride", type=int, default=1)
    ap.add_argument("--cell", type=float, default=0.02)
    ap.add_argument("--edge", type=float, default=None)
    ap.add_argument("--min-obs", type=int, default=1)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-host", action="store_true", help="skip the numpy statement (minutes at the default size)")
    ap.add_argument("--stream", type=int, default=0, metavar="K",
                    help="also run the frames K at a time through frames.Fuser (K divides --frames); see stream_leg")
    ap.add_argument("--stream-no-host", action="store_true", help="with --stream: skip frames.VoterHost on the host")
    ap.add_argument("--track", type=int, default=0, metavar="K",
                    help="also update a frames.Tracker on the snapshot after every K frames (K divides --frames); see track_leg")
    ap.add_argument("--track-host", action="store_true", help="with --track and --no-host: run frames.TrackerHost all the same")
    ap.add_argument("--carve", type=int, default=0, metavar="K",
                    help="also observe every K frames with a frames.Carver after the Fuser added them (K divides --frames); see carve_leg")
    ap.add_argument("--carve-host", action="store_true", help="with --carve and --no-host: run frames.CarverHost all the same")
    args = ap.parse_args()
    W, H = (int(v) for v in args.size.lower().split("x"))

    import geoformer_amd

    geoformer_amd.configure_runtime()
    from geoformer_amd import _lib, frames, pointops
    from geoformer_amd._lib import check, ptr, stream_ptr

    depth, color, K, pose = room_frames(args.frames, W, H)
    fr = frames.make(depth, K, pose, color)
    dfr = fr._replace(depth=fr.depth.cuda(), color=fr.color.cuda())
    lib = _lib.load()
    dev = torch.device("cuda")
    F, s = args.frames, args.stride
    Hs, Ws = -(-H // s), -(-W // s)
    T = F * Hs * Ws
    edge = 0.0 if args.edge is None else args.edge
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)  # noqa: E731
    table = torch.from_numpy(fr.table).cuda()
    xyz, rgb = torch.empty((T, 3), dtype=torch.float32, device=dev), torch.empty((T, 3), dtype=torch.uint8, device=dev)
    pixel_of, point_of, words = i32(T), i32(T), i32(2)
    lo = torch.empty(3, dtype=torch.float32, device=dev)
    ws = torch.empty(lib.gf_frames_backproject_scratch_bytes(T, 0) // 8 + 1, dtype=torch.int64, device=dev)

    def backproject():
        check(lib.gf_frames_backproject(ptr(dfr.depth), 0, fr.depth_shift, ptr(dfr.color), ptr(table), F, W, H, s, 0.1, 10.0,
                                        edge, 0, ptr(ws), ptr(xyz), ptr(rgb), ptr(pixel_of), ptr(point_of), ptr(lo), ptr(words),
                                        stream_ptr()), "gf_frames_backproject")

    backproject()
    n = int(words[0])
    pts, cols = xyz[:n], rgb[:n]
    org = lo.clone()
    assert torch.equal(org, pts.amin(0))
    _, cell_of, count = pointops.grid_subsample(pts, args.cell, mode="first", origin=org)
    cell_of, count = cell_of.contiguous(), count.contiguous()
    M = int(count.shape[0])
    g_out, g_words = i32(3, n), i32(2)
    g_ws = torch.empty(lib.gf_grid_subsample_scratch_bytes(n) // 8 + 1, dtype=torch.int64, device=dev)
    m_xyz, m_rgb = torch.empty((M, 3), dtype=torch.float32, device=dev), torch.empty((M, 3), dtype=torch.uint8, device=dev)
    m_out, m_words = i32(2, M), i32(2)
    m_ws = torch.empty(lib.gf_frames_cell_means_scratch_bytes(M, 0) // 8 + 1, dtype=torch.int64, device=dev)
    composed = i32(T)

    def cells():
        check(lib.gf_grid_subsample(ptr(pts), n, args.cell, 0, ptr(org), ptr(g_ws), ptr(g_out[0]), ptr(g_out[1]),
                                    ptr(g_out[2]), ptr(g_words), stream_ptr()), "gf_grid_subsample")

    def means(aggregate):
        check(lib.gf_frames_cell_means(ptr(pts), ptr(cols), ptr(cell_of), ptr(count), n, M, ptr(org), args.min_obs, aggregate,
                                       0, ptr(m_ws), ptr(m_xyz), ptr(m_rgb), ptr(m_out[0]), ptr(m_out[1]), ptr(m_words),
                                       stream_ptr()), "gf_frames_cell_means")

    def compose():
        composed.copy_(point_of)
        check(lib.gf_frames_compose(ptr(composed), T, ptr(cell_of), ptr(m_out[1]), stream_ptr()), "gf_frames_compose")

    def timed(fn):
        us = []
        for i in range(args.reps + 2):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if i >= 2:
                us.append(a.elapsed_time(b) * 1e3)
        return round(float(np.median(us)), 1)

    stages = {"backproject_us": timed(backproject), "grid_subsample_us": timed(cells), "cell_means_aggregated_us": timed(lambda: means(1)),
              "cell_means_plain_us": timed(lambda: means(0)), "compose_with_copy_us": timed(compose),
              "copy_alone_us": timed(lambda: composed.copy_(point_of))}
    m = int(m_words[0])
    moved = T * (2 + 3 + 4) + n * (12 + 3 + 4)  # depth, colour, point_of; xyz, rgb, pixel_of
    wall = []
    for _ in range(5):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fused = frames.fuse(dfr, args.cell, s, 0.1, 10.0, args.edge, args.min_obs)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t) * 1e3)
    out = {"frames": F, "size": [W, H], "stride": s, "cell": args.cell, "edge": args.edge, "min_obs": args.min_obs,
           "sampled_pixels": T, "valid_pixels": n, "cells": M, "fused_points": m, **stages,
           "backproject_bytes": moved, "backproject_share_of_hbm_peak": round(moved / (stages["backproject_us"] * 1e-6) / HBM_PEAK, 3),
           "fuse_ms_wall": round(float(np.median(wall)), 2), "aggregate_default": frames.AGGREGATE}
    if not args.no_host:
        t = time.perf_counter()
        want = frames.fuse_host(fr, args.cell, s, 0.1, 10.0, args.edge, args.min_obs)
        out["fuse_host_numpy_ms"] = round((time.perf_counter() - t) * 1e3, 1)
        out["equal_to_numpy"] = all(torch.equal(a.cpu(), b) for a, b in zip(fused, want))

    # ---- the vote (csrc/frames_vote.hip): a label image lifted onto the fused points ------------------------------------
    # the label of a pixel is the 1 m block its OWN back-projected point lies in (1 .. 90; 0 without a point), so the
    # pixels of a fused point next to a block's face disagree, as the pixels at a segment's border do
    group = fused.point_of.reshape(-1).contiguous()
    own = pts[point_of.clamp(min=0).long()].floor().clamp(min=0).to(torch.int32)
    block = torch.where(point_of >= 0, 1 + own[:, 0].clamp(max=5) + 6 * own[:, 1].clamp(max=4) + 30 * own[:, 2].clamp(max=2),
                        torch.zeros_like(point_of))
    del own
    default, proven = frames.vote_slots(T, m)
    v_out, v_words = i32(3, m), i32(3)
    v_ws = torch.empty(lib.gf_frames_vote_scratch_bytes(proven, m) // 8 + 1, dtype=torch.int64, device=dev)
    vote = {"vote_groups": m, "vote_slots_default": default, "vote_slots_proven": proven,
            "vote_aggregate_default": frames.VOTE_AGGREGATE}
    for name, dt, kind in (("u8", torch.uint8, 0), ("u16", torch.uint16, 1), ("i32", torch.int32, 2)):
        image = block.to(dt).contiguous()

        def run(slots, aggregate):
            check(lib.gf_frames_vote(ptr(group), ptr(image), kind, 1, T, 1, 1, m, 0, 1, -100, slots, aggregate, ptr(v_ws),
                                     ptr(v_out[0]), ptr(v_out[1]), ptr(v_out[2]), ptr(v_words), stream_ptr()), "gf_frames_vote")

        us = {"default_aggregated": timed(lambda: run(default, 1)), "default_plain": timed(lambda: run(default, 0)),
              "proven_aggregated": timed(lambda: run(proven, 1)), "proven_plain": timed(lambda: run(proven, 0))}
        run(default, 1)
        pairs, overflow, beyond = v_words.tolist()
        nbytes = T * (4 + image.element_size())
        vote[name] = {**{f"vote_{k}_us": v for k, v in us.items()}, "pairs": pairs, "overflow": overflow, "bytes": nbytes,
                      "share_of_hbm_peak": round(nbytes / (us["default_aggregated"] * 1e-6) / HBM_PEAK, 3)}
        if not args.no_host and name == "u8":
            t = time.perf_counter()
            want, want_pairs = frames.vote_host(group.cpu(), image.cpu(), m, 0)
            vote["vote_host_numpy_ms"] = round((time.perf_counter() - t) * 1e3, 1)
            vote["vote_equal_to_numpy"] = bool(all(torch.equal(a.cpu(), b) for a, b in zip(v_out, want)) and pairs == want_pairs)
    out["vote"] = vote
    if args.stream:
        out["stream"] = stream_leg(args, fr, dfr, timed)
        labels = block.to(torch.uint8).reshape(F, Hs, Ws).contiguous()
        del block, group
        out["stream_vote"] = voter_leg(args, fr, dfr, labels, timed)
    if args.track:
        out["track"] = track_leg(args, dfr, timed)
    if args.carve:
        out["carve"] = carve_leg(args, fr, dfr, timed)
    print(json.dumps(out))


def carve_leg(args, fr, dfr, timed):
    """frames.Carver (csrc/frames_carve.hip) beside a Fuser fed --carve K frames at a time: after every add both launch
    shapes observe the chunk (a carver each).  Reported: the device time of every observe from events (the snapshot and its
    read-back included); gf_frames_visibility alone with the state update on the last chunk and the whole map, median of
    --reps after a warm-up, per launch shape; Fuser.snapshot over every cell so far with and without keep=; the kept
    shape's time against the least its algorithmic bytes allow at the HBM peak (the points, 12 bytes; the state read and
    written and the three counts written, 36 bytes per cell; one depth value per probe that reaches the depth read);
    FuserHost + CarverHost on the same chunks (wall clock of every observe) and whether state and keep agree."""
    from geoformer_amd import _lib, frames
    from geoformer_amd._lib import check, ptr, stream_ptr

    lib = _lib.load()
    F, K = args.frames, args.carve
    if K < 1 or F % K:
        raise SystemExit(f"--carve {K}: a divisor of --frames {F}")
    dev = dfr.depth.device
    cut = lambda f, a, b: f._replace(depth=f.depth[a:b], color=f.color[a:b], table=f.table[a:b])  # noqa: E731
    kw = dict(cell=args.cell, stride=args.stride, near=0.1, far=10.0, edge=args.edge)
    fu = frames.Fuser(**kw)
    carvers = {v: frames.Carver(fu, variant=v) for v in (0, 1)}
    per, cells = {0: [], 1: []}, []
    for a in range(0, F, K):
        part = cut(dfr, a, a + K)
        cells.append(fu.add(part))
        for v, c in carvers.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            c.observe(part)
            e1.record()
            torch.cuda.synchronize()
            per[v].append(round(e0.elapsed_time(e1) * 1e3, 1))
    ca = carvers[0]
    keep = ca.keep()
    same = all(torch.equal(x, y) for x, y in zip((ca._seen[:ca.cells], ca._free[:ca.cells], ca._score[:ca.cells]),
                                                 (carvers[1]._seen[:ca.cells], carvers[1]._free[:ca.cells], carvers[1]._score[:ca.cells])))
    M = fu.cells
    res = {"chunk_frames": K, "variant_default": frames.CARVE_VARIANT, "cells": M, "dropped": int((~keep).sum()),
           "band": ca.band, "observe_with_snapshot_us_per_point": per[0], "observe_with_snapshot_us_per_probe": per[1],
           "shapes_agree": bool(same)}
    # the library call alone: the last chunk against the whole map, the state updated in place on copies
    xyz = fu.snapshot(1).xyz.contiguous()
    inv = torch.from_numpy(frames.inverse_records(part)).to(dev)
    table = torch.from_numpy(part.table).to(dev)
    near, far, e, band, rel = (float(v) for v in ca._probe)
    state = torch.stack([ca._seen[:M], ca._free[:M], ca._score[:M]]).contiguous()
    out = torch.empty((3, M), dtype=torch.int32, device=dev)
    codes = torch.empty((K, M), dtype=torch.uint8, device=dev)
    H, W = part.depth.shape[1:]

    def run(variant, with_codes=False):
        check(lib.gf_frames_visibility(ptr(xyz), M, ptr(part.depth), int(part.depth.dtype == torch.float32), K, H, W,
                                       part.depth_shift, ptr(table), ptr(inv), near, far, e, band, rel, ptr(out),
                                       ptr(codes) if with_codes else None, ptr(state[0]), ptr(state[1]), ptr(state[2]),
                                       *ca._rule, variant, stream_ptr()), "gf_frames_visibility")

    res["visibility_us_per_point"], res["visibility_us_per_probe"] = timed(lambda: run(0)), timed(lambda: run(1))
    res["visibility_us_per_point_again"] = timed(lambda: run(0))
    run(0, True)
    classes = torch.bincount(codes.reshape(-1).long(), minlength=5).tolist()
    reads = sum(classes[1:])  # the probes that read a depth value
    nbytes = M * (12 + 36) + reads * part.depth.element_size()
    best = min(res["visibility_us_per_point"], res["visibility_us_per_probe"])
    res.update(probes=K * M, classes=classes, bytes=nbytes, least_us_at_hbm_peak=round(nbytes / HBM_PEAK * 1e6, 2),
               share_of_hbm_peak=round(nbytes / (best * 1e-6) / HBM_PEAK, 4))
    every = torch.cat(cells)
    res["snapshot_us"] = timed(lambda: fu.snapshot(1, every))
    res["snapshot_keep_us"] = timed(lambda: fu.snapshot(1, every, keep=keep))
    if args.carve_host or not args.no_host:
        fh = frames.FuserHost(**kw)
        ch, host_ms = frames.CarverHost(fh), []
        for a in range(0, F, K):
            part = cut(fr, a, a + K)
            fh.add(part)
            t0 = time.perf_counter()
            ch.observe(part)
            host_ms.append(round((time.perf_counter() - t0) * 1e3, 1))
        res["carver_host_numpy_ms"] = host_ms
        res["equal_to_numpy"] = bool(all((x == y).all() for x, y in zip(ca.state(), ch.state())) and torch.equal(keep.cpu(), ch.keep()))
    return res


def track_leg(args, dfr, timed):
    """frames.Tracker (csrc/frames_track.hip) beside a Fuser fed --track K frames at a time: after every chunk the tracker is
    updated on fuser.kept(1) with synthetic owners -- the block of 1.2 x 1 x 1.5 m the fused point lies in, 50 rows, numbered
    in a different order at every snapshot.  Reported: the device time of every update from events (its one read-back
    included); gf_frames_track_update alone on the last snapshot (every row continues its track: the steady state), median
    of --reps, with and without the aggregation of equal pairs among adjacent lanes; the share of the HBM peak on the
    algorithmic bytes (cells, owner and ids, 4 bytes each per point, one read and one write of the map per point);
    TrackerHost on the same updates (wall clock) and whether the two agree."""
    from geoformer_amd import _lib, frames
    from geoformer_amd._lib import check, ptr, stream_ptr

    lib = _lib.load()
    F, K = args.frames, args.track
    if K < 1 or F % K:
        raise SystemExit(f"--track {K}: a divisor of --frames {F}")
    dev = dfr.depth.device
    cut = lambda f, a, b: f._replace(depth=f.depth[a:b], color=f.color[a:b], table=f.table[a:b])  # noqa: E731
    fu = frames.Fuser(cell=args.cell, stride=args.stride, near=0.1, far=10.0, edge=args.edge)
    trackers = {agg: frames.Tracker(aggregate=agg) for agg in (1, 0)}
    host = frames.TrackerHost() if args.track_host or not args.no_host else None
    updates, cells, res, equal, host_ms = [], [], {"chunk_frames": K, "aggregate_default": frames.TRACK_AGGREGATE}, True, []
    per = {1: [], 0: []}
    for k, a in enumerate(range(0, F, K)):
        cells.append(fu.add(cut(dfr, a, a + K)))
        fused = fu.snapshot(1, torch.cat(cells))
        kept = fu.kept(1)
        b = (fused.xyz / torch.tensor([1.2, 1.0, 1.5], device=dev)).floor().to(torch.int64)
        block = b[:, 0].clamp(0, 4) + 5 * b[:, 1].clamp(0, 4) + 25 * b[:, 2].clamp(0, 1)
        turn = torch.from_numpy(np.random.default_rng(k).permutation(50)).to(dev)
        owner = turn[block].to(torch.int32)
        cls = (torch.arange(50, device=dev) % 7).to(torch.int32)
        score = torch.full((50,), 0.5 + k / 64, dtype=torch.float32, device=dev)
        updates.append((kept, owner, cls, score))
        for agg, t in trackers.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            got = t.update(kept, owner, cls, score)
            e1.record()
            torch.cuda.synchronize()
            per[agg].append(round(e0.elapsed_time(e1) * 1e3, 1))
        if host is not None:
            t0 = time.perf_counter()
            want = host.update(kept.cpu().numpy(), owner.cpu().numpy(), cls.cpu().numpy(), score.cpu().numpy())
            host_ms.append(round((time.perf_counter() - t0) * 1e3, 2))
            equal = equal and all(torch.equal(x.cpu(), y) for x, y in zip(got, want))
    t = trackers[1]
    m, p, T = int(kept.shape[0]), 50, t.tracks
    res.update(points=m, rows=p, tracks=T, live=t.live, pairs_last=t.pairs, retries=t.retries, map_growths=t.map_growths,
               update_with_readback_us_aggregated=per[1], update_with_readback_us_plain=per[0])
    if host is not None:
        res.update(tracker_host_numpy_ms=host_ms, equal_to_numpy=bool(equal))
    # the library call alone, on copies of the state: the last snapshot again and again (every row continues its track)
    slots = min(frames.tracker_slots(p, t.live, m))
    table, track_of = t._tab.clone(), t._map.clone()
    i32 = lambda n: torch.empty(max(n, 1), dtype=torch.int32, device=dev)  # noqa: E731
    ids, track, gone, words = i32(m), i32(p), i32(T), i32(16)
    ws = torch.empty(lib.gf_frames_track_scratch_bytes(m, p, T, slots) // 8 + 1, dtype=torch.int64, device=dev)
    keep = torch.ones(p, dtype=torch.uint8, device=dev)

    def run(agg):
        check(lib.gf_frames_track_update(ptr(kept), ptr(owner), m, ptr(cls), ptr(score), ptr(keep), p, ptr(track_of), t.cells,
                                         track_of.shape[0], ptr(table), T, table.shape[1], 0.3, 2, 1, 0, t.updates, slots, agg,
                                         ptr(ws), ptr(ids), ptr(track), ptr(gone), ptr(words), stream_ptr()), "gf_frames_track_update")

    res["update_us_aggregated"], res["update_us_plain"] = timed(lambda: run(1)), timed(lambda: run(0))
    res["update_us_aggregated_again"] = timed(lambda: run(1))
    run(1)
    res["words"] = words.tolist()[:8]
    nbytes = m * (4 + 4 + 4 + 4 + 4)
    best = min(res["update_us_aggregated"], res["update_us_plain"])
    res.update(slots=slots, bytes=nbytes, share_of_hbm_peak=round(nbytes / (best * 1e-6) / HBM_PEAK, 4))
    return res


def stream_leg(args, fr, dfr, timed):
    """frames.Fuser (csrc/frames_stream.hip) on the same frames, --stream K at a time: per configuration (aggregation on
    and off; the compact table that grows by doubling and a table of the proven size from the start) the device time of
    every add and of the snapshot from events, and the wall clock of the whole stream next to one-shot frames.fuse in the
    same process; the entry points on their own on the last chunk (an insert that meets known cells only, which numbers
    nothing); peak device memory of a stream fed from host memory against the one-shot call; FuserHost on the host."""
    from geoformer_amd import _lib, frames
    from geoformer_amd._lib import check, ptr, stream_ptr

    lib = _lib.load()
    F, K, s = args.frames, args.stream, args.stride
    if K < 1 or F % K:
        raise SystemExit(f"--stream {K}: a divisor of --frames {F}")
    kw = dict(cell=args.cell, stride=s, near=0.1, far=10.0, edge=args.edge)
    cut = lambda f, a, b: f._replace(depth=f.depth[a:b], color=f.color[a:b], table=f.table[a:b])  # noqa: E731
    parts = [cut(dfr, a, a + K) for a in range(0, F, K)]
    origin = None

    def stream(fu, source=parts):
        cells = [fu.add(p) for p in source]
        return fu.snapshot(args.min_obs, torch.cat(cells))

    # the origin every configuration shares (the first chunk's minimum minus the margin), and the cells at the end
    probe = frames.Fuser(**kw)
    snap = stream(probe)
    origin, M = probe.origin, probe.cells
    one = frames.fuse(dfr, args.cell, s, 0.1, 10.0, args.edge, args.min_obs, origin=origin)
    res = {"chunk_frames": K, "adds": F // K, "cells": M, "valid_pixels": probe.pixels, "origin": [float(v) for v in origin],
           "equal_to_one_shot_fuse": all(torch.equal(a, b) for a, b in zip(snap, one)),
           "default_table_slots_at_the_end": probe.slots, "rehashes": probe.rehashes, "retries": probe.retries,
           "row_growths": probe.row_growths, "aggregate_default": frames.STREAM_AGGREGATE}
    H, W = dfr.depth.shape[1:]
    proven = frames.stream_slots(M, K * -(-H // s) * -(-W // s))[1]  # at least 2 (M + n) at every add
    res["proven_table_slots"] = proven
    for table, slots in (("compact", None), ("proven", proven)):
        for agg in (1, 0):
            adds, snaps, walls = [], [], []
            for rep in range(args.reps + 1):
                fu = frames.Fuser(**kw, origin=origin, slots=slots, capacity=None if slots is None else M, aggregate=agg)
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(parts) + 2)]
                torch.cuda.synchronize()
                t = time.perf_counter()
                cells = []
                for k, p in enumerate(parts):
                    ev[k].record()
                    cells.append(fu.add(p))
                ev[len(parts)].record()
                fu.snapshot(args.min_obs, torch.cat(cells))
                ev[len(parts) + 1].record()
                torch.cuda.synchronize()
                if rep:  # (the first run warms the allocator up)
                    walls.append((time.perf_counter() - t) * 1e3)
                    adds.append([ev[k].elapsed_time(ev[k + 1]) * 1e3 for k in range(len(parts))])
                    snaps.append(ev[len(parts)].elapsed_time(ev[len(parts) + 1]) * 1e3)
            per_add = np.median(np.array(adds), axis=0)
            res[f"{table}_{'aggregated' if agg else 'plain'}"] = {
                "first_add_us": round(float(per_add[0]), 1),
                "later_add_us_median": round(float(np.median(per_add[1:])), 1) if len(per_add) > 1 else None,
                "adds_us_sum": round(float(per_add.sum()), 1), "snapshot_us": round(float(np.median(snaps)), 1),
                "stream_ms_wall": round(float(np.median(walls)), 2), "slots_at_the_end": fu.slots, "rehashes": fu.rehashes}
    wall = []
    for _ in range(5):
        torch.cuda.synchronize()
        t = time.perf_counter()
        frames.fuse(dfr, args.cell, s, 0.1, 10.0, args.edge, args.min_obs, origin=origin)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t) * 1e3)
    res["one_shot_fuse_ms_wall"] = round(float(np.median(wall)), 2)

    # the entry points on their own, on the last chunk and the final map: every cell is known, so the insert numbers
    # nothing and may be repeated; the accumulate adds into a copy of the rows
    last = parts[-1]
    pts, cols, _, _, _ = frames.backproject(last, s, 0.1, 10.0, args.edge, return_origin=True)
    pts, cols = pts.contiguous(), cols.contiguous()
    n = int(pts.shape[0])
    res["last_chunk"] = {"valid_pixels": n, "backproject_us": timed(lambda: frames.backproject(last, s, 0.1, 10.0, args.edge))}
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=pts.device)  # noqa: E731
    cell_of, words = i32(n), i32(4)
    ws = torch.empty(lib.gf_frames_map_insert_scratch_bytes(n, 0) // 8 + 1, dtype=torch.int64, device=pts.device)
    count, sums = probe._count.clone(), probe._sums.clone()
    org = torch.from_numpy(origin).to(pts.device)
    for name, fu in (("compact", probe), ("proven", fu)):  # (fu: the last configuration above, a table of the proven size)
        def insert():
            check(lib.gf_frames_map_insert(ptr(pts), n, args.cell, ptr(org), ptr(fu._keys), ptr(fu._ids), ptr(fu._first), fu.slots,
                                           fu.cells, 0, ptr(ws), ptr(cell_of), ptr(words), stream_ptr()), "gf_frames_map_insert")

        res["last_chunk"][f"insert_known_cells_{name}_us"] = timed(insert)
        assert words.tolist() == [M, 0, 0, 0]
    for agg in (1, 0):
        def accumulate():
            check(lib.gf_frames_map_accumulate(ptr(pts), ptr(cols), ptr(cell_of), n, M, ptr(org), agg, ptr(count), ptr(sums),
                                               ptr(words), stream_ptr()), "gf_frames_map_accumulate")

        res["last_chunk"][f"accumulate_{'aggregated' if agg else 'plain'}_us"] = timed(accumulate)
    res["last_chunk"]["rehash_to_the_same_size_us"] = timed(lambda: probe._rehash(probe.slots))
    res["snapshot_means_only_us"] = timed(lambda: probe.snapshot(args.min_obs))
    del pts, cols, cell_of, ws, count, sums, one, snap, fu, probe, last, parts

    # peak device memory: the frames in host memory, uploaded a chunk at a time, against the one-shot call on all of them
    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)

    host_parts = [cut(fr, a, a + K) for a in range(0, F, K)]
    res["peak_MiB_stream_from_host"] = peak(lambda: stream(frames.Fuser(**kw, origin=origin), host_parts))
    res["peak_MiB_one_shot_from_host"] = peak(lambda: frames.fuse(fr, args.cell, s, 0.1, 10.0, args.edge, args.min_obs,
                                                                  origin=origin))
    res["resident_frames_MiB"] = round((dfr.depth.numel() * dfr.depth.element_size() + dfr.color.numel()) / 2 ** 20, 1)
    if not args.no_host:
        t = time.perf_counter()
        fz = frames.FuserHost(**kw, origin=origin)
        want = fz.snapshot(args.min_obs, torch.cat([fz.add(p) for p in host_parts]))
        res["fuser_host_numpy_ms"] = round((time.perf_counter() - t) * 1e3, 1)
        got = stream(frames.Fuser(**kw, origin=origin), host_parts)
        res["equal_to_numpy"] = all(torch.equal(a.cpu(), b) for a, b in zip(got, want))
    return res


def voter_leg(args, fr, dfr, labels, timed):
    """frames.Voter (csrc/frames_vote_stream.hip) beside a frames.Fuser on the same frames, --stream K at a time, fed the
    synthetic label image (uint8 [F, Hs, Ws] on the device): per configuration (aggregation on and off; the compact table
    that grows by doubling and a table of the proven size from the start) the device time of every add and of the
    snapshot from events and the wall clock of all adds plus one snapshot, next to one frames.vote (gf_frames_vote) over
    everything in the same process; the claim / commit split of one add and a same-size rehash on the final table; the
    peak device memory of a streamed fuse-and-lift fed from host memory against the path that keeps every cell and image
    until the end; VoterHost on the host."""
    from geoformer_amd import _lib, frames
    from geoformer_amd._lib import check, ptr, stream_ptr

    lib = _lib.load()
    F, K, s = args.frames, args.stream, args.stride
    kw = dict(cell=args.cell, stride=s, near=0.1, far=10.0, edge=args.edge)
    cut = lambda f, a, b: f._replace(depth=f.depth[a:b], color=f.color[a:b], table=f.table[a:b])  # noqa: E731
    spans = [(a, a + K) for a in range(0, F, K)]
    fu = frames.Fuser(**kw)
    cells = [fu.add(cut(dfr, a, b)) for a, b in spans]
    origin, M = fu.origin, fu.cells
    values = [labels[a:b].contiguous() for a, b in spans]
    per_add = int(values[0].numel())

    probe = frames.Voter(0)
    for c, v in zip(cells, values):
        probe.add(c, v)
    got, pairs = probe.snapshot(M)
    whole_g, whole_v = torch.cat(cells).reshape(-1), labels.reshape(-1)
    one, one_pairs = frames.vote(whole_g, whole_v, M, 0)
    proven = frames.voter_slots(pairs, per_add)[1]  # at least 2 (P + T) at every add
    res = {"chunk_frames": K, "adds": len(spans), "groups": M, "elements_per_add": per_add, "pairs": pairs,
           "equal_to_one_vote": bool(all(torch.equal(a, b) for a, b in zip(got, one)) and pairs == one_pairs),
           "default_table_slots_at_the_end": probe.slots, "rehashes": probe.rehashes, "retries": probe.retries,
           "proven_table_slots": proven, "aggregate_default": frames.VOTER_AGGREGATE}
    for table, slots in (("compact", None), ("proven", proven)):
        for agg in (1, 0):
            adds, snaps, walls = [], [], []
            for rep in range(args.reps + 1):
                vt = frames.Voter(0, slots=slots, aggregate=agg)
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(spans) + 2)]
                torch.cuda.synchronize()
                t = time.perf_counter()
                for k, (c, v) in enumerate(zip(cells, values)):
                    ev[k].record()
                    vt.add(c, v)
                ev[len(spans)].record()
                vt.snapshot(M)
                ev[len(spans) + 1].record()
                torch.cuda.synchronize()
                if rep:  # (the first run warms the allocator up)
                    walls.append((time.perf_counter() - t) * 1e3)
                    adds.append([ev[k].elapsed_time(ev[k + 1]) * 1e3 for k in range(len(spans))])
                    snaps.append(ev[len(spans)].elapsed_time(ev[len(spans) + 1]) * 1e3)
            per = np.median(np.array(adds), axis=0)
            res[f"{table}_{'aggregated' if agg else 'plain'}"] = {
                "first_add_us": round(float(per[0]), 1),
                "later_add_us_median": round(float(np.median(per[1:])), 1) if len(per) > 1 else None,
                "adds_us_sum": round(float(per.sum()), 1), "snapshot_us": round(float(np.median(snaps)), 1),
                "stream_ms_wall": round(float(np.median(walls)), 2), "slots_at_the_end": vt.slots, "rehashes": vt.rehashes,
                "retries": vt.retries}
    wall = []
    for _ in range(5):
        torch.cuda.synchronize()
        t = time.perf_counter()
        frames.vote(whole_g, whole_v, M, 0)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t) * 1e3)
    res["one_vote_ms_wall"] = round(float(np.median(wall)), 2)
    res["one_vote_us"] = timed(lambda: frames.vote(whole_g, whole_v, M, 0))

    # one add in its two launches, on the last chunk and the final table: every key is known, so the claim claims nothing
    # and may be repeated; the commit adds into a copy of the counts
    g, v = cells[-1].contiguous(), values[-1]
    Fk, Hs, Ws = g.shape
    words = torch.empty(2, dtype=torch.int32, device=g.device)
    ws = torch.empty(lib.gf_frames_votes_add_scratch_bytes(per_add) // 8 + 1, dtype=torch.int64, device=g.device)
    cnt = probe._cnt.clone()
    for agg in (1, 0):
        def claim():
            check(lib.gf_frames_votes_claim(ptr(g), ptr(v), 0, 1, per_add, 1, 1, 0, 1, ptr(probe._keys), probe.slots, pairs, agg,
                                            ptr(ws), ptr(words), stream_ptr()), "gf_frames_votes_claim")

        def commit():
            check(lib.gf_frames_votes_commit(ptr(ws), per_add, ptr(cnt), probe.slots, ptr(words), stream_ptr()),
                  "gf_frames_votes_commit")

        name = "aggregated" if agg else "plain"
        res[f"claim_known_pairs_{name}_us"] = timed(claim)
        assert words.tolist() == [0, 0]
        res[f"commit_{name}_us"] = timed(commit)
    res["snapshot_us"] = timed(lambda: probe.snapshot(M))
    res["rehash_to_the_same_size_us"] = timed(lambda: probe._rehash(probe.slots))
    del g, v, ws, cnt, cells, values, whole_g, whole_v, got, one, probe, fu, vt

    # peak device memory, the frames and the label images coming from host memory: everything streamed (nothing kept but
    # the map and the two tables) against the path that keeps every chunk's cells and both images until the end
    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)

    host_labels = labels.cpu().numpy()
    del labels

    def streamed():
        fz, sv, iv = frames.Fuser(**kw, origin=origin), frames.Voter(0), frames.Voter(0)
        for a, b in spans:
            c = fz.add(cut(fr, a, b))
            sv.add(c, host_labels[a:b])
            iv.add(c, host_labels[a:b])
        return frames.lift_scene_stream(fz, sv, iv, args.min_obs)

    def kept():
        fz = frames.Fuser(**kw, origin=origin)
        fused = fz.snapshot(args.min_obs, torch.cat([fz.add(cut(fr, a, b)) for a, b in spans]))
        return frames.lift_scene(fused, host_labels, host_labels, ignore=0)

    res["peak_MiB_streamed_fuse_and_lift"] = peak(streamed)
    res["peak_MiB_keep_everything"] = peak(kept)
    a, b = streamed(), kept()
    res["streamed_equal_to_keep_everything"] = all(torch.equal(x, y) for x, y in zip(a, b))
    if not (args.no_host or args.stream_no_host):
        t = time.perf_counter()
        vh = frames.VoterHost(0)
        fz = frames.FuserHost(**kw, origin=origin)
        for a, b in spans:
            vh.add(fz.add(cut(fr, a, b)), host_labels[a:b])
        want, want_pairs = vh.snapshot(fz.cells)
        res["fuser_and_voter_host_numpy_ms"] = round((time.perf_counter() - t) * 1e3, 1)
        vt, fz2 = frames.Voter(0), frames.Fuser(**kw, origin=origin)
        for a, b in spans:
            vt.add(fz2.add(cut(fr, a, b)), host_labels[a:b])
        got, got_pairs = vt.snapshot(fz2.cells)
        res["equal_to_numpy"] = bool(all(torch.equal(x.cpu(), y) for x, y in zip(got, want)) and got_pairs == want_pairs)
    return res


if __name__ == "__main__":
    main()
