"""Training batches on the GPU: the augmentation and collate of ``InstDataset.trainMerge``
(``datasets/scannetv2_inst.py:267-387``) as HIP kernels (``csrc/augment.hip``).

    batch = train_merge([raw0, raw1], rng="device", seed=7, batch_index=i, device="cuda")
    for batch in TrainFeeder(scenes, batch_size=4, seed=7, device="cuda"): loss = crit(model(batch, ep), batch, ep)

A raw scene is the reference's ``[N, 8]`` float64 array (xyz mean-centred, rgb, 20-class label, instance id or -100),
as a numpy array or a device tensor.  The result is the reference's batch dict, same keys, dtypes and shapes, on the
device (``spatial_shape`` a numpy array, ``id`` a list).

Two sources of randomness share every kernel but the draw:
  rng="reference": numpy's legacy global stream and torch's CPU generator, consumed in exactly the reference's order and
                   amounts (the parity mode; it reads a few scalars back per scene);
  rng="device":    Philox4x32-10 on the device keyed by (seed, batch index, scene, draw, axis, cell); nothing is read
                   back before the hand-over, the same (seed, batch index) gives the same batch bit for bit.

One deliberate deviation: a scene left without instances counts 0 instances; the reference's
``int(max) + 1`` counts -99 there and shifts the ids of every later scene of the batch.

Few-shot episodes (``FSInstDataset.trainMergeFS``, ``datasets/scannetv2_fs_inst.py:397-566``) reuse the
query kernels and add the few-shot collate and the support path:

    index = FSIndex.build(scenes_by_name)
    support, query, scene_infos = train_merge_fs(scenes_by_name, index, 8, rng="device", seed=7, batch_index=i)
    for support, query, scene_infos in FSTrainFeeder(scenes_by_name, index, 8, seed=7, device="cuda"): ...
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from . import _abi, _lib
from ._lib import check, ptr

# the per-scene record of include/geoformer_hip.h (64-bit words).  Its sizes are the header's #defines; the R_* / H_* word
# offsets and the ERR_* bits are enumerators there (GF_AUG_R_*, GF_AUG_H_*, GF_AUG_ERR_*), not #defines, and stay restated
REC = _abi.const("GF_AUG_REC")
R_M, R_SHIFT, R_FLIP, R_THETA, R_AMAX0, R_AMAX1 = 0, 9, 12, 13, 14, 17
R_MIN, R_MAX, R_CHOSEN, R_ERR, R_CAP0, R_BASE0, R_CAP1, R_BASE1 = 20, 23, 26, 27, 28, 29, 30, 31
R_PCMIN, R_PCMAX, R_NINST, R_IBASE, R_COUNTS, R_CROPU = 32, 35, 38, 39, 64, 128
R_PBASE, R_CLASS, R_SUPID = 40, 41, 42
R_BMIN, R_BMAX, R_BCNT, R_BLMAX = 43, 46, 49, 50
H_N, H_NINST, H_ERR, H_SHAPE = 0, 1, 2, 6
HEAD = _abi.const("GF_AUG_HEAD")
MAX_INST = _abi.const("GF_AUG_MAX_INST")
MAX_CROP = _abi.const("GF_AUG_MAX_CROP")
ERR_CELLS, ERR_INST, ERR_NOINST = 1, 2, 4
NORMAL_MAX = 6.67  # |Box-Muller normal| from 32-bit uniforms: sqrt(2 ln 2^32) = 6.66

# datasets/scannetv2.py: the training classes of the two folds
FOLD = {0: (2, 3, 4, 7, 9, 11, 12, 13, 18), 1: (5, 6, 8, 10, 14, 15, 16, 17, 19)}


def elastic_params(scale):
    """(gran, mag) of the two elastic passes (datasets/scannetv2_inst.py:299-300)."""
    return ((6 * scale // 50, 40 * scale / 50), (20 * scale // 50, 160 * scale / 50))


def crop_candidates(full_scale_max):
    """Crop iterations that can run: candidate k has full_scale (fs - 32k, fs - 32k, fs); the first with fs - 32k <= 0
    keeps nothing and so ends the reference's loop."""
    return -(-int(full_scale_max) // 32) + 1


def grid_bb(absmax, gran):
    """Noise-grid extents: int32(|x| max) // gran + 3 (datasets/scannetv2_inst.py:147)."""
    return np.asarray(absmax, np.float64).astype(np.int32) // gran + 3


def _radius(sc):
    """Largest |xyz| row norm of a raw scene (bounds the noise grids of rng="device"); read once per device tensor."""
    if torch.is_tensor(sc):
        r = getattr(sc, "_gf_radius", None)
        if r is None:
            r = float(sc[:, :3].double().norm(dim=1).max()) if sc.shape[0] else 0.0
            sc._gf_radius = r
        return r
    return float(np.sqrt((np.asarray(sc[:, :3], np.float64) ** 2).sum(1)).max()) if len(sc) else 0.0


def device_cell_bounds(radius, scale):
    """Cells per noise grid that rng="device" can need, per pass, for a scene of the given radius: |x @ m| <= 3.01 r
    (||m||_2 <= 1 + 0.1 ||G||_F, |G_ij| <= 6.67), and pass 0 moves a point by at most mag0 * 6.67 (the blurs and the
    interpolation average)."""
    (g0, m0), (g1, _) = elastic_params(scale)
    e0 = 3.01 * radius * scale
    e1 = e0 + NORMAL_MAX * m0
    b0 = int(e0) // g0 + 4
    b1 = int(e1) // g1 + 4
    return b0 ** 3, b1 ** 3


class _Batch:
    """Device buffers of one batch (capacity = the raw points) and the struct handed to the kernels."""

    def __init__(self, raw, sizes, device, cells, max_inst=MAX_INST):
        lib = _lib.load()
        B, n = len(sizes), int(sum(sizes))
        self.B, self.n, self.sizes, self.device = B, n, list(sizes), device
        self.max_scene = max(sizes) if sizes else 0
        e = lambda shape, dt: torch.empty(shape, dtype=dt, device=device)  # noqa: E731
        i32, i64, f32, f64 = torch.int32, torch.int64, torch.float32, torch.float64
        self.raw = raw
        off = np.zeros(B + 1, np.int64)
        off[1:] = np.cumsum(sizes)
        self.off_host = off
        self.off = torch.from_numpy(off).pin_memory().to(device, non_blocking=True)
        self.rec = e((B, REC), i64)
        self.xyz_middle, self.xyz = e((n, 3), f64), e((n, 3), f64)
        self.noise = [e(max(int(c), 1) * 1, f32) for c in cells]
        self.work = [e(2 * max(int(c), 1), f32) for c in cells]
        self.cells = [max(int(c), 1) for c in cells]
        nb = lib.gf_aug_scan_blocks(n)
        self.flags, self.lab, self.inst, self.sidx = e(n, i32), e(n, i32), e(n, i32), e(n, i32)
        self.start, self.cursor = e(n + 1, i32), e(max(n, 1), i32)
        self.block_sums, self.block_off = e(nb, i32), e(nb, i32)
        self.bitmap = e(B * max_inst // 32, i32)
        self.inst_map = e(B * max_inst, i32)
        self.inst_stats = e(B * max_inst * 10, i64)
        self.out = {
            "locs": e((n, 4), i64), "locs_float": e((n, 3), f32), "feats": e((n, 3), f64), "labels": e(n, i64),
            "instance_labels": e(n, i64), "instance_infos": e((n, 9), f32),
            "instance_pointnum": e(B * max_inst, i32), "offsets": e(B + 1, i32), "pc_mins": e((B, 3), f32),
            "pc_maxs": e((B, 3), f32),
        }
        self.head = e(HEAD, i32)
        s = _lib.AugBatch()
        s.B, s.n_raw, s.max_inst = B, n, max_inst
        s.raw, s.raw_off, s.rec = ptr(self.raw), ptr(self.off), ptr(self.rec)
        s.xyz_middle, s.xyz = ptr(self.xyz_middle), ptr(self.xyz)
        for p in range(2):
            s.noise[p], s.work[p], s.cells[p] = ptr(self.noise[p]), ptr(self.work[p]), self.cells[p]
        for k in ("flags", "lab", "inst", "start", "cursor", "block_sums", "block_off", "sidx", "bitmap", "inst_map",
                  "inst_stats", "head"):
            setattr(s, k, ptr(getattr(self, k)))
        for k, v in self.out.items():
            setattr(s, k, ptr(v))
        self.s = s
        self.ref = ctypes.byref(s)

    def set_noise(self, p, cells):
        """(rng="reference") buffers of one scene's grids, sized exactly."""
        cells = max(int(cells), 1)
        e = lambda k: torch.empty(k, dtype=torch.float32, device=self.device)  # noqa: E731
        self.noise[p], self.work[p], self.cells[p] = e(cells * 3), e(cells * 6), cells * 3
        self.s.noise[p], self.s.work[p], self.s.cells[p] = ptr(self.noise[p]), ptr(self.work[p]), cells * 3


def _rec_init(B, caps=None, classes=None):
    rec = np.zeros((B, REC), np.int64)
    if classes is not None:
        rec[:, R_CLASS] = classes
    rec[:, R_MIN:R_MIN + 3] = -1  # order keys: min starts at the largest key, max at 0 (the smallest)
    rec[:, R_PCMIN:R_PCMIN + 3] = -1
    rec[:, R_CHOSEN] = -1
    if caps is not None:
        for p, (rc, rb) in enumerate(((R_CAP0, R_BASE0), (R_CAP1, R_BASE1))):
            c = np.asarray(caps[p], np.int64)
            rec[:, rc] = c
            rec[:, rb] = np.concatenate([[0], np.cumsum(3 * c)[:-1]])
    return rec


def _raw_upload(scenes, device):
    """[N,8] float64 per scene -> one device tensor [n,8] (device tensors are concatenated on the device)."""
    sizes = [int(sc.shape[0]) for sc in scenes]
    if all(torch.is_tensor(sc) and sc.is_cuda for sc in scenes):
        raw = torch.cat([sc.to(torch.float64) for sc in scenes]).contiguous()
        return raw, sizes
    host = np.concatenate([np.asarray(sc.cpu() if torch.is_tensor(sc) else sc, np.float64) for sc in scenes])
    pin = torch.from_numpy(np.ascontiguousarray(host)).pin_memory()
    raw = pin.to(device, non_blocking=True)
    raw._gf_keep = pin  # (the copy may still read it)
    return raw, sizes


class _Pending:
    """A batch whose kernels are queued; its sizes arrive in pinned words."""

    __slots__ = ("bt", "head_host", "vhead", "vhead_host", "input_map", "vscratch", "done", "mode", "fs_min", "ids",
                 "draws", "kind")


def _voxelise_count(bt, mode, st):
    lib = _lib.load()
    n = max(bt.n, 1)
    p = _Pending()
    p.vscratch = torch.empty(lib.gf_voxelize_idx_scratch_bytes(n) // 8 + 1, dtype=torch.int64, device=bt.device)
    p.input_map = torch.empty(n, dtype=torch.int32, device=bt.device)
    p.vhead = torch.empty(3, dtype=torch.int32, device=bt.device)
    check(lib.gf_voxelize_idx_count(ptr(bt.out["locs"]), bt.n, 4, int(mode), ptr(p.vscratch), ptr(p.input_map),
                                    ptr(p.vhead), st), "gf_voxelize_idx_count")
    return p


def _launch_tail(bt, cvfold, full_scale, mode, st, pinned=None, kind="merge"):
    """Collate (kind "merge": trainMerge's; "fs_query": the few-shot query's) + first half of the voxelisation + the
    sizes on their way to pinned words; returns the _Pending."""
    lib = _lib.load()
    if kind == "fs_query":
        check(lib.gf_aug_collate_fs(bt.ref, int(full_scale[0]), int(full_scale[1]), bt.max_scene, st),
              "gf_aug_collate_fs")
    else:
        fold = (ctypes.c_int32 * 9)(*FOLD[cvfold])
        check(lib.gf_aug_collate(bt.ref, fold, 9, int(full_scale[0]), int(full_scale[1]), bt.max_scene, st),
              "gf_aug_collate")
    return _queue_handover(bt, mode, st, pinned, kind)


def _queue_handover(bt, mode, st, pinned, kind):
    p = _voxelise_count(bt, mode, st)
    if pinned is None:
        pinned = (torch.empty(HEAD, dtype=torch.int32).pin_memory(), torch.empty(3, dtype=torch.int32).pin_memory())
    p.head_host, p.vhead_host = pinned
    p.head_host.copy_(bt.head, non_blocking=True)
    p.vhead_host.copy_(p.vhead, non_blocking=True)
    p.done = torch.cuda.Event()
    p.done.record(torch.cuda.current_stream(bt.device))
    p.bt, p.mode, p.kind = bt, mode, kind
    return p


def _finish(p, stream=None):
    """Read the pinned words (the work that wrote them was queued earlier), queue the second half of the voxelisation,
    hand the batch over: the current stream waits on an event only."""
    lib = _lib.load()
    bt = p.bt
    p.done.synchronize()
    head = p.head_host.tolist()
    M_pad, max_active, verr = p.vhead_host.tolist()
    what = "train_merge" if p.kind == "merge" else "train_merge_fs"
    if head[H_ERR]:
        raise _lib.GeoFormerHipError(
            what + ": " + ("a noise grid exceeds its buffer; " if head[H_ERR] & ERR_CELLS else "")
            + (f"an instance id outside [0, {MAX_INST}) (or negative but not -100)" if head[H_ERR] & ERR_INST else ""))
    if verr:
        raise _lib.GeoFormerHipError(what + ": a voxel coordinate lies outside [0, 65535]")
    N, ninst = head[H_N], head[H_NINST]
    M = M_pad - (bt.n - N)
    max_active = max(max_active, 1)
    dev = bt.device
    cur = torch.cuda.current_stream(dev)
    work = stream if stream is not None else cur
    with torch.cuda.stream(work):
        out_coords = torch.empty((max(M_pad, 0), 4), dtype=torch.int64, device=dev)
        out_map = torch.empty((max(M_pad, 0), max_active + 1), dtype=torch.int32, device=dev)
        check(lib.gf_voxelize_idx_fill(ptr(bt.out["locs"]), bt.n, 4, int(p.mode), ptr(p.vscratch), ptr(p.input_map),
                                       M_pad, max_active, ptr(out_coords), ptr(out_map), work.cuda_stream),
              "gf_voxelize_idx_fill")
        ready = torch.cuda.Event()
        ready.record(work)
    if work is not cur:
        cur.wait_event(ready)
    o = bt.out
    shape = np.asarray(head[H_SHAPE:H_SHAPE + 3], np.int64)
    if p.kind == "merge":
        batch = {
            "locs": o["locs"][:N], "voxel_locs": out_coords[:M], "p2v_map": p.input_map[:N], "v2p_map": out_map[:M],
            "locs_float": o["locs_float"][:N], "feats": o["feats"][:N], "labels": o["labels"][:N],
            "instance_labels": o["instance_labels"][:N], "instance_pointnum": o["instance_pointnum"][:ninst],
            "instance_infos": o["instance_infos"][:N], "id": p.ids, "offsets": o["offsets"],
            "spatial_shape": shape, "pc_mins": o["pc_mins"], "pc_maxs": o["pc_maxs"],
        }
    else:  # the key order of trainMergeFS's support_dict / query_dict (datasets/scannetv2_fs_inst.py:515-565)
        batch = {"voxel_locs": out_coords[:M], "p2v_map": p.input_map[:N], "v2p_map": out_map[:M],
                 "locs": o["locs"][:N], "locs_float": o["locs_float"][:N], "feats": o["feats"][:N]}
        if p.kind == "fs_query":
            batch.update(labels=o["labels"][:N], instance_labels=o["instance_labels"][:N],
                         instance_pointnum=o["instance_pointnum"][:ninst])
        elif p.kind == "fs_support":
            batch["support_masks"] = o["support_masks"][:N]
        batch.update(spatial_shape=shape, batch_offsets=o["offsets"], pc_mins=o["pc_mins"], pc_maxs=o["pc_maxs"])
    if work is not cur:
        for v in batch.values():
            if torch.is_tensor(v):
                v.record_stream(cur)
    return batch


def _host_draw_m():
    """dataAugment(xyz, True, True, True)'s draws and matrix (datasets/scannetv2_inst.py:193-204), numpy's stream."""
    m = np.eye(3)
    g = np.random.randn(3, 3)
    m += g * 0.1
    flip = np.random.randint(0, 2)
    m[0][0] *= flip * 2 - 1
    theta = np.random.rand() * 2 * math.pi
    m = np.matmul(m, [[math.cos(theta), math.sin(theta), 0], [-math.sin(theta), math.cos(theta), 0], [0, 0, 1]])
    return m, g, flip, theta


def _rec_read(bt, s):
    return bt.rec[s].cpu().numpy()


def _queue_device(scenes, raw, sizes, dev, st, scale, full_scale, max_npoint, seed, batch_index, classes=None):
    """rng="device": every launch of a batch up to the collate, on stream `st`, nothing read back (classes: the
    few-shot query's sampled class per scene)."""
    lib = _lib.load()
    B = len(sizes)
    K = crop_candidates(full_scale[1])
    caps = np.array([device_cell_bounds(_radius(sc), scale) for sc in scenes], np.int64).T
    bt = _Batch(raw, sizes, dev, (3 * int(caps[0].sum()), 3 * int(caps[1].sum())))
    bt.rec.copy_(torch.from_numpy(_rec_init(B, caps, classes)).pin_memory(), non_blocking=True)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    check(lib.gf_aug_draw(bt.ref, seed, int(batch_index), K, st), "gf_aug_draw")
    check(lib.gf_aug_transform(bt.ref, 0, B, float(scale), bt.max_scene, st), "gf_aug_transform")
    for p, (g, mg) in enumerate(elastic_params(scale)):
        check(lib.gf_aug_elastic(bt.ref, 0, B, p, int(g), float(mg), 1, seed, int(batch_index), bt.max_scene,
                                 int(caps[p].max()), st), "gf_aug_elastic")
    check(lib.gf_aug_crop(bt.ref, 0, B, int(full_scale[1]), K, int(max_npoint), bt.max_scene, st), "gf_aug_crop")
    return bt


def _device_draws(bt, scale, colour_shift, dev):
    """(rng="device", return_draws) every draw of the queued batch, read back after a sync."""
    (g0, _), (g1, _) = elastic_params(scale)
    draws = {"m": [], "flip": [], "theta": [], "noise": [], "crop_u": [], "chosen": [], "shift": [], "bb": [],
             "blurred": []}
    torch.cuda.current_stream(dev).synchronize()
    rec = bt.rec.cpu().numpy()
    nz = [bt.noise[0].cpu().numpy(), bt.noise[1].cpu().numpy()]
    wk = [bt.work[0].cpu().numpy(), bt.work[1].cpu().numpy()]
    for s in range(bt.B):
        r = rec[s]
        m = r[R_M:R_M + 9].view(np.float64).reshape(3, 3).copy()
        draws["m"].append(m)
        draws["flip"].append(int(r[R_FLIP:R_FLIP + 1].view(np.float64)[0]))
        draws["theta"].append(float(r[R_THETA:R_THETA + 1].view(np.float64)[0]))
        bbs, grids, blurred = [], [], []
        for p, (g, amax_at, capw, basew) in enumerate(((g0, R_AMAX0, R_CAP0, R_BASE0),
                                                       (g1, R_AMAX1, R_CAP1, R_BASE1))):
            bb = grid_bb(r[amax_at:amax_at + 3].view(np.float64), g)
            n = int(np.prod(bb))
            cap, base = int(r[capw]), int(r[basew])
            bbs.append(bb)
            grids.append([nz[p][base + a * cap: base + a * cap + n].reshape(bb) for a in range(3)])
            c = bt.cells[p]
            blurred.append([wk[p][c + base + a * cap: c + base + a * cap + n].reshape(bb) for a in range(3)])
        draws["bb"].append(bbs)
        draws["noise"].append(grids)
        draws["blurred"].append(blurred)
        ch = int(r[R_CHOSEN])
        draws["chosen"].append(ch)
        draws["crop_u"].append(r[R_CROPU:R_CROPU + 3 * (ch + 1)].view(np.float64).reshape(-1, 3).copy())
        if colour_shift:
            draws["shift"].append(r[R_SHIFT:R_SHIFT + 3].view(np.float64).copy())
    return draws


def _queue_reference(bt, scale, full_scale, max_npoint, st, colour_shift, return_draws):
    """rng="reference": scene by scene, numpy's legacy stream (and, with colour_shift, torch's CPU generator) in the
    reference's order and amounts, the grid extents and the crop choice read back between the launches.  Returns the
    draws used."""
    lib = _lib.load()
    dev, sizes, B = bt.device, bt.sizes, bt.B
    K = crop_candidates(full_scale[1])
    (g0, m0), (g1, m1) = elastic_params(scale)
    draws = {"m": [], "flip": [], "theta": [], "noise": [], "crop_u": [], "chosen": [], "shift": [], "bb": [],
             "blurred": []}
    fdev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    for s in range(B):
        m, g, flip, theta = _host_draw_m()
        bt.rec[s, R_M:R_M + 9] = fdev(m.reshape(-1)).view(torch.int64)
        check(lib.gf_aug_transform(bt.ref, s, 1, float(scale), sizes[s], st), "gf_aug_transform")
        bbs, grids, blurred = [], [], []
        for p, (gr, mg, amax_at, capw) in enumerate(((g0, m0, R_AMAX0, R_CAP0), (g1, m1, R_AMAX1, R_CAP1))):
            r = _rec_read(bt, s)
            bb = grid_bb(r[amax_at:amax_at + 3].view(np.float64), gr)
            n = int(np.prod(bb))
            noise = [np.random.randn(bb[0], bb[1], bb[2]).astype("float32") for _ in range(3)]
            bt.set_noise(p, n)
            bt.noise[p].copy_(fdev(np.concatenate([x.reshape(-1) for x in noise])))
            bt.rec[s, capw] = n
            bt.rec[s, capw + 1] = 0
            check(lib.gf_aug_elastic(bt.ref, s, 1, p, int(gr), float(mg), 0, 0, 0, sizes[s], n, st),
                  "gf_aug_elastic")
            bbs.append(bb)
            grids.append(noise)
            if return_draws:
                w = bt.work[p][3 * n:].cpu().numpy()
                blurred.append([w[a * n:(a + 1) * n].reshape(bb) for a in range(3)])
        chosen = -1
        u = np.zeros((0, 3))
        if sizes[s] > max_npoint:
            state = np.random.get_state()
            cand = np.random.rand(K, 3)
            bt.rec[s, R_CROPU:R_CROPU + 3 * K] = fdev(cand.reshape(-1)).view(torch.int64)
            check(lib.gf_aug_crop(bt.ref, s, 1, int(full_scale[1]), K, int(max_npoint), sizes[s], st),
                  "gf_aug_crop")
            chosen = int(_rec_read(bt, s)[R_CHOSEN])
            np.random.set_state(state)
            u = np.random.rand(chosen + 1, 3)  # what the reference's loop consumed
            assert (u == cand[:chosen + 1]).all()
        if colour_shift:
            shift = (torch.randn(3) * 0.1).double().numpy()
            bt.rec[s, R_SHIFT:R_SHIFT + 3] = fdev(shift).view(torch.int64)
            draws["shift"].append(shift)
        for k, v in (("m", m), ("flip", int(flip)), ("theta", theta), ("noise", grids), ("crop_u", u),
                     ("chosen", chosen), ("bb", bbs), ("blurred", blurred)):
            draws[k].append(v)
    return draws


def train_merge(scenes, *, scale=50, full_scale=(128, 512), max_npoint=250000, mode=4, cvfold=0, rng="reference",
                seed=None, batch_index=0, device="cuda", stream=None, return_draws=False, ids=None):
    """The reference's trainMerge on the GPU.  Returns the batch dict (and, with return_draws, a dict of every draw
    used: m, flip, theta, the raw noise grids per scene and pass, the crop offsets of the iterations that ran, the chosen
    iteration, the colour shift; plus the blurred grids)."""
    if rng not in ("reference", "device"):
        raise ValueError("rng: 'reference' or 'device'")
    if rng == "device" and seed is None:
        raise ValueError('rng="device" needs a seed')
    if cvfold not in FOLD:
        raise ValueError("cvfold: 0 or 1")
    dev = torch.device(device)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    st_obj = stream if stream is not None else torch.cuda.current_stream(dev)
    with torch.cuda.stream(st_obj):
        st = st_obj.cuda_stream
        raw, sizes = _raw_upload(scenes, dev)
        B = len(sizes)
        if crop_candidates(full_scale[1]) > MAX_CROP:
            raise ValueError(f"full_scale[1] allows at most {32 * (MAX_CROP - 1)}")
        if rng == "device":
            bt = _queue_device(scenes, raw, sizes, dev, st, scale, full_scale, max_npoint, seed, batch_index)
            draws = _device_draws(bt, scale, True, dev) if return_draws else None
        else:
            bt = _Batch(raw, sizes, dev, (1, 1))
            bt.rec.copy_(torch.from_numpy(_rec_init(B)))
            draws = _queue_reference(bt, scale, full_scale, max_npoint, st, True, return_draws)
        p = _launch_tail(bt, cvfold, full_scale, mode, st)
        p.ids = list(ids) if ids is not None else list(range(B))
    batch = _finish(p)
    return (batch, draws) if return_draws else batch


class TrainFeeder:
    """for batch in TrainFeeder(scenes, batch_size=4, seed=7, device="cuda"): ...

    Freshly augmented batches (rng="device", batch index = 0, 1, 2, ...) built one batch ahead on the feeder's own
    stream, with DeviceFeeder's hand-over: start(i+1) queues every kernel of batch i+1 and the first half of its
    voxelisation, the sizes go to pinned words; finish(i+1), at the next hand-over, reads those words (written by work
    queued a step earlier), queues the second half and hands the batch over behind an event.  scene_source yields raw
    [N,8] scenes (device tensors: nothing crosses the bus; numpy arrays: uploaded through pinned staging);
    reserve_points: the largest batch (points) to stage, allocated up front."""

    def __init__(self, scene_source, batch_size, seed, device, reserve_points=None, **train_merge_kw):
        for k in ("rng", "return_draws", "batch_index", "seed", "stream"):
            if k in train_merge_kw:
                raise TypeError(f"TrainFeeder: {k} is set by the feeder")
        self.kw = dict(scale=50, full_scale=(128, 512), max_npoint=250000, mode=4, cvfold=0)
        self.kw.update(train_merge_kw)
        self.src = iter(scene_source)
        self.batch_size, self.seed = int(batch_size), int(seed) & 0xFFFFFFFFFFFFFFFF
        dev = torch.device(device)
        self.device = dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())
        self.stream = torch.cuda.Stream(device=self.device)
        self.batch_index = 0
        self.slot = 0
        self.pinned = [(torch.zeros(HEAD, dtype=torch.int32).pin_memory(), torch.zeros(3, dtype=torch.int32).pin_memory())
                       for _ in range(3)]
        self.stage = None
        if reserve_points:
            self.stage = [torch.empty((int(reserve_points), 8), dtype=torch.float64).pin_memory() for _ in range(3)]
        self.stage_done = [None, None, None]
        self.next = self._start()

    def _upload(self, scenes):
        if all(torch.is_tensor(sc) and sc.is_cuda for sc in scenes):
            return _raw_upload(scenes, self.device)
        sizes = [int(sc.shape[0]) for sc in scenes]
        n = sum(sizes)
        if self.stage is None or self.stage[self.slot].shape[0] < n:
            rows = max(n, int(1.3 * n))
            self.stage = [torch.empty((rows, 8), dtype=torch.float64).pin_memory() for _ in range(3)]
        if self.stage_done[self.slot] is not None:
            self.stage_done[self.slot].synchronize()  # three hand-overs ago: long done
        buf = self.stage[self.slot][:n]
        o = 0
        for sc, k in zip(scenes, sizes):
            buf[o:o + k].numpy()[...] = sc.cpu().numpy() if torch.is_tensor(sc) else sc
            o += k
        raw = buf.to(self.device, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        self.stage_done[self.slot] = ev
        return raw, sizes

    def _start(self):
        scenes = []
        for _ in range(self.batch_size):
            try:
                scenes.append(next(self.src))
            except StopIteration:
                break
        if len(scenes) < self.batch_size:  # drop_last, as the reference's trainLoader
            return None
        kw = self.kw
        bi = self.batch_index
        with torch.cuda.stream(self.stream):
            st = self.stream.cuda_stream
            raw, sizes = self._upload(scenes)
            bt = _queue_device(scenes, raw, sizes, self.device, st, kw["scale"], kw["full_scale"], kw["max_npoint"],
                               self.seed, bi)
            p = _launch_tail(bt, kw["cvfold"], kw["full_scale"], kw["mode"], st, self.pinned[self.slot])
            p.ids = list(range(bi * self.batch_size, (bi + 1) * self.batch_size))
        self.batch_index += 1
        self.slot = (self.slot + 1) % 3
        return p

    def __iter__(self):
        return self

    def __next__(self):
        if self.next is None:
            raise StopIteration
        out = _finish(self.next, self.stream)
        self.next = self._start()
        return out


# ============================== few-shot episodes (FSInstDataset.trainMergeFS) ==============================
# datasets/scannetv2_fs_inst.py:397-566 per episode item: a class of the fold, a query scene listing it (augmented and
# cropped as in trainMerge, label = (label == class), no colour shift, scene-local instance ids), a support instance of
# the class whose scene has more than SUPPORT_MIN_LABELLED nonzero labels (no augmentation, no crop).

SUPPORT_MIN_LABELLED = 100  # np.count_nonzero(support_label) > 100 (the whole scene's labels, not the instance's)
SUPPORT_MAX_INST = 256  # (the support path uses no instance buffers; the smallest legal size)
DRAW_CHOICE = 5  # Philox draw id of rng="device"'s episode choices (csrc/augment.hip's device draws use 0..4)
CHOICE_CLASS, CHOICE_QUERY, CHOICE_SUPPORT = 0, 1, 2
N_CLASSES = 20


def _host_array(sc):
    return sc.detach().cpu().numpy() if torch.is_tensor(sc) else np.asarray(sc)


class FSIndex:
    """The few-shot sampling tables: class2scans {class: [scene, ...]}, class2instances {class: [[scene, id], ...]} and,
    per scene, the nonzero-label count the support loop tests.  The order of each list decides random.choice."""

    SCAN_RATIO, INST_RATIO, MIN_PTS = 0.05, 0.002, 100  # datasets/scannetv2.py:88-89, 124-125

    def __init__(self, class2scans, class2instances, counts):
        self.class2scans = {int(k): list(v) for k, v in class2scans.items()}
        self.class2instances = {int(k): [list(t) for t in v] for k, v in class2instances.items()}
        self.counts = {str(k): int(v) for k, v in counts.items()}
        missing = {s for v in self.class2instances.values() for s, _ in v} - set(self.counts)
        if missing:
            raise ValueError(f"FSIndex: no nonzero-label count for {sorted(missing)[:5]}")

    @classmethod
    def from_tables(cls, class2scans, class2instances, counts):
        """The reference's pickled tables as they are (class2scans.pkl, class2instances.pkl) plus the per-scene counts."""
        return cls(class2scans, class2instances, counts)

    @classmethod
    def build(cls, scenes_by_name):
        """The tables of datasets/scannetv2.py:75-159 over {name: raw [N,8] scene}: a scene lists a class when more
        than max(int(5 % N), 100) of its points carry it (scenes in the mapping's order, which stands for the glob's);
        an instance is listed under the label of its first point when it has more than max(int(0.2 % N), 100) points
        and that label is not -100 (scenes in sorted order, ids ascending)."""
        c2s = {k: [] for k in range(N_CLASSES)}
        c2i = {k: [] for k in range(N_CLASSES)}
        counts, host = {}, {}
        for name, sc in scenes_by_name.items():
            data = _host_array(sc)
            host[name] = data
            labels = data[:, 6].astype(np.int64)
            counts[name] = int(np.count_nonzero(labels))
            threshold = max(int(data.shape[0] * cls.SCAN_RATIO), cls.MIN_PTS)
            for c, n in zip(*np.unique(labels, return_counts=True)):
                if c != -100 and n > threshold:
                    c2s.setdefault(int(c), []).append(name)
        for name in sorted(host):
            data = host[name]
            labels, inst = data[:, 6].astype(np.int64), data[:, 7].astype(np.int64)
            threshold = max(int(data.shape[0] * cls.INST_RATIO), cls.MIN_PTS)
            ids, first, n = np.unique(inst, return_index=True, return_counts=True)
            for i, f, k in zip(ids, first, n):
                if i != -100 and k > threshold and labels[f] != -100:
                    c2i.setdefault(int(labels[f]), []).append([name, i])
        return cls(c2s, c2i, counts)


def _philox_host(c, seed):
    """Philox4x32-10 of csrc/augment.hip on the host (counter of four 32-bit words, key = seed)."""
    M = 0xFFFFFFFF
    c0, c1, c2, c3 = (int(v) & M for v in c)
    k0, k1 = seed & M, (seed >> 32) & M
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M, (p0 >> 32) ^ c3 ^ k1, p0 & M
        k0, k1 = (k0 + 0x9E3779B9) & M, (k1 + 0xBB67AE85) & M
    return c0, c1, c2, c3


def choice_index(n, seed, batch_index, item, what, attempt=0):
    """rng="device"'s choice among n: counter (attempt, DRAW_CHOICE << 2 | what, item, batch index), key = seed, a
    53-bit uniform scaled to [0, n)."""
    x, y, _, _ = _philox_host((attempt, DRAW_CHOICE << 2 | what, item, batch_index), int(seed) & 0xFFFFFFFFFFFFFFFF)
    u = ((x >> 5) * 67108864 + (y >> 6)) / 9007199254740992.0
    return min(int(u * n), n - 1)


def sample_episode(index, batch_size, cvfold=0, rng="reference", seed=None, batch_index=0):
    """The choices of one episode, as trainMergeFS's scene_infos: per item {sampled_class, query_scene, support_scene,
    support_instance_id}.  rng="reference" calls random.choice in the reference's order (class, query scene, support
    draws until one fits, item by item); rng="device" takes choice_index keyed by (seed, batch index, item)."""
    import random

    classes = FOLD[cvfold]
    if rng == "reference":
        pick = lambda seq, item, what, attempt: random.choice(seq)  # noqa: E731
    else:
        pick = lambda seq, item, what, attempt: seq[choice_index(len(seq), seed, batch_index, item, what,  # noqa: E731
                                                                 attempt)]
    infos = []
    for i in range(batch_size):
        c = pick(classes, i, CHOICE_CLASS, 0)
        scans = index.class2scans.get(c, [])
        if not scans:
            raise ValueError(f"train_merge_fs: class {c} lists no scene (class2scans)")
        q = pick(scans, i, CHOICE_QUERY, 0)
        insts = index.class2instances.get(c, [])
        if not any(index.counts[s] > SUPPORT_MIN_LABELLED for s, _ in insts):
            raise ValueError(f"train_merge_fs: class {c} lists no support instance in a scene with more than "
                             f"{SUPPORT_MIN_LABELLED} labelled points (the reference's loop would not end)")
        k = 0
        while True:
            s, sid = pick(insts, i, CHOICE_SUPPORT, k)
            k += 1
            if index.counts[s] > SUPPORT_MIN_LABELLED:
                break
        infos.append({"sampled_class": c, "query_scene": q, "support_scene": s, "support_instance_id": sid})
    return infos


def _queue_support(scenes, ids, dev, st, scale, full_scale, mode, pinned=None):
    """The support batch (load_single(aug=False, support=True) per scene, the collate): three launches and the first
    half of the voxelisation on stream `st`; returns the _Pending."""
    lib = _lib.load()
    raw, sizes = _raw_upload(scenes, dev)
    bt = _Batch(raw, sizes, dev, (1, 1), max_inst=SUPPORT_MAX_INST)
    bt.out["support_masks"] = torch.empty(bt.n, dtype=torch.int64, device=dev)
    rec = _rec_init(bt.B)
    rec[:, R_SUPID] = np.asarray(ids, np.int64)
    bt.rec.copy_(torch.from_numpy(rec).pin_memory(), non_blocking=True)
    check(lib.gf_aug_support(bt.ref, ptr(bt.out["support_masks"]), float(scale), int(full_scale[0]), bt.max_scene, st),
          "gf_aug_support")
    return _queue_handover(bt, mode, st, pinned, "fs_support")



def _queue_fs(scene_of, infos, dev, st, rng, seed, batch_index, scale, full_scale, max_npoint, mode, return_draws,
              pinned=(None, None)):
    """Every launch of one episode on stream `st`: the query batch (rng as in train_merge, no colour shift, the
    few-shot collate), then the support batch.  Returns (query _Pending, support _Pending, draws)."""
    if crop_candidates(full_scale[1]) > MAX_CROP:
        raise ValueError(f"full_scale[1] allows at most {32 * (MAX_CROP - 1)}")
    q_scenes = [scene_of[i["query_scene"]] for i in infos]
    classes = np.array([i["sampled_class"] for i in infos], np.int64)
    raw, sizes = _raw_upload(q_scenes, dev)
    draws = None
    if rng == "device":
        bt = _queue_device(q_scenes, raw, sizes, dev, st, scale, full_scale, max_npoint, seed, batch_index, classes)
        if return_draws:
            draws = _device_draws(bt, scale, False, dev)
    else:
        bt = _Batch(raw, sizes, dev, (1, 1))
        bt.rec.copy_(torch.from_numpy(_rec_init(len(sizes), classes=classes)))
        draws = _queue_reference(bt, scale, full_scale, max_npoint, st, False, return_draws)
    pq = _launch_tail(bt, 0, full_scale, mode, st, pinned[0], kind="fs_query")
    ps = _queue_support([scene_of[i["support_scene"]] for i in infos], [i["support_instance_id"] for i in infos], dev,
                        st, scale, full_scale, mode, pinned[1])
    return pq, ps, draws


def train_merge_fs(scene_of, index, batch_size, *, rng="reference", seed=None, batch_index=0, cvfold=0, scale=50,
                   full_scale=(128, 512), max_npoint=250000, mode=4, device="cuda", stream=None, return_draws=False):
    """The reference's trainMergeFS on the GPU: returns (support_dict, query_dict, scene_infos) with the reference's
    keys and dtypes, tensors on the device (spatial_shape a numpy array).  scene_of maps a scene name to its raw [N,8]
    scene (numpy or device tensor); index is an FSIndex.  rng="reference" consumes Python's random and numpy's legacy
    stream as the reference does, and no torch draw; rng="device" draws the choices on the host with choice_index and
    the augmentation with the device Philox, keyed by (seed, batch index).  return_draws adds a fourth value: the query
    augmentation's draws as train_merge returns them (no colour shift)."""
    if rng not in ("reference", "device"):
        raise ValueError("rng: 'reference' or 'device'")
    if rng == "device" and seed is None:
        raise ValueError('rng="device" needs a seed')
    if cvfold not in FOLD:
        raise ValueError("cvfold: 0 or 1")
    dev = torch.device(device)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    infos = sample_episode(index, batch_size, cvfold, rng, seed, batch_index)
    st_obj = stream if stream is not None else torch.cuda.current_stream(dev)
    with torch.cuda.stream(st_obj):
        pq, ps, draws = _queue_fs(scene_of, infos, dev, st_obj.cuda_stream, rng, seed, batch_index, scale, full_scale,
                                  max_npoint, mode, return_draws)
    query, support = _finish(pq), _finish(ps)
    return (support, query, infos, draws) if return_draws else (support, query, infos)


class FSTrainFeeder:
    """for support, query, scene_infos in FSTrainFeeder(scenes, index, batch_size=8, seed=7, device="cuda"): ...

    Few-shot episodes (rng="device", batch index = 0, 1, 2, ...) built one episode ahead on the feeder's own stream
    with TrainFeeder's hand-over: start(i+1) queues every launch of episode i+1 (query and support) and the first half
    of both voxelisations; finish(i+1), at the next hand-over, reads their sizes from pinned words written by work
    queued a step earlier, queues the second halves and hands the episode over behind an event.  scene_of maps names to
    raw [N,8] scenes (resident device tensors: nothing crosses the bus); episodes: how many (None: no end)."""

    def __init__(self, scene_of, index, batch_size, seed, device, episodes=None, **train_merge_fs_kw):
        for k in ("rng", "return_draws", "batch_index", "seed", "stream"):
            if k in train_merge_fs_kw:
                raise TypeError(f"FSTrainFeeder: {k} is set by the feeder")
        self.kw = dict(scale=50, full_scale=(128, 512), max_npoint=250000, mode=4, cvfold=0)
        self.kw.update(train_merge_fs_kw)
        if self.kw["cvfold"] not in FOLD:
            raise ValueError("cvfold: 0 or 1")
        self.scene_of, self.index = scene_of, index
        self.batch_size, self.seed = int(batch_size), int(seed) & 0xFFFFFFFFFFFFFFFF
        self.episodes = episodes
        dev = torch.device(device)
        self.device = dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())
        self.stream = torch.cuda.Stream(device=self.device)
        self.batch_index = 0
        self.slot = 0
        pin = lambda n: torch.zeros(n, dtype=torch.int32).pin_memory()  # noqa: E731
        self.pinned = [((pin(HEAD), pin(3)), (pin(HEAD), pin(3))) for _ in range(3)]
        self.next = self._start()

    def _start(self):
        if self.episodes is not None and self.batch_index >= self.episodes:
            return None
        kw, bi = self.kw, self.batch_index
        infos = sample_episode(self.index, self.batch_size, kw["cvfold"], "device", self.seed, bi)
        with torch.cuda.stream(self.stream):
            pq, ps, _ = _queue_fs(self.scene_of, infos, self.device, self.stream.cuda_stream, "device", self.seed, bi,
                                  kw["scale"], kw["full_scale"], kw["max_npoint"], kw["mode"], False,
                                  self.pinned[self.slot])
        self.batch_index += 1
        self.slot = (self.slot + 1) % 3
        return pq, ps, infos

    def __iter__(self):
        return self

    def __next__(self):
        if self.next is None:
            raise StopIteration
        pq, ps, infos = self.next
        query, support = _finish(pq, self.stream), _finish(ps, self.stream)
        self.next = self._start()
        return support, query, infos


# ============================== few-shot test time (FSInstDataset.testMergeFS) ==============================
# datasets/scannetv2_fs_inst.py:568-700 per val scene: the query (load_single(aug=False, val=True): no crop), and, without
# fix_support, per active label the block support of its (scene, instance id) (load_single_block with get_region_inst,
# scale_factor 1).  test_fs.py's full-scene supports (fix_support) are full_scene_supports below.

def _keys_to_f64(keys):
    """Order-preserving keys of csrc/augment.hip (int64 device tensor) back to the doubles, on the device."""
    k = torch.where(keys < 0, keys & 0x7FFFFFFFFFFFFFFF, ~keys)  # top bit set: the key of a non-negative double
    return k.contiguous().view(torch.float64)


def _device_of(device):
    dev = torch.device(device)
    return dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())


def _voxelise_tail(p, locs, n, mode, M_pad, max_active, stream):
    """Second half of a voxelisation queued by _voxelise_count on `locs` [n, 4] (its sizes already read)."""
    lib = _lib.load()
    max_active = max(max_active, 1)
    dev = locs.device
    out_coords = torch.empty((max(M_pad, 0), 4), dtype=torch.int64, device=dev)
    out_map = torch.empty((max(M_pad, 0), max_active + 1), dtype=torch.int32, device=dev)
    check(lib.gf_voxelize_idx_fill(ptr(locs), n, 4, int(mode), ptr(p.vscratch), ptr(p.input_map), M_pad, max_active,
                                   ptr(out_coords), ptr(out_map), stream), "gf_voxelize_idx_fill")
    return out_coords, out_map


def _queue_test_query(scene, dev, st, scale, full_scale, mode):
    """The few-shot test query of one raw scene: gf_aug_test_query and the first half of the voxelisation."""
    lib = _lib.load()
    raw, sizes = _raw_upload([scene], dev)
    bt = _Batch(raw, sizes, dev, (1, 1), max_inst=SUPPORT_MAX_INST)
    bt.rec.copy_(torch.from_numpy(_rec_init(1)).pin_memory(), non_blocking=True)
    check(lib.gf_aug_test_query(bt.ref, float(scale), int(full_scale[0]), bt.max_scene, st), "gf_aug_test_query")
    return _queue_handover(bt, mode, st, None, "fs_test_query")


def _finish_test_query(p):
    """The query dict of testMergeFS (its key order and dtypes: float32 feats, float64 [1,3] pc_mins / pc_maxs)."""
    bt = p.bt
    b = _finish(p)
    rec = bt.rec[0]
    return {"voxel_locs": b["voxel_locs"], "p2v_map": b["p2v_map"], "v2p_map": b["v2p_map"], "locs": b["locs"],
            "locs_float": b["locs_float"], "feats": b["feats"].float(), "spatial_shape": b["spatial_shape"],
            "batch_offsets": b["batch_offsets"],
            "pc_mins": _keys_to_f64(rec[R_PCMIN:R_PCMIN + 3]).unsqueeze(0),
            "pc_maxs": _keys_to_f64(rec[R_PCMAX:R_PCMAX + 3]).unsqueeze(0),
            "labels": bt.out["labels"][:b["locs"].shape[0]]}


class _Range:
    """One scene's raw range of a batch, with the attributes _voxelise_count reads."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def support_blocks(scene_of, pairs, *, scale=50, full_scale_support=(64, 128), mode=4, device="cuda", stream=None):
    """load_single_block(scene, id, aug=False, permutate=False) + testMergeFS's support dict for every (scene name,
    instance id) pair, as one batch (gf_aug_support_block) with one synchronisation for all the sizes.  Returns the list
    of support dicts in the reference's key order and dtypes.  An id without points in its scene raises
    GeoFormerHipError (the reference fails inside np.min)."""
    lib = _lib.load()
    dev = _device_of(device)
    if not pairs:
        return []
    st_obj = stream if stream is not None else torch.cuda.current_stream(dev)
    with torch.cuda.stream(st_obj):
        st = st_obj.cuda_stream
        raw, sizes = _raw_upload([scene_of[s] for s, _ in pairs], dev)
        bt = _Batch(raw, sizes, dev, (1, 1), max_inst=SUPPORT_MAX_INST)
        masks = torch.empty(bt.n, dtype=torch.int64, device=dev)
        scene_sizes = torch.empty((bt.B, 5), dtype=torch.int32, device=dev)
        rec = _rec_init(bt.B)
        rec[:, R_SUPID] = np.asarray([i for _, i in pairs], np.int64)
        rec[:, R_BMIN:R_BMIN + 3] = -1
        bt.rec.copy_(torch.from_numpy(rec).pin_memory(), non_blocking=True)
        check(lib.gf_aug_support_block(bt.ref, ptr(masks), ptr(scene_sizes), float(scale), int(full_scale_support[0]),
                                       bt.max_scene, st), "gf_aug_support_block")
        off = bt.off_host
        pend = []
        for s in range(bt.B):  # each scene's raw range voxelises on its own (padding rows behind its kept points)
            locs = bt.out["locs"][off[s]:off[s + 1]]
            sub = _Range(out={"locs": locs}, n=int(sizes[s]), device=dev)
            pend.append((_voxelise_count(sub, mode, st), locs))
        host = torch.empty(HEAD + bt.B * 5 + 3 * bt.B, dtype=torch.int32).pin_memory()
        host[:HEAD].copy_(bt.head, non_blocking=True)
        host[HEAD:HEAD + bt.B * 5].copy_(scene_sizes.view(-1), non_blocking=True)
        vh = host[HEAD + bt.B * 5:]
        for s, (p, _) in enumerate(pend):
            vh[3 * s:3 * s + 3].copy_(p.vhead, non_blocking=True)
        done = torch.cuda.Event()
        done.record(st_obj)
    done.synchronize()  # the batch's one synchronisation
    h = host.tolist()
    if h[H_ERR]:
        raise _lib.GeoFormerHipError(
            "support_blocks: " + ("a support instance id has no point in its scene" if h[H_ERR] & ERR_NOINST else
                                  f"error bits {h[H_ERR]}"))
    out = []
    with torch.cuda.stream(st_obj):
        st = st_obj.cuda_stream
        pcmin = _keys_to_f64(bt.rec[:, R_PCMIN:R_PCMIN + 3])
        pcmax = _keys_to_f64(bt.rec[:, R_PCMAX:R_PCMAX + 3])
        for s, (p, locs) in enumerate(pend):
            kept, ninst = h[HEAD + 5 * s], h[HEAD + 5 * s + 1]
            shape = np.asarray(h[HEAD + 5 * s + 2:HEAD + 5 * s + 5], np.int64)
            M_pad, max_active, verr = h[HEAD + 5 * bt.B + 3 * s:HEAD + 5 * bt.B + 3 * s + 3]
            if verr:
                raise _lib.GeoFormerHipError("support_blocks: a voxel coordinate lies outside [0, 65535]")
            n = int(sizes[s])
            coords, vmap = _voxelise_tail(p, locs, n, mode, M_pad, max_active, st)
            M = M_pad - (n - kept)
            r0 = int(off[s])
            out.append({
                "voxel_locs": coords[:M], "p2v_map": p.input_map[:kept], "v2p_map": vmap[:M], "locs": locs[:kept],
                "locs_float": bt.out["locs_float"][r0:r0 + kept], "feats": bt.out["feats"][r0:r0 + kept].float(),
                "support_masks": masks[r0:r0 + kept], "spatial_shape": shape,
                "batch_offsets": torch.tensor([0, kept], dtype=torch.int32, device=dev),
                "mask_offsets": torch.tensor([0, ninst], dtype=torch.int32, device=dev),
                "pc_mins": pcmin[s:s + 1], "pc_maxs": pcmax[s:s + 1]})
    return out


def full_scene_supports(scene_of, pairs, *, scale=50, full_scale=(128, 512), mode=4, device="cuda", stream=None):
    """The support dict load_set_support builds (test_fs.py:61-108: load_single(aug=False, val=True, support=True), the
    spatial shape clipped at full_scale[0]) for a BATCH of (scene name, instance id) pairs: one dict with batch index =
    position, ready for process_support with B = len(pairs).  Keys: the reference's (mask_offsets = running counts of
    the masks, int32 [B+1]) plus pc_mins / pc_maxs."""
    dev = _device_of(device)
    st_obj = stream if stream is not None else torch.cuda.current_stream(dev)
    with torch.cuda.stream(st_obj):
        p = _queue_support([scene_of[s] for s, _ in pairs], [i for _, i in pairs], dev, st_obj.cuda_stream, scale,
                           full_scale, mode)
    d = _finish(p)
    counts = torch.zeros(len(pairs) + 1, dtype=torch.int64, device=dev)
    bidx = d["locs"][:, 0]
    counts[1:] = torch.bincount(bidx[d["support_masks"] == 1], minlength=len(pairs))
    return {"voxel_locs": d["voxel_locs"], "p2v_map": d["p2v_map"], "v2p_map": d["v2p_map"], "locs": d["locs"],
            "locs_float": d["locs_float"], "feats": d["feats"].float(), "support_masks": d["support_masks"],
            "spatial_shape": d["spatial_shape"], "batch_offsets": d["batch_offsets"],
            "mask_offsets": counts.cumsum(0).to(torch.int32), "pc_mins": d["pc_mins"], "pc_maxs": d["pc_maxs"]}


def test_merge_fs(scene_of, test_set, name, *, fix_support=True, cvfold=0, scale=50, full_scale=(128, 512),
                  full_scale_support=(64, 128), mode=4, device="cuda", stream=None):
    """The reference's testMergeFS for val scene `name` on the GPU: (is_valid, list_support_dicts, query_dict,
    scene_infos) with its keys, values and dtypes (tensors on the device, spatial_shape a numpy array).  test_set: a
    fs_eval.FSTestSet (its combinations give the active labels and, without fix_support, each label's (scene, id)).
    A scene without active label gives (False, {}, {}, {}) as the reference does."""
    if cvfold not in FOLD:
        raise ValueError("cvfold: 0 or 1")
    comb = test_set.combination(name)
    active = list(comb["active_label"])
    if not active:
        return False, {}, {}, {}
    dev = _device_of(device)
    infos = {"query_scene": name, "active_label": active}
    st_obj = stream if stream is not None else torch.cuda.current_stream(dev)
    with torch.cuda.stream(st_obj):
        pq = _queue_test_query(scene_of[name], dev, st_obj.cuda_stream, scale, full_scale, mode)
    query = _finish_test_query(pq)
    if fix_support:
        return True, [None] * len(active), query, infos
    pairs = [tuple(comb[l]) for l in active]
    for l, t in zip(active, pairs):
        infos[l] = t
    sups = support_blocks(scene_of, pairs, scale=scale, full_scale_support=full_scale_support, mode=mode, device=dev,
                          stream=stream)
    return True, sups, query, infos
