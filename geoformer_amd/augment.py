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
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr

# the per-scene record of include/geoformer_hip.h (64-bit words)
REC = 320
R_M, R_SHIFT, R_FLIP, R_THETA, R_AMAX0, R_AMAX1 = 0, 9, 12, 13, 14, 17
R_MIN, R_MAX, R_CHOSEN, R_ERR, R_CAP0, R_BASE0, R_CAP1, R_BASE1 = 20, 23, 26, 27, 28, 29, 30, 31
R_PCMIN, R_PCMAX, R_NINST, R_IBASE, R_COUNTS, R_CROPU = 32, 35, 38, 39, 64, 128
H_N, H_NINST, H_ERR, H_SHAPE = 0, 1, 2, 6
HEAD = 16
MAX_INST = 4096
MAX_CROP = 64
ERR_CELLS, ERR_INST = 1, 2
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


def _rec_init(B, caps=None):
    rec = np.zeros((B, REC), np.int64)
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
                 "draws")


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


def _launch_tail(bt, cvfold, full_scale, mode, st, pinned=None):
    """Collate + first half of the voxelisation + the sizes on their way to pinned words; returns the _Pending."""
    lib = _lib.load()
    fold = (ctypes.c_int32 * 9)(*FOLD[cvfold])
    check(lib.gf_aug_collate(bt.ref, fold, 9, int(full_scale[0]), int(full_scale[1]), bt.max_scene, st),
          "gf_aug_collate")
    p = _voxelise_count(bt, mode, st)
    if pinned is None:
        pinned = (torch.empty(HEAD, dtype=torch.int32).pin_memory(), torch.empty(3, dtype=torch.int32).pin_memory())
    p.head_host, p.vhead_host = pinned
    p.head_host.copy_(bt.head, non_blocking=True)
    p.vhead_host.copy_(p.vhead, non_blocking=True)
    p.done = torch.cuda.Event()
    p.done.record(torch.cuda.current_stream(bt.device))
    p.bt, p.mode = bt, mode
    return p


def _finish(p, stream=None):
    """Read the pinned words (the work that wrote them was queued earlier), queue the second half of the voxelisation,
    hand the batch over: the current stream waits on an event only."""
    lib = _lib.load()
    bt = p.bt
    p.done.synchronize()
    head = p.head_host.tolist()
    M_pad, max_active, verr = p.vhead_host.tolist()
    if head[H_ERR]:
        raise _lib.GeoFormerHipError(
            "train_merge: " + ("a noise grid exceeds its buffer; " if head[H_ERR] & ERR_CELLS else "")
            + (f"an instance id outside [0, {MAX_INST}) (or negative but not -100)" if head[H_ERR] & ERR_INST else ""))
    if verr:
        raise _lib.GeoFormerHipError("train_merge: a voxel coordinate lies outside [0, 65535]")
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
    batch = {
        "locs": o["locs"][:N], "voxel_locs": out_coords[:M], "p2v_map": p.input_map[:N], "v2p_map": out_map[:M],
        "locs_float": o["locs_float"][:N], "feats": o["feats"][:N], "labels": o["labels"][:N],
        "instance_labels": o["instance_labels"][:N], "instance_pointnum": o["instance_pointnum"][:ninst],
        "instance_infos": o["instance_infos"][:N], "id": p.ids, "offsets": o["offsets"],
        "spatial_shape": np.asarray(head[H_SHAPE:H_SHAPE + 3], np.int64), "pc_mins": o["pc_mins"],
        "pc_maxs": o["pc_maxs"],
    }
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


def _queue_device(scenes, raw, sizes, dev, st, scale, full_scale, max_npoint, seed, batch_index):
    """rng="device": every launch of a batch up to the collate, on stream `st`, nothing read back."""
    lib = _lib.load()
    B = len(sizes)
    K = crop_candidates(full_scale[1])
    caps = np.array([device_cell_bounds(_radius(sc), scale) for sc in scenes], np.int64).T
    bt = _Batch(raw, sizes, dev, (3 * int(caps[0].sum()), 3 * int(caps[1].sum())))
    bt.rec.copy_(torch.from_numpy(_rec_init(B, caps)).pin_memory(), non_blocking=True)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    check(lib.gf_aug_draw(bt.ref, seed, int(batch_index), K, st), "gf_aug_draw")
    check(lib.gf_aug_transform(bt.ref, 0, B, float(scale), bt.max_scene, st), "gf_aug_transform")
    for p, (g, mg) in enumerate(elastic_params(scale)):
        check(lib.gf_aug_elastic(bt.ref, 0, B, p, int(g), float(mg), 1, seed, int(batch_index), bt.max_scene,
                                 int(caps[p].max()), st), "gf_aug_elastic")
    check(lib.gf_aug_crop(bt.ref, 0, B, int(full_scale[1]), K, int(max_npoint), bt.max_scene, st), "gf_aug_crop")
    return bt


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
    lib = _lib.load()
    st_obj = stream if stream is not None else torch.cuda.current_stream(dev)
    with torch.cuda.stream(st_obj):
        st = st_obj.cuda_stream
        raw, sizes = _raw_upload(scenes, dev)
        B = len(sizes)
        K = crop_candidates(full_scale[1])
        if K > MAX_CROP:
            raise ValueError(f"full_scale[1] allows at most {32 * (MAX_CROP - 1)}")
        (g0, m0), (g1, m1) = elastic_params(scale)
        draws = {"m": [], "flip": [], "theta": [], "noise": [], "crop_u": [], "chosen": [], "shift": [], "bb": [],
                 "blurred": []}
        if rng == "device":
            bt = _queue_device(scenes, raw, sizes, dev, st, scale, full_scale, max_npoint, seed, batch_index)
            if return_draws:
                torch.cuda.current_stream(dev).synchronize()
                rec = bt.rec.cpu().numpy()
                nz = [bt.noise[0].cpu().numpy(), bt.noise[1].cpu().numpy()]
                wk = [bt.work[0].cpu().numpy(), bt.work[1].cpu().numpy()]
                for s in range(B):
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
                    draws["shift"].append(r[R_SHIFT:R_SHIFT + 3].view(np.float64).copy())
        else:
            bt = _Batch(raw, sizes, dev, (1, 1))
            bt.rec.copy_(torch.from_numpy(_rec_init(B)))
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
                shift = (torch.randn(3) * 0.1).double().numpy()
                bt.rec[s, R_SHIFT:R_SHIFT + 3] = fdev(shift).view(torch.int64)
                for k, v in (("m", m), ("flip", int(flip)), ("theta", theta), ("noise", grids), ("crop_u", u),
                             ("chosen", chosen), ("shift", shift), ("bb", bbs), ("blurred", blurred)):
                    draws[k].append(v)
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
