"""numpy restatement of InstDataset.trainMerge (datasets/scannetv2_inst.py:142-232, 267-387), steps 2-11 of
geoformer_amd/augment.py, written from the reference's semantics without scipy: the yardstick of the GPU tests.

draws=None: the draws come from numpy's legacy global stream and torch's CPU generator in the reference's order;
otherwise they are replayed from a draws dict as train_merge(return_draws=True) returns it.  Instance-free scenes count
0 instances (the documented deviation from the reference's int(max) + 1 = -99).
"""
import math

import numpy as np
import torch

from geoformer_amd import augment, scene

W = np.float64(np.float32(1.0) / np.float32(3.0))  # the reference's fp32 box weights


def blur_axis(a, axis):
    """scipy.ndimage.convolve(a, ones(3)/3 along axis, mode="constant", cval=0) on fp32: fp64 taps -1, 0, +1, fp32 out."""
    a = a.astype(np.float64)
    pad = [(0, 0)] * 3
    pad[axis] = (1, 1)
    p = np.pad(a, pad)
    n = a.shape[axis]
    take = lambda o: np.take(p, np.arange(o, o + n), axis=axis)  # noqa: E731
    return (((0.0 + take(0) * W) + take(1) * W) + take(2) * W).astype(np.float32)


def blur6(g):
    for ax in (0, 1, 2, 0, 1, 2):
        g = blur_axis(g, ax)
    return g


def interp(grids, bb, gran, x):
    """scipy RegularGridInterpolator(linear, bounds_error=0, fill_value=0) of the three grids at x [n,3]."""
    axes = [np.linspace(-(b - 1) * gran, (b - 1) * gran, b) for b in bb]
    idx, t = [], []
    oob = np.zeros(x.shape[0], bool)
    for a in range(3):
        g = axes[a]
        i = np.clip(np.searchsorted(g, x[:, a], side="right") - 1, 0, bb[a] - 2)
        idx.append(i)
        t.append((x[:, a] - g[i]) / (g[i + 1] - g[i]))
        oob |= (x[:, a] < g[0]) | (x[:, a] > g[-1])
    out = np.zeros((x.shape[0], 3))
    for k, G in enumerate(grids):
        v = np.zeros(x.shape[0])
        for c in range(8):
            cs = ((c >> 2) & 1, (c >> 1) & 1, c & 1)
            w = np.ones(x.shape[0])
            for a in range(3):
                w = w * (t[a] if cs[a] else 1 - t[a])
            v = v + G[idx[0] + cs[0], idx[1] + cs[1], idx[2] + cs[2]].astype(np.float64) * w
        v[oob] = 0
        out[:, k] = v
    return out


def cropped_inst_label_loop(inst):
    """getCroppedInstLabel as the reference writes it (datasets/scannetv2_inst.py:224-232)."""
    inst = inst.copy()
    j = 0
    while j < inst.max():
        if len(np.where(inst == j)[0]) == 0:
            inst[inst == inst.max()] = j
        j += 1
    return inst


def cropped_inst_map(present):
    """The same mapping in closed form (what csrc/augment.hip k_relabel computes): with n ids present, ids below n keep
    their value and the k-th largest id >= n takes the k-th lowest hole below n."""
    present = np.unique(np.asarray(present, np.int64))
    n = present.size
    holes = np.setdiff1d(np.arange(n), present)
    big = present[present >= n][::-1]
    m = {int(i): int(i) for i in present[present < n]}
    m.update({int(b): int(h) for b, h in zip(big, holes)})
    return m


def instance_info(xyz, inst, n_inst):
    info = np.full((xyz.shape[0], 9), -100.0, np.float32)
    pointnum = []
    for i in range(n_inst):
        sel = np.where(inst == i)
        x = xyz[sel]
        info[sel[0], 0:3] = x.mean(0)
        info[sel[0], 3:6] = x.min(0)
        info[sel[0], 6:9] = x.max(0)
        pointnum.append(sel[0].size)
    return info, pointnum


def train_merge_numpy(scenes, draws=None, scale=50, full_scale=(128, 512), max_npoint=250000, cvfold=0, mode=4,
                      voxelise=True):
    """Returns (batch dict of numpy arrays, draws used, diagnostics {"bb", "blurred"})."""
    used = {"m": [], "flip": [], "theta": [], "noise": [], "crop_u": [], "chosen": [], "shift": []}
    diag = {"bb": [], "blurred": []}
    fold = augment.FOLD[cvfold]
    out = {k: [] for k in ("locs", "locs_float", "feats", "labels", "instance_labels", "instance_infos", "pc_mins",
                           "pc_maxs")}
    pointnum, offsets, total = [], [0], 0
    for s, data in enumerate(scenes):
        data = np.asarray(data, np.float64)
        xyz0, rgb = data[:, :3], data[:, 3:6]
        label, inst = data[:, 6].astype(np.int64), data[:, 7].astype(np.int64)
        if draws is None:
            m, g, flip, theta = augment._host_draw_m()
        else:
            m, flip, theta = draws["m"][s], draws["flip"][s], draws["theta"][s]
        xyz_middle = np.matmul(xyz0, m)
        xyz = xyz_middle * scale
        grids_used, bbs, blurred = [], [], []
        for p, (gran, mag) in enumerate(augment.elastic_params(scale)):
            bb = augment.grid_bb(np.abs(xyz).max(0), gran)
            if draws is None:
                noise = [np.random.randn(bb[0], bb[1], bb[2]).astype("float32") for _ in range(3)]
            else:
                noise = draws["noise"][s][p]
                assert tuple(noise[0].shape) == tuple(bb), (s, p, noise[0].shape, bb)
            bl = [blur6(n) for n in noise]
            xyz = xyz + interp(bl, bb, gran, xyz) * mag
            grids_used.append(noise)
            bbs.append(bb)
            blurred.append(bl)
        xyz -= xyz.min(0)
        # crop (datasets/scannetv2_inst.py:206-222)
        valid = np.ones(xyz.shape[0], bool)
        fs = np.array([full_scale[1]] * 3)
        rng_range = xyz.max(0) - xyz.min(0)
        us, k = [], 0
        while valid.sum() > max_npoint:
            u = np.random.rand(3) if draws is None else draws["crop_u"][s][k]
            us.append(u)
            offset = np.clip(fs - rng_range + 0.001, None, 0) * u
            xyz_off = xyz + offset
            valid = (xyz_off.min(1) >= 0) * ((xyz_off < fs).sum(1) == 3)
            fs[:2] -= 32
            k += 1
        if us:
            xyz = xyz_off
        chosen = len(us) - 1
        if draws is not None:
            assert chosen == draws["chosen"][s], (s, chosen, draws["chosen"][s])
        xyz_middle, xyz, rgb = xyz_middle[valid], xyz[valid], rgb[valid]
        label, inst = label[valid], inst[valid]
        l2 = np.full_like(label, -1)
        l2[label == 0] = 0
        l2[label == 1] = 1
        for i, c in enumerate(fold):
            l2[label == c] = i + 4
        l2[label == -100] = 2
        l2[l2 == -1] = 3
        label = l2
        inst[label <= 3] = -100
        inst = cropped_inst_label_loop(inst) if inst.size else inst
        n_inst = int(inst.max()) + 1 if (inst >= 0).any() else 0  # the deviation: 0, not -99
        info, pn = instance_info(xyz_middle, inst.astype(np.int32), n_inst)
        inst[inst != -100] += total
        total += n_inst
        if draws is None:
            shift = (torch.randn(3) * 0.1).double().numpy()
        else:
            shift = np.asarray(draws["shift"][s], np.float64)
        offsets.append(offsets[-1] + xyz.shape[0])
        out["locs"].append(np.concatenate([np.full((xyz.shape[0], 1), s, np.int64), xyz.astype(np.int64)], 1))
        out["locs_float"].append(xyz_middle.astype(np.float32))
        out["feats"].append(rgb + shift)
        out["labels"].append(label)
        out["instance_labels"].append(inst)
        out["instance_infos"].append(info)
        out["pc_mins"].append(xyz_middle.min(0).astype(np.float32))
        out["pc_maxs"].append(xyz_middle.max(0).astype(np.float32))
        pointnum += pn
        for k_, v in (("m", m), ("flip", int(flip)), ("theta", theta), ("noise", grids_used),
                      ("crop_u", np.array(us).reshape(-1, 3)), ("chosen", chosen), ("shift", shift)):
            used[k_].append(v)
        diag["bb"].append(bbs)
        diag["blurred"].append(blurred)
    b = {k: (np.stack(v) if k in ("pc_mins", "pc_maxs") else np.concatenate(v)) for k, v in out.items()}
    b["instance_pointnum"] = np.asarray(pointnum, np.int32)
    b["offsets"] = np.asarray(offsets, np.int32)
    b["spatial_shape"] = np.clip(b["locs"].max(0)[1:] + 1, full_scale[0], None)
    if voxelise:
        b["voxel_locs"], b["p2v_map"], b["v2p_map"] = scene.voxelize_host(b["locs"], mode)
    return b, used, diag


INT_KEYS = ("locs", "voxel_locs", "p2v_map", "v2p_map", "labels", "instance_labels", "instance_pointnum", "offsets",
            "spatial_shape")
FLOAT_KEYS = ("locs_float", "instance_infos", "pc_mins", "pc_maxs", "feats")


def compare(got, want, tol=1e-6):
    """Integer fields exactly, float fields to tol; returns a list of mismatch descriptions."""
    bad = []
    for k in INT_KEYS:
        if k not in want:
            continue
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if g.shape != w.shape or not (g.astype(np.int64) == w.astype(np.int64)).all():
            bad.append(f"{k}: shape {g.shape} vs {w.shape}" if g.shape != w.shape else f"{k}: {(g != w).sum()} differ")
    for k in FLOAT_KEYS:
        g, w = np.asarray(got[k], np.float64), np.asarray(want[k], np.float64)
        if g.shape != w.shape:
            bad.append(f"{k}: shape {g.shape} vs {w.shape}")
        elif g.size and np.abs(g - w).max() > tol:
            bad.append(f"{k}: max diff {np.abs(g - w).max()}")
    return bad
