"""numpy restatement of FSInstDataset.trainMergeFS (datasets/scannetv2_fs_inst.py:330-365, 397-566) and of the class
tables it samples from (datasets/scannetv2.py:75-159), written from the reference's semantics on top of
tests/augment_numpy.py's elastic pieces: the yardstick of the few-shot GPU tests.

draws=None: the choices come from Python's random and the augmentation from numpy's legacy stream, in the reference's
order; otherwise both are replayed (scene_infos and a draws dict as train_merge_fs(return_draws=True) returns them).
"""
import random

import numpy as np

from geoformer_amd import augment, scene
from tests import augment_numpy as an

INT_KEYS = ("locs", "voxel_locs", "p2v_map", "v2p_map", "labels", "instance_labels", "instance_pointnum",
            "batch_offsets", "spatial_shape", "support_masks")
FLOAT_KEYS = ("locs_float", "feats", "pc_mins", "pc_maxs")


def tables(scenes_by_name):
    """class2scans (scenes in the mapping's order), class2instances (scenes sorted, ids ascending), nonzero counts."""
    c2s = {k: [] for k in range(20)}
    c2i = {k: [] for k in range(20)}
    counts = {}
    for name, data in scenes_by_name.items():
        labels = data[:, 6].astype(np.int64)
        counts[name] = int(np.count_nonzero(labels))
        for c in np.unique(labels):
            if c != -100 and np.count_nonzero(labels == c) > max(int(data.shape[0] * 0.05), 100):
                c2s[int(c)].append(name)
    for name in sorted(scenes_by_name):
        data = scenes_by_name[name]
        labels, inst = data[:, 6].astype(np.int64), data[:, 7].astype(np.int64)
        for i in np.unique(inst):
            if i == -100:
                continue
            n = np.count_nonzero(inst == i)
            c = labels[(inst == i).nonzero()[0][0]]
            if n > max(int(data.shape[0] * 0.002), 100) and c != -100:
                c2i[int(c)].append([name, i])
    return c2s, c2i, counts


def sample(c2s, c2i, counts, batch_size, cvfold=0):
    """The reference's random.choice calls, item by item."""
    infos = []
    for _ in range(batch_size):
        c = random.choice(augment.FOLD[cvfold])
        q = random.choice(c2s[c])
        while True:
            s, i = random.choice(c2i[c])
            if counts[s] > 100:
                break
        infos.append({"sampled_class": c, "query_scene": q, "support_scene": s, "support_instance_id": i})
    return infos


def load_query(data, cls, s, draws, scale, full_scale, max_npoint, used):
    """load_single(aug=True) + the query's labels: (xyz_middle, xyz, rgb, label 0/1, instance ids 0..n-1 or -100)."""
    xyz0, rgb = data[:, :3], data[:, 3:6]
    label, inst = data[:, 6].astype(np.int64), data[:, 7].astype(np.int64)
    if draws is None:
        m, _, flip, theta = augment._host_draw_m()
    else:
        m, flip, theta = draws["m"][s], draws["flip"][s], draws["theta"][s]
    xyz_middle = np.matmul(xyz0, m)
    xyz = xyz_middle * scale
    grids = []
    for p, (gran, mag) in enumerate(augment.elastic_params(scale)):
        bb = augment.grid_bb(np.abs(xyz).max(0), gran)
        if draws is None:
            noise = [np.random.randn(bb[0], bb[1], bb[2]).astype("float32") for _ in range(3)]
        else:
            noise = draws["noise"][s][p]
            assert tuple(noise[0].shape) == tuple(bb), (s, p, noise[0].shape, bb)
        xyz = xyz + an.interp([an.blur6(n) for n in noise], bb, gran, xyz) * mag
        grids.append(noise)
    xyz -= xyz.min(0)
    valid = np.ones(xyz.shape[0], bool)
    fs = np.array([full_scale[1]] * 3)
    room = xyz.max(0) - xyz.min(0)
    us = []
    xyz_off = xyz
    while valid.sum() > max_npoint:
        u = np.random.rand(3) if draws is None else draws["crop_u"][s][len(us)]
        us.append(u)
        xyz_off = xyz + np.clip(fs - room + 0.001, None, 0) * u
        valid = (xyz_off.min(1) >= 0) * ((xyz_off < fs).sum(1) == 3)
        fs[:2] -= 32
    if draws is not None:
        assert len(us) - 1 == draws["chosen"][s], (s, len(us) - 1, draws["chosen"][s])
    xyz_middle, xyz, rgb = xyz_middle[valid], xyz_off[valid], rgb[valid]
    label, inst = label[valid] == cls, inst[valid]
    inst[label == 0] = -100
    inst = an.cropped_inst_label_loop(inst) if inst.size else inst
    for k, v in (("m", m), ("flip", int(flip)), ("theta", theta), ("noise", grids),
                 ("crop_u", np.array(us).reshape(-1, 3)), ("chosen", len(us) - 1)):
        used[k].append(v)
    return xyz_middle, xyz, rgb, label, inst


def train_merge_fs_numpy(scene_of, c2s, c2i, counts, batch_size, infos=None, draws=None, cvfold=0, scale=50,
                         full_scale=(128, 512), max_npoint=250000, mode=4):
    """Returns (support dict, query dict, scene_infos, draws used), numpy arrays."""
    if infos is None:
        infos = sample(c2s, c2i, counts, batch_size, cvfold)
    used = {"m": [], "flip": [], "theta": [], "noise": [], "crop_u": [], "chosen": []}
    q = {k: [] for k in ("locs", "locs_float", "feats", "labels", "instance_labels", "pc_mins", "pc_maxs")}
    sp = {k: [] for k in ("locs", "locs_float", "feats", "support_masks", "pc_mins", "pc_maxs")}
    pointnum, q_off, s_off = [], [0], [0]
    for s, inf in enumerate(infos):
        data = np.asarray(scene_of[inf["query_scene"]], np.float64)
        xm, xyz, rgb, label, inst = load_query(data, inf["sampled_class"], s, draws, scale, full_scale, max_npoint,
                                               used)
        n_inst = int(inst.max()) + 1 if inst.size else 0
        pointnum += [int((inst == i).sum()) for i in range(n_inst)]  # (none when int(max) + 1 <= 0)
        q_off.append(q_off[-1] + xyz.shape[0])
        q["locs"].append(np.concatenate([np.full((xyz.shape[0], 1), s, np.int64), xyz.astype(np.int64)], 1))
        q["locs_float"].append(xm.astype(np.float32))
        q["feats"].append(rgb)
        q["labels"].append(label.astype(np.int64))
        q["instance_labels"].append(inst)  # + total_inst_num, which stays 0
        q["pc_mins"].append(xm.min(0).astype(np.float32))
        q["pc_maxs"].append(xm.max(0).astype(np.float32))
        sd = np.asarray(scene_of[inf["support_scene"]], np.float64)
        sxyz = sd[:, :3] * scale
        sxyz -= sxyz.min(0)
        s_off.append(s_off[-1] + sd.shape[0])
        sp["locs"].append(np.concatenate([np.full((sd.shape[0], 1), s, np.int64), sxyz.astype(np.int64)], 1))
        sp["locs_float"].append(sd[:, :3].astype(np.float32))
        sp["feats"].append(sd[:, 3:6])
        sp["support_masks"].append((sd[:, 7].astype(np.int64) == inf["support_instance_id"]).astype(np.int64))
        sp["pc_mins"].append(sd[:, :3].min(0).astype(np.float32))
        sp["pc_maxs"].append(sd[:, :3].max(0).astype(np.float32))
    out = []
    for d, off in ((sp, s_off), (q, q_off)):
        b = {k: (np.stack(v) if k in ("pc_mins", "pc_maxs") else np.concatenate(v)) for k, v in d.items()}
        b["batch_offsets"] = np.asarray(off, np.int32)
        b["spatial_shape"] = np.clip(b["locs"].max(0)[1:] + 1, full_scale[0], None)
        b["voxel_locs"], b["p2v_map"], b["v2p_map"] = scene.voxelize_host(b["locs"], mode)
        out.append(b)
    out[1]["instance_pointnum"] = np.asarray(pointnum, np.int32)
    return out[0], out[1], infos, used


def compare(got, want, tol=1e-6):
    """Integer fields exactly, float fields to tol, for the keys both have; returns a list of mismatches."""
    bad = []
    for k in INT_KEYS + FLOAT_KEYS:
        if k not in want or k not in got:
            continue
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if g.shape != w.shape:
            bad.append(f"{k}: shape {g.shape} vs {w.shape}")
        elif k in INT_KEYS and not (g.astype(np.int64) == w.astype(np.int64)).all():
            bad.append(f"{k}: {(g.astype(np.int64) != w.astype(np.int64)).sum()} differ")
        elif k in FLOAT_KEYS and g.size and np.abs(g.astype(np.float64) - w.astype(np.float64)).max() > tol:
            bad.append(f"{k}: max diff {np.abs(g.astype(np.float64) - w.astype(np.float64)).max()}")
    return bad
