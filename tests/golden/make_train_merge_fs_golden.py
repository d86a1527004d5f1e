"""Golden fixture of the few-shot training episode, produced by the REFERENCE's own FSInstDataset.trainMergeFS
(datasets/scannetv2_fs_inst.py:330-365, 397-566) and its class tables (datasets/scannetv2.py:75-159, ScanNetDataset's
get_class2scans / get_class2instances), imported from the reference checkout; nothing is copied.

    python tests/golden/make_train_merge_fs_golden.py [/path/to/reference]   -> tests/golden/train_merge_fs.npz

The workarounds of make_train_merge_golden.py: ``np.int = int``, a ``datasets`` package pinned to the reference's
directory, datasets made with ``__new__`` plus the attributes the methods read, pointgroup_ops.voxelization_idx on the
CPU oracle (ref_shims).  The synthetic scenes are written to a temporary data root, where the reference's builders make
the class tables and load_single reads them.  Recorded: the scenes, the tables (class2scans in the builder's glob
order), the per-scene nonzero-label counts, and per case the seed (random, numpy and torch seeded with it), the three
generators' final states, both dicts (values and dtypes) and scene_infos.  The support dict's feats and locs_float are
the support scenes' raw rows (asserted here) and are rebuilt from the scenes on load rather than stored twice.  A case's seed is searched until its
conditions hold and no pre-floor query coordinate or |x| max lies within 1e-7 of an integer (as in the trainMerge
golden), so integer outputs can be required to match exactly.

Cases: "crop"    batch 4, max_npoint lowered: a crop with several iterations, and a query whose sampled class the crop
                 removed entirely (its labels all 0, no instances);
       "episode" batch 6, no crop: a support draw retried (a listed scene with <= 100 nonzero labels, "retry") and a
                 query scene drawn twice.
"""
import os
import random
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
sys.argv = ["make_train_merge_fs_golden", "--config", os.path.join(REF, "config/geoformer_fs_scannet.yaml")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests.golden import ref_shims  # noqa: E402

ref_shims.install(REF)
np.int = int
pkg = types.ModuleType("datasets")
pkg.__path__ = [os.path.join(REF, "datasets")]
sys.modules["datasets"] = pkg
from datasets.scannetv2 import FOLD, ScanNetDataset  # noqa: E402
from datasets.scannetv2_fs_inst import FSInstDataset  # noqa: E402

from geoformer_amd import scene  # noqa: E402

CVFOLD = 0
# (name, points, seed, boxes, room): every class of fold 0 lists scenes and instances
SCENES = [(f"scene{i:04d}_00", n, 700 + i, 3, (1.2, 1.0, 0.6)) for i, n in enumerate((950, 850, 1000, 900, 800, 900))]
RETRY = "scene0099_00"  # one listed instance, but only its first point labelled: <= 100 nonzero labels in the scene
CASES = {"crop": dict(batch=4, max_npoint=400), "episode": dict(batch=6, max_npoint=250000)}
_STORE = {"locs": np.int16, "voxel_locs": np.int16, "p2v_map": np.int32, "v2p_map": np.int32, "labels": np.int8,
          "instance_labels": np.int16, "support_masks": np.int8, "feats": np.float32}

_rec = {"amax": [], "crop": [], "support": 0}


def make_scenes():
    out = {}
    classes = FOLD[CVFOLD]
    k = 0
    for name, n, sd, boxes, room in SCENES:
        r = scene.make_raw_scene(n, sd, n_boxes=boxes, room=room)
        ins = r[:, 7]
        for b in np.unique(ins[ins >= 0]):  # the fold's classes in turn
            r[(ins == b) & (r[:, 6] != -100), 6] = classes[k % len(classes)]
            k += 1
        out[name] = r
    r = scene.make_raw_scene(900, 799, n_boxes=1, room=(1.2, 1.0, 0.6))
    ins = r[:, 7]
    box = ins == np.unique(ins[ins >= 0])[0]
    r[r[:, 6] != -100, 6] = 0
    r[np.flatnonzero(box)[0], 6] = classes[0]
    out[RETRY] = r
    return out


def tables(root, names):
    ds = ScanNetDataset.__new__(ScanNetDataset)
    ds.data_path, ds.classes = root, 20
    ds.class2type = {i: str(i) for i in range(20)}
    return ds.get_class2scans(block=False), ds.get_class2instances()


def dataset(root, c2s, c2i, batch, max_npoint):
    ds = FSInstDataset.__new__(FSInstDataset)
    ds.data_root, ds.dataset = os.path.dirname(root), os.path.basename(root)
    ds.batch_size, ds.full_scale, ds.scale, ds.max_npoint, ds.mode = batch, [128, 512], 50, max_npoint, 4
    ds.SEMANTIC_LABELS = FOLD[CVFOLD]
    ds.class2scans_scenes, ds.class2instances = c2s, c2i
    el, cr, ls = ds.elastic, ds.crop, ds.load_single

    def elastic(x, gran, mag):
        _rec["amax"].append(np.abs(x).max(0))
        return el(x, gran, mag)

    def crop(xyz):
        r = cr(xyz)
        _rec["crop"].append(r[0].copy())
        return r

    def load_single(name, aug=True, permutate=True, val=False, support=False):
        _rec["support"] += bool(support)
        return ls(name, aug=aug, permutate=permutate, val=val, support=support)

    ds.elastic, ds.crop, ds.load_single = elastic, crop, load_single
    return ds


def margins_ok():
    for a in _rec["amax"]:
        if (np.abs(a - np.round(a)) < 1e-7).any():
            return False
    for x in _rec["crop"]:
        d = np.abs(x - np.round(x))
        if ((d < 1e-7) & (x != 0)).any():
            return False
    return True


def conditions(name, batch, sup, query, infos, raws):
    off = query["batch_offsets"].numpy()
    if name == "crop":
        cropped = [i for i, inf in enumerate(infos)
                   if query["labels"][off[i]:off[i + 1]].sum() == 0
                   and (raws[inf["query_scene"]][:, 6] == inf["sampled_class"]).any()]
        return bool(cropped) and len(_rec["crop"]) == batch
    qs = [inf["query_scene"] for inf in infos]
    return _rec["support"] > batch and len(set(qs)) < len(qs)


def main():
    out = {}
    tmp = tempfile.mkdtemp()
    root = os.path.join(tmp, "scannetv2")
    os.makedirs(os.path.join(root, "scenes"))
    raws = make_scenes()
    for name, r in raws.items():
        np.save(os.path.join(root, "scenes", name + ".npy"), r)
    c2s, c2i = tables(root, list(raws))
    for c in FOLD[CVFOLD]:
        assert c2s[c] and c2i[c], (c, c2s[c], c2i[c])
    assert RETRY in [s for s, _ in c2i[FOLD[CVFOLD][0]]] and np.count_nonzero(raws[RETRY][:, 6].astype(int)) <= 100
    names = sorted(raws)
    raw = np.concatenate([raws[n] for n in names])
    xyzrgb, labinst = raw[:, :6].astype(np.float32), raw[:, 6:].astype(np.int16)
    assert (xyzrgb.astype(np.float64) == raw[:, :6]).all() and (labinst.astype(np.float64) == raw[:, 6:]).all()
    out["names"] = np.array(names)
    out["sizes"] = np.array([raws[n].shape[0] for n in names], np.int64)
    out["raw_xyzrgb"], out["raw_labinst"] = xyzrgb, labinst
    out["counts"] = np.array([np.count_nonzero(raws[n][:, 6].astype(int)) for n in names], np.int64)
    for c in range(20):
        out[f"c2s_{c}"] = np.array(c2s[c], dtype="U12")
        out[f"c2i_{c}_scene"] = np.array([s for s, _ in c2i[c]], dtype="U12")
        out[f"c2i_{c}_id"] = np.array([i for _, i in c2i[c]], np.int64)
    for name, c in CASES.items():
        for seed in range(5000):
            _rec["amax"].clear(), _rec["crop"].clear()
            _rec["support"] = 0
            random.seed(seed)
            np.random.seed(seed)
            torch.manual_seed(seed)
            sup, query, infos = dataset(root, c2s, c2i, c["batch"], c["max_npoint"]).trainMergeFS(
                list(range(c["batch"])))
            if margins_ok() and conditions(name, c["batch"], sup, query, infos, raws):
                break
        else:
            raise RuntimeError(f"{name}: no seed meets the conditions")
        print(name, "seed", seed, "support loads", _rec["support"], "kept", query["batch_offsets"].tolist(),
              [(i["sampled_class"], i["query_scene"], i["support_scene"], int(i["support_instance_id"])) for i in infos])
        p = name + "/"
        out[p + "seed"], out[p + "batch"], out[p + "max_npoint"] = (np.int64(seed), np.int64(c["batch"]),
                                                                     np.int64(c["max_npoint"]))
        rs = random.getstate()
        assert rs[2] is None
        out[p + "random_state"] = np.array(rs[1], np.int64)
        st = np.random.get_state()
        out[p + "np_state_key"], out[p + "np_state_pos"] = st[1], np.int64(st[2])
        out[p + "np_state_gauss"] = np.array([st[3], st[4]], np.float64)
        out[p + "torch_state"] = torch.get_rng_state().numpy()
        out[p + "info_class"] = np.array([i["sampled_class"] for i in infos], np.int64)
        out[p + "info_query"] = np.array([i["query_scene"] for i in infos], dtype="U12")
        out[p + "info_support"] = np.array([i["support_scene"] for i in infos], dtype="U12")
        out[p + "info_id"] = np.array([i["support_instance_id"] for i in infos], np.int64)
        rows = np.concatenate([raws[i["support_scene"]] for i in infos])
        assert (sup["feats"].numpy() == rows[:, 3:6]).all()
        assert (sup["locs_float"].numpy() == rows[:, :3].astype(np.float32)).all()
        for part, d in (("support", sup), ("query", query)):
            out[p + part + "_keys"] = np.array(list(d))
            for k, v in d.items():
                v = v.numpy() if torch.is_tensor(v) else np.asarray(v)
                q = p + part + "/"
                out[q + "dtype_" + k] = np.array(str(v.dtype))
                if part == "support" and k in ("feats", "locs_float"):
                    continue
                if k in _STORE:
                    w = v.astype(_STORE[k])
                    assert k == "feats" or (w == v).all(), k
                    v = w
                out[q + k] = v
    np.savez_compressed(os.path.join(HERE, "train_merge_fs.npz"), **out)


if __name__ == "__main__":
    main()
