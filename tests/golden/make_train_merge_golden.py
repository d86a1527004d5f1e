"""Golden fixture of the training collate, produced by the REFERENCE's own InstDataset.trainMerge
(datasets/scannetv2_inst.py:267-387, imported from the reference checkout; nothing is copied).

    python tests/golden/make_train_merge_golden.py [/path/to/reference]   -> tests/golden/train_merge.npz

Three workarounds let the reference's loader run here: ``np.int = int`` (numpy 2 removed it), a ``datasets`` package
pinned to the reference's directory (the HF ``datasets`` package would shadow it), and an InstDataset made with
``__new__`` plus the attributes trainMerge reads (no data root, no split files).  pointgroup_ops.voxelization_idx runs
on the CPU oracle (ref_shims).  Besides inputs, seeds and outputs the fixture keeps both generators' final states and,
recorded around ``elastic``, every noise grid's extents and its blurred values.  A case is re-seeded until no
pre-floor coordinate lies within 1e-7 of an integer (0 itself, the minimum, is exact) and no |x| max lies within 1e-7
of an integer, so integer outputs can be required to match exactly.

Cases: "crop"  batch 2, cvfold 0, max_npoint lowered: several crop iterations;
       "plain" batch 3, cvfold 1, no crop, the last scene without instances (the deviation: 0 instances, not -99).
"""
import os
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
sys.argv = ["make_train_merge_golden", "--config", os.path.join(REF, "config/geoformer_scannet.yaml")]

import numpy as np  # noqa: E402
import scipy.interpolate  # noqa: E402
import torch  # noqa: E402

from tests.golden import ref_shims  # noqa: E402

ref_shims.install(REF)
np.int = int
pkg = types.ModuleType("datasets")
pkg.__path__ = [os.path.join(REF, "datasets")]
sys.modules["datasets"] = pkg
from datasets.scannetv2_inst import InstDataset  # noqa: E402

from datasets.scannetv2 import FOLD  # noqa: E402
from geoformer_amd import scene  # noqa: E402

# (points, seed, instances, room): small rooms keep the noise grids small; the crop case's rooms are narrower than
# full_scale, so its loop runs a dozen iterations before it bites
CASES = {
    "crop": dict(scenes=[(1400, 101, True, (2.2, 1.8, 1.2)), (1100, 102, True, (2.0, 1.8, 1.2))], cvfold=0,
                 max_npoint=700),
    "plain": dict(scenes=[(900, 201, True, (1.8, 1.6, 1.2)), (1000, 202, True, (2.0, 1.6, 1.2)),
                          (700, 203, False, (1.6, 1.6, 1.2))], cvfold=1, max_npoint=250000),
}
# stored compactly, every value exact except the fp64 colours (feats, compared to 1e-6: fp32 is within 1e-7); the
# reference's dtypes are recorded and restored by tests/test_augment_host.py:golden_case
_STORE = {"locs": np.int16, "voxel_locs": np.int16, "p2v_map": np.int32, "v2p_map": np.int32, "labels": np.int8,
          "instance_labels": np.int16, "feats": np.float32}

_rec = {"grids": [], "amax": [], "crop": []}
_RGI = scipy.interpolate.RegularGridInterpolator


def _rgi(points, values, *a, **k):
    _rec["grids"].append(np.array(values))
    return _RGI(points, values, *a, **k)


scipy.interpolate.RegularGridInterpolator = _rgi


def dataset(files, cvfold, max_npoint):
    ds = InstDataset.__new__(InstDataset)
    ds.batch_size, ds.full_scale, ds.scale, ds.max_npoint, ds.mode = len(files), [128, 512], 50, max_npoint, 4
    ds.file_names = files
    ds.SEMANTIC_LABELS = FOLD[cvfold]
    el, cr = ds.elastic, ds.crop

    def elastic(x, gran, mag):
        _rec["amax"].append(np.abs(x).max(0))
        return el(x, gran, mag)

    def crop(xyz):
        r = cr(xyz)
        _rec["crop"].append(r[0].copy())
        return r

    ds.elastic, ds.crop = elastic, crop
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


def main():
    out = {}
    tmp = tempfile.mkdtemp()
    for name, c in CASES.items():
        raws = [scene.make_raw_scene(n, sd, instances=inst, room=room) for (n, sd, inst, room) in c["scenes"]]
        files = []
        for i, r in enumerate(raws):
            f = os.path.join(tmp, f"{name}_{i}.npy")
            np.save(f, r)
            files.append(f)
        for seed in range(1000):
            _rec["grids"].clear(), _rec["amax"].clear(), _rec["crop"].clear()
            np.random.seed(seed)
            torch.manual_seed(seed + 1)
            batch = dataset(files, c["cvfold"], c["max_npoint"]).trainMerge(list(range(len(files))))
            if margins_ok():
                break
        else:
            raise RuntimeError(f"{name}: no seed with clear margins")
        print(name, "seed", seed, "points", [r.shape[0] for r in raws], "kept", batch["offsets"].tolist())
        st = np.random.get_state()
        p = name + "/"
        raw = np.concatenate(raws)
        xyzrgb, labinst = raw[:, :6].astype(np.float32), raw[:, 6:].astype(np.int16)
        assert (xyzrgb.astype(np.float64) == raw[:, :6]).all() and (labinst.astype(np.float64) == raw[:, 6:]).all()
        out[p + "raw_xyzrgb"], out[p + "raw_labinst"] = xyzrgb, labinst
        out[p + "sizes"] = np.array([r.shape[0] for r in raws], np.int64)
        out[p + "numpy_seed"], out[p + "torch_seed"] = np.int64(seed), np.int64(seed + 1)
        out[p + "cvfold"], out[p + "max_npoint"] = np.int64(c["cvfold"]), np.int64(c["max_npoint"])
        out[p + "np_state_key"], out[p + "np_state_pos"] = st[1], np.int64(st[2])
        out[p + "np_state_gauss"] = np.array([st[3], st[4]], np.float64)
        out[p + "torch_state"] = torch.get_rng_state().numpy()
        for k, v in batch.items():
            if k == "id":
                continue
            v = v.numpy() if torch.is_tensor(v) else np.asarray(v)
            out[p + "dtype_" + k] = np.array(str(v.dtype))
            if k in _STORE:
                w = v.astype(_STORE[k])
                assert k == "feats" or (w == v).all(), k
                v = w
            out[p + k] = v
        for i, g in enumerate(_rec["grids"]):  # per scene: pass 0 x/y/z, pass 1 x/y/z
            out[p + f"blurred_{i}"] = g
    np.savez_compressed(os.path.join(HERE, "train_merge.npz"), **out)


if __name__ == "__main__":
    main()
