"""Golden fixture of the few-shot TEST path, produced by the REFERENCE's own code imported from its checkout (nothing is
copied): FSInstDataset.get_support_set / get_test_comb / testMergeFS (datasets/scannetv2_fs_inst.py:80-183, 568-700),
test_fs.load_set_support (test_fs.py:33-112, with a stub model whose process_support records the dicts), and the eval
tail: util/utils_3d.matrix_non_max_suppression and util/eval.py (assign_instances_for_scan, evaluate_matches,
compute_averages, accumulate_averages_over_runs, compute_averages_over_runs).

    python tests/golden/make_test_merge_fs_golden.py [/path/to/reference]   -> tests/golden/test_merge_fs.npz

The workarounds of make_train_merge_fs_golden.py (ref_shims, np.int = int, a ``datasets`` package pinned to the
reference's directory, datasets made with ``__new__``), plus np.float = float for util/eval.py.  The config is the
shipped test yaml (cvfold 1) with run_num lowered to RUN_NUM.  Synthetic scenes are written to a temporary data root;
their instances are the points nearest to a centre, so the region block of an instance holds other points too.

Recorded: the scenes, the class tables, the support sets and test combinations of both generation orders ("both": no
pickle, support sets first and the combinations continuing their random stream; "comb": support sets loaded, the
combinations after random.seed(test_seed)), whether a support draw was retried under the 1000-point rule, testMergeFS
for every val scene (the query with fix_support True, asserted equal with False; the block supports of False with the
rows they keep; values and dtypes; a scene without active label is invalid), the
full-scene support dicts load_set_support hands process_support (the first CAPTURE of run 0), and per run the reference's
NMS picks and AP summaries of recorded proposal sets, one scene without a proposal in some runs.
"""
import os
import pickle
import random
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
sys.argv = ["make_test_merge_fs_golden", "--config", os.path.join(REF, "config/test_geoformer_fs_scannet.yaml")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests.golden import ref_shims  # noqa: E402

ref_shims.install(REF)
np.int = int
np.float = float
pkg = types.ModuleType("datasets")
pkg.__path__ = [os.path.join(REF, "datasets")]
sys.modules["datasets"] = pkg
from util.config import cfg  # noqa: E402
from datasets.scannetv2 import BENCHMARK_SEMANTIC_LABELS, FOLD, ScanNetDataset  # noqa: E402
from datasets.scannetv2_fs_inst import FSInstDataset  # noqa: E402
import util.eval as ref_eval  # noqa: E402
from util.utils_3d import matrix_non_max_suppression  # noqa: E402

from geoformer_amd import scene  # noqa: E402

RUN_NUM = 3
CAPTURE = 2
CV = cfg.cvfold
CLS = FOLD[CV]
# support scenes: (name, seed, [(class, points)]): every class of the fold has an instance of >= 1000 points; class
# CLS[0]'s list also holds a small instance (a draw retried under the 1000-point rule)
SUPPORT = [("scene0100_00", 11, [(CLS[0], 1050), (CLS[1], 1010), (CLS[0], 150)]),
           ("scene0101_00", 12, [(CLS[2], 1020), (CLS[3], 1000), (CLS[0], 160), (CLS[0], 170)]),
           ("scene0102_00", 13, [(CLS[4], 1030), (CLS[5], 1040), (CLS[1], 180)]),
           ("scene0103_00", 14, [(CLS[6], 1010), (CLS[7], 1060)]),
           ("scene0104_00", 15, [(CLS[8], 1005), (CLS[0], 1001), (CLS[3], 140)])]
SUPPORT_POINTS = 2400
# val scenes: (name, seed, points, [(class, points)]); the last holds no class of the fold
VAL = [("scene0500_00", 21, 1500, [(CLS[0], 300), (CLS[3], 250), (CLS[0], 200), (CLS[7], 180)]),
       ("scene0501_00", 22, 1300, [(CLS[1], 400), (CLS[8], 220)]),
       ("scene0502_00", 23, 1400, [(CLS[2], 350), (CLS[5], 260), (CLS[6], 150)]),
       ("scene0503_00", 24, 900, [(2, 300), (3, 200)])]


def make(n, seed, insts):
    """A raw [n, 8] scene: make_raw_scene's points and colours; instance k = the insts[k][1] unassigned points nearest
    to a random centre, label insts[k][0]; the rest floor / wall (no instance), ~3 % unannotated."""
    r = scene.make_raw_scene(n, seed, n_boxes=2, room=(1.2, 1.0, 0.6))
    n = r.shape[0]
    rng = np.random.default_rng(seed + 1)
    lab = np.where(r[:, 2] < np.quantile(r[:, 2], 0.2), 0, 1).astype(np.float64)
    ins = np.full(n, -100.0)
    free = np.ones(n, bool)
    for k, (c, m) in enumerate(insts):
        ctr = r[rng.integers(n), :3]
        d = np.where(free, ((r[:, :3] - ctr) ** 2).sum(1), np.inf)
        sel = np.argsort(d, kind="stable")[:m]
        lab[sel], ins[sel] = c, 3 * k + 1  # ids with holes
        free[sel] = False
    un = free & (rng.random(n) < 0.03)
    lab[un], ins[un] = -100, -100
    r[:, 6], r[:, 7] = lab, ins
    return r


def dataset(root, c2i, names):
    ds = FSInstDataset.__new__(FSInstDataset)
    ds.data_root, ds.dataset = os.path.dirname(root), os.path.basename(root)
    ds.batch_size, ds.full_scale, ds.scale, ds.max_npoint, ds.mode = 1, cfg.full_scale, cfg.scale, cfg.max_npoint, 4
    ds.SEMANTIC_LABELS = CLS
    ds.class2instances = c2i
    ds.file_names = [os.path.join(root, "scenes", n + ".npy") for n in names]
    ds.test_names = list(names)
    return ds


_loads = [0]


def counting(ds):
    ls = ds.load_single

    def load_single(name, aug=True, permutate=True, val=False, support=False):
        _loads[0] += 1
        return ls(name, aug=aug, permutate=permutate, val=val, support=support)

    ds.load_single = load_single
    return ds


def store(out, prefix, d, rows):
    """A dict's keys, dtypes and values; locs_float and feats are the float32 of `rows` (raw rows, asserted) and are
    rebuilt from the scenes on load rather than stored twice."""
    out[prefix + "keys"] = np.array(list(d))
    for k, v in d.items():
        v = v.numpy() if torch.is_tensor(v) else np.asarray(v)
        out[prefix + "dtype_" + k] = np.array(str(v.dtype))
        if k in ("locs_float", "feats"):
            assert v.dtype == np.float32 and (v == rows[:, slice(0, 3) if k == "locs_float" else slice(3, 6)]
                                              .astype(np.float32)).all(), k
            continue
        if v.dtype == np.int64 and v.size and np.abs(v).max() < 2 ** 15:
            v = v.astype(np.int16)
        out[prefix + k] = v


def sets_array(ss):
    """support sets -> [run, class, shot] scene names and ids"""
    names = np.array([[[t[0] for t in run[c]] for c in CLS] for run in ss], dtype="U12")
    ids = np.array([[[int(t[1]) for t in run[c]] for c in CLS] for run in ss], np.int64)
    return names, ids


def combs_arrays(out, prefix, combs, names):
    for n in names:
        c = combs[n]
        out[prefix + n + "/active"] = np.array([int(l) for l in c["active_label"]], np.int64)
        out[prefix + n + "/scene"] = np.array([c[l][0] for l in c["active_label"]], dtype="U12")
        out[prefix + n + "/id"] = np.array([int(c[l][1]) for l in c["active_label"]], np.int64)


def proposals(raws, names):
    """Recorded proposal sets per run and scene: masks around the GT instances (grown / shrunk / shifted), a duplicate
    and a background mask, scores in [0.4, 1), categories the instances' nyu40 ids; val scene 1 has none in run 1."""
    rng = np.random.default_rng(20261016)
    runs = []
    for k in range(RUN_NUM):
        per = {}
        for si, n in enumerate(names):
            r = raws[n]
            N = r.shape[0]
            if k == 1 and si == 1:
                per[n] = None
                continue
            masks, cats = [], []
            for i in np.unique(r[:, 7][r[:, 7] >= 0]):
                m = r[:, 7] == i
                lab = int(r[m, 6][0])
                for _ in range(int(rng.integers(1, 3))):
                    mm = m.copy()
                    flip = rng.random(N) < rng.uniform(0.0, 0.25)
                    mm[flip & (rng.random(N) < 0.15)] = True
                    mm[flip & m] = False
                    masks.append(mm)
                    cats.append(BENCHMARK_SEMANTIC_LABELS[lab] if lab in CLS else BENCHMARK_SEMANTIC_LABELS[CLS[0]])
            masks.append(rng.random(N) < 0.2)
            cats.append(BENCHMARK_SEMANTIC_LABELS[CLS[int(rng.integers(len(CLS)))]])
            masks = np.array(masks, np.int32)
            scores = rng.uniform(0.4, 1.0, len(masks)).astype(np.float32)
            per[n] = (masks, scores, np.array(cats, np.float32))
        runs.append(per)
    return runs


def gt_ids(r):
    """val_gt ids: nyu40 id * 1000 + instance + 1 (data/scannetv2/prepare_data_inst_gttxt.py), 0 unannotated"""
    ins, lab = r[:, 7].astype(np.int64), r[:, 6].astype(np.int64)
    out = np.zeros(len(ins), np.int64)
    for i in np.unique(ins[ins >= 0]):
        m = ins == i
        out[m] = BENCHMARK_SEMANTIC_LABELS[lab[m][0]] * 1000 + i + 1
    return out


def main():
    out = {}
    tmp = tempfile.mkdtemp()
    root = os.path.join(tmp, "scannetv2")
    os.makedirs(os.path.join(root, "scenes"))
    raws = {n: make(SUPPORT_POINTS, sd, ins) for n, sd, ins in SUPPORT}
    raws.update({n: make(p, sd, ins) for n, sd, p, ins in VAL})
    for name, r in raws.items():
        np.save(os.path.join(root, "scenes", name + ".npy"), r)
    ds0 = ScanNetDataset.__new__(ScanNetDataset)
    ds0.data_path, ds0.classes = root, 20
    ds0.class2type = {i: str(i) for i in range(20)}
    c2i = ds0.get_class2instances()
    val = [n for n, _, _, _ in VAL]
    names = sorted(raws)
    raw = np.concatenate([raws[n] for n in names])
    xyzrgb, labinst = raw[:, :6].astype(np.float32), raw[:, 6:].astype(np.int16)
    assert (xyzrgb.astype(np.float64) == raw[:, :6]).all() and (labinst.astype(np.float64) == raw[:, 6:]).all()
    out["names"], out["val_names"] = np.array(names), np.array(val)
    out["sizes"] = np.array([raws[n].shape[0] for n in names], np.int64)
    out["raw_xyzrgb"], out["raw_labinst"] = xyzrgb, labinst
    out["cvfold"], out["run_num"], out["k_shot"] = np.int64(CV), np.int64(RUN_NUM), np.int64(cfg.k_shot)
    out["test_seed"] = np.int64(cfg.test_seed)
    out["full_scale"], out["full_scale_support"] = np.array(cfg.full_scale), np.array(cfg.full_scale_support)
    for c in range(20):
        out[f"c2i_{c}_scene"] = np.array([s for s, _ in c2i[c]], dtype="U12")
        out[f"c2i_{c}_id"] = np.array([i for _, i in c2i[c]], np.int64)
    cfg.run_num, cfg.data_root, cfg.dataset = RUN_NUM, tmp, "scannetv2"
    sfile = os.path.join(root, "support_sets", f"{cfg.type_support}{CV}_{cfg.k_shot}shot_10sets.pkl")
    cfile = os.path.join(root, f"test_combinations_fold{CV}.pkl")

    # order "both": support sets generated, then the combinations on the same random stream
    random.seed(cfg.test_seed)
    ds = counting(dataset(root, c2i, val))
    _loads[0] = 0
    ss = ds.get_support_set(k_shot=cfg.k_shot)
    picks = RUN_NUM * len(CLS) * cfg.k_shot
    assert _loads[0] > picks, "no support draw was retried"
    out["support_retries"] = np.int64(_loads[0] - picks)
    combs = ds.get_test_comb()
    out["both/support_scene"], out["both/support_id"] = sets_array(ss)
    combs_arrays(out, "both/", combs, val)
    # order "comb": support sets loaded, combinations after random.seed(test_seed)
    os.remove(cfile)
    random.seed(cfg.test_seed)
    ds = dataset(root, c2i, val)
    ds.get_support_set(k_shot=cfg.k_shot)
    combs_c = ds.get_test_comb()
    combs_arrays(out, "comb/", combs_c, val)
    assert any(combs_c[n] != combs[n] for n in val if combs[n]["active_label"])
    assert not combs[val[-1]]["active_label"]

    # testMergeFS, both fix_support settings (the "both" combinations, on file)
    with open(cfile, "wb") as f:
        pickle.dump(combs, f, pickle.HIGHEST_PROTOCOL)
    ds = dataset(root, c2i, val)
    ds.test_combs = combs
    queries = {}
    for fix in (True, False):
        cfg.fix_support = fix
        for i, n in enumerate(val):
            ok, sups, q, infos = ds.testMergeFS([i])
            p = f"merge/{int(fix)}/{n}/"
            out[p + "valid"] = np.bool_(ok)
            if not ok:
                continue
            assert (q["labels"].numpy() == raws[n][:, 6].astype(np.int64)).all()
            if fix:
                store(out, p + "query/", q, raws[n])
                queries[n] = q
            else:  # the same query as with fix_support
                assert list(q) == list(queries[n])
                for k, v in q.items():
                    assert np.array_equal(np.asarray(v), np.asarray(queries[n][k])), k
            out[p + "n_support"] = np.int64(len(sups))
            out[p + "infos_active"] = np.array([int(l) for l in infos["active_label"]], np.int64)
            for j, s in enumerate(sups):
                if s is None:
                    continue
                l = infos["active_label"][j]
                out[p + f"support{j}/pair_scene"], out[p + f"support{j}/pair_id"] = (np.array(infos[l][0]),
                                                                                     np.int64(infos[l][1]))
                r = raws[infos[l][0]]
                kept = ds.get_region_inst(r[:, :3], r[:, 7].astype(np.int64), infos[l][1], scale_factor=1)[0]
                out[p + f"support{j}/rows"] = kept.astype(np.int32)
                store(out, p + f"support{j}/", s, r[kept])

    # load_set_support's per-support dicts, captured by a stub process_support
    import test_fs

    test_fs.logger = types.SimpleNamespace(info=lambda *a, **k: None)
    seen = []

    class Stub:
        def eval(self):
            return self

        def parameters(self):
            return iter([torch.zeros(1)])

        def process_support(self, d, training=False):
            seen.append({k: (v.clone() if torch.is_tensor(v) else v) for k, v in d.items()})
            return torch.full((1, 4), float(len(seen)))

    cfg.fix_support = True
    ds = dataset(root, c2i, val)
    test_fs.load_set_support(Stub(), ds)
    assert len(seen) == RUN_NUM * len(CLS) * cfg.k_shot
    for i in range(CAPTURE):
        t = ss[0][CLS[i // cfg.k_shot]][i % cfg.k_shot]
        out[f"vec/{i}/pair_scene"], out[f"vec/{i}/pair_id"] = np.array(t[0]), np.int64(t[1])
        store(out, f"vec/{i}/", seen[i], raws[t[0]])

    # the eval tail on recorded proposals
    runs = proposals(raws, val)
    run_dict = {}
    for k, per in enumerate(runs):
        matches = {}
        for si, n in enumerate(val):
            pr = per[n]
            p = f"eval/{k}/{n}/"
            out[p + "none"] = np.bool_(pr is None)
            if pr is None:
                continue
            masks, scores, cats = pr
            out[p + "masks"], out[p + "scores"], out[p + "cats"] = np.packbits(masks.astype(bool), axis=1), scores, cats
            pick = matrix_non_max_suppression(torch.from_numpy(masks).float(), torch.from_numpy(scores),
                                              torch.from_numpy(cats), final_score_thresh=0.5).numpy()
            out[p + "pick"] = pick.astype(np.int64)
            pred = {"conf": scores[pick], "label_id": cats[pick], "mask": masks[pick]}
            g2p, p2g = ref_eval.assign_instances_for_scan(n, pred, gt_ids(raws[n]))
            matches[n] = {"gt": g2p, "pred": p2g}
        avgs = ref_eval.compute_averages(ref_eval.evaluate_matches(matches))
        for key in ("all_ap", "all_ap_50%", "all_ap_25%"):
            out[f"eval/{k}/{key}"] = np.float64(avgs[key])
        out[f"eval/{k}/class_ap"] = np.array([[avgs["classes"][nm][t] for t in ("ap", "ap50%", "ap25%")]
                                              for nm in ref_eval.CLASS_LABELS], np.float64)
        run_dict = ref_eval.accumulate_averages_over_runs(run_dict, avgs)
    avg = ref_eval.compute_averages_over_runs(run_dict)
    for key in ("all_ap", "all_ap_50%", "all_ap_25%", "all_ap_std", "all_ap_50%_std", "all_ap_25%_std"):
        out["eval/avg/" + key] = np.float64(avg[key])
    out["eval/avg/class_ap"] = np.array([[avg["classes"][nm][t] for t in ("ap", "ap50%", "ap25%")]
                                         for nm in ref_eval.CLASS_LABELS], np.float64)
    for n in val:
        out["gt/" + n] = gt_ids(raws[n])
    np.savez_compressed(os.path.join(HERE, "test_merge_fs.npz"), **out)
    print("written", os.path.getsize(os.path.join(HERE, "test_merge_fs.npz")), "bytes; retries",
          int(out["support_retries"]))


if __name__ == "__main__":
    main()
