"""CPU: the few-shot test tables (geoformer_amd/fs_eval.py FSTestSet) and the eval tail of test_fs.py against the
reference's own get_support_set / get_test_comb, matrix_non_max_suppression and util/eval.py
(tests/golden/test_merge_fs.npz, tests/golden/make_test_merge_fs_golden.py)."""
import functools
import os
import pickle
import types

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "test_merge_fs.npz")


@functools.lru_cache(maxsize=1)
def fs_test_golden():
    """The golden as plain structures: scenes {name: raw [N, 8]}, val names, class2instances, tables, eval cases."""
    z = np.load(GOLDEN)
    g = {k: z[k] for k in z.files}
    names, sizes = [str(n) for n in g["names"]], g["sizes"]
    raw = np.concatenate([g["raw_xyzrgb"].astype(np.float64), g["raw_labinst"].astype(np.float64)], axis=1)
    off = np.concatenate([[0], np.cumsum(sizes)])
    g["scenes"] = {n: raw[off[i]:off[i + 1]].copy() for i, n in enumerate(names)}
    g["val"] = [str(n) for n in g["val_names"]]
    g["c2i"] = {c: [[str(s), int(i)] for s, i in zip(g[f"c2i_{c}_scene"], g[f"c2i_{c}_id"])] for c in range(20)}
    return g


def golden_sets(g):
    from geoformer_amd.augment import FOLD

    cls = FOLD[int(g["cvfold"])]
    return [{c: [[str(s), int(i)] for s, i in zip(g["both/support_scene"][r, ci], g["both/support_id"][r, ci])]
             for ci, c in enumerate(cls)} for r in range(int(g["run_num"]))]


def golden_combs(g, order):
    out = {}
    for n in g["val"]:
        act = [int(l) for l in g[f"{order}/{n}/active"]]
        out[n] = {"active_label": act}
        for l, s, i in zip(act, g[f"{order}/{n}/scene"], g[f"{order}/{n}/id"]):
            out[n][l] = [str(s), int(i)]
    return out


def build(g, **kw):
    from geoformer_amd.fs_eval import FSTestSet

    index = types.SimpleNamespace(class2instances=g["c2i"])
    return FSTestSet.build(g["scenes"], g["val"], index, int(g["cvfold"]), int(g["k_shot"]), int(g["run_num"]),
                           test_seed=int(g["test_seed"]), **kw)


def test_build_reproduces_both_generation_orders():
    g = fs_test_golden()
    assert int(g["support_retries"]) > 0  # a draw was retried under the 1000-point rule
    ts = build(g)
    assert ts.support_sets == golden_sets(g)
    assert ts.combinations == golden_combs(g, "both")
    assert ts.names == g["val"]
    assert ts.combinations[g["val"][-1]] == {"active_label": []}  # a val scene without active label
    ts2 = build(g, support_sets=ts.support_sets)  # support sets on file: the combinations follow random.seed(567)
    assert ts2.combinations == golden_combs(g, "comb")
    assert ts2.combinations != ts.combinations


def test_from_tables_takes_the_pickled_structures():
    from geoformer_amd.fs_eval import FSTestSet

    g = fs_test_golden()
    combs = {}
    for n, c in golden_combs(g, "both").items():
        combs[n] = {"active_label": [np.int64(l) for l in c["active_label"]]}
        for l in c["active_label"]:
            combs[n][np.int64(l)] = [c[l][0], np.int64(c[l][1])]
    sets = [{np.int64(k): [[s, np.int64(i)] for s, i in v] for k, v in run.items()} for run in golden_sets(g)]
    ts = FSTestSet.from_tables(pickle.loads(pickle.dumps(combs)), pickle.loads(pickle.dumps(sets)))
    ref = build(g)
    assert ts.combinations == ref.combinations and ts.support_sets == ref.support_sets and ts.names == ref.names
    assert all(type(l) is int for c in ts.combinations.values() for l in c["active_label"])


def eval_runs(g):
    runs = []
    for k in range(int(g["run_num"])):
        per = []
        for n in g["val"]:
            p = f"eval/{k}/{n}/"
            if bool(g[p + "none"]):
                per.append((n, None))
                continue
            N = g["scenes"][n].shape[0]
            masks = np.unpackbits(g[p + "masks"], axis=1)[:, :N].astype(np.int32)
            per.append((n, (torch.from_numpy(masks), torch.from_numpy(g[p + "scores"]), torch.from_numpy(g[p + "cats"]))))
        runs.append(per)
    return runs


def test_eval_tail_matches_reference_per_run_and_averaged():
    from geoformer_amd import evaluation
    from geoformer_amd.fs_eval import nms_and_evaluate

    g = fs_test_golden()
    runs = eval_runs(g)
    assert any(pr is None for per in runs for _, pr in per)  # a scene left out of a run
    gt = {n: g["gt/" + n] for n in g["val"]}
    summaries, avg, picks = nms_and_evaluate(runs, gt, int(g["cvfold"]))
    names = evaluation.class_set(int(g["cvfold"]))[1]
    for k, s in enumerate(summaries):
        for n, pr in runs[k]:
            if pr is not None:
                assert np.array_equal(picks[k][n].numpy(), g[f"eval/{k}/{n}/pick"]), (k, n)
            else:
                assert n not in picks[k]
        for key in ("all_ap", "all_ap_50%", "all_ap_25%"):
            assert np.isclose(s[key], g[f"eval/{k}/{key}"], rtol=0, atol=1e-12, equal_nan=True), (k, key)
        got = np.array([[s["classes"][nm][t] for t in ("ap", "ap50%", "ap25%")] for nm in names])
        assert np.allclose(got, g[f"eval/{k}/class_ap"], rtol=0, atol=1e-12, equal_nan=True), k
    for key in ("all_ap", "all_ap_50%", "all_ap_25%", "all_ap_std", "all_ap_50%_std", "all_ap_25%_std"):
        assert np.isclose(avg[key], g["eval/avg/" + key], rtol=0, atol=1e-12, equal_nan=True), key
    got = np.array([[avg["classes"][nm][t] for t in ("ap", "ap50%", "ap25%")] for nm in names])
    assert np.allclose(got, g["eval/avg/class_ap"], rtol=0, atol=1e-12, equal_nan=True)
    # the run where a scene has no proposal differs from counting it with an empty prediction set
    k = next(k for k in range(len(runs)) if any(pr is None for _, pr in runs[k]))
    empty = [(n, pr if pr is not None else (torch.zeros((0, g["scenes"][n].shape[0]), dtype=torch.int32),
                                            torch.zeros(0), torch.zeros(0))) for n, pr in runs[k]]
    alt = nms_and_evaluate([empty], gt, int(g["cvfold"]))[0][0]
    assert alt["all_ap_25%"] != summaries[k]["all_ap_25%"]


def test_too_few_support_sets_is_a_value_error():
    from geoformer_amd.fs_eval import FSTestSet

    g = fs_test_golden()
    ts = FSTestSet.from_tables(golden_combs(g, "both"), golden_sets(g)[:1])  # one set, as the shipped 1-shot pickle
    with pytest.raises(ValueError, match=r"1 support set.*run_num 10"):
        ts.check(10, 1)
    ts.check(1, 1)


def test_fold_2_is_rejected():
    from geoformer_amd.fs_eval import FSTestSet, nms_and_evaluate

    g = fs_test_golden()
    with pytest.raises(ValueError, match="cvfold 2"):
        build(dict(g, cvfold=np.int64(2)))
    ts = FSTestSet.from_tables(golden_combs(g, "both"), golden_sets(g))
    with pytest.raises(ValueError, match="cvfold 2"):
        ts.check(3, 2)
    with pytest.raises(ValueError, match="cvfold 2"):
        nms_and_evaluate([], {}, 2)


def test_scene_missing_from_the_combinations_is_a_value_error():
    from geoformer_amd.fs_eval import FSTestSet

    g = fs_test_golden()
    ts = FSTestSet.from_tables(golden_combs(g, "both"), golden_sets(g))
    with pytest.raises(ValueError, match="scene9999_00"):
        ts.combination("scene9999_00")
