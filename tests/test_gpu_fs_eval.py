"""GPU: the few-shot test path (geoformer_amd/augment.py test_merge_fs / support_blocks / full_scene_supports,
csrc/augment.hip gf_aug_test_query / gf_aug_support_block; geoformer_amd/fs_eval.py) against the reference's own
testMergeFS and load_set_support (tests/golden/test_merge_fs.npz), and evaluate_fs against the reference-shaped
sequential loop written here from the public API."""
import numpy as np
import pytest
import torch

from tests.test_fs_eval_host import fs_test_golden, golden_combs, golden_sets

pytestmark = pytest.mark.gpu


def _ts(g):
    from geoformer_amd.fs_eval import FSTestSet

    return FSTestSet.from_tables(golden_combs(g, "both"), golden_sets(g))


def _compare(got, g, prefix, rows):
    assert list(got) == [str(k) for k in g[prefix + "keys"]], (prefix, list(got))
    for k, v in got.items():
        want_dt = str(g[prefix + "dtype_" + k])
        if torch.is_tensor(v):
            assert v.is_cuda and str(v.dtype).replace("torch.", "") == want_dt, (prefix, k, v.dtype, want_dt)
            v = v.cpu().numpy()
        else:
            assert str(v.dtype) == want_dt, (prefix, k)
        if k in ("locs_float", "feats"):
            want = rows[:, :3] if k == "locs_float" else rows[:, 3:6]
            assert np.array_equal(v, want.astype(np.float32)), (prefix, k)
        else:
            assert np.array_equal(v, g[prefix + k].astype(v.dtype)), (prefix, k)


@pytest.mark.parametrize("fix_support", [True, False])
def test_test_merge_fs_matches_reference(hip, fix_support):
    from geoformer_amd import augment

    g = fs_test_golden()
    ts = _ts(g)
    fs, fss = tuple(int(x) for x in g["full_scale"]), tuple(int(x) for x in g["full_scale_support"])
    for n in g["val"]:
        ok, sups, q, infos = augment.test_merge_fs(g["scenes"], ts, n, fix_support=fix_support, cvfold=1,
                                                   full_scale=fs, full_scale_support=fss, device="cuda")
        p = f"merge/{int(fix_support)}/{n}/"
        assert ok == bool(g[p + "valid"])
        if not ok:
            assert (sups, q, infos) == ({}, {}, {})
            continue
        _compare(q, g, f"merge/1/{n}/query/", g["scenes"][n])
        assert infos["active_label"] == [int(l) for l in g[p + "infos_active"]]
        assert len(sups) == int(g[p + "n_support"])
        for j, s in enumerate(sups):
            if fix_support:
                assert s is None
                continue
            sp = p + f"support{j}/"
            assert infos[infos["active_label"][j]] == (str(g[sp + "pair_scene"]), int(g[sp + "pair_id"]))
            _compare(s, g, sp, g["scenes"][str(g[sp + "pair_scene"])][g[sp + "rows"]])


def test_absent_support_instance_is_a_hip_error(hip):
    from geoformer_amd import _lib, augment

    g = fs_test_golden()
    n = g["val"][0]
    with pytest.raises(_lib.GeoFormerHipError, match="no point"):
        augment.support_blocks(g["scenes"], [(n, int(g["scenes"][n][:, 7].max()) + 1)], device="cuda")
    good = augment.support_blocks(g["scenes"], [(n, int(g["scenes"][n][:, 7].max()))], device="cuda")
    assert good[0]["mask_offsets"][1].item() > 0


def test_full_scene_supports_match_load_set_support(hip):
    from geoformer_amd import augment

    g = fs_test_golden()
    pairs = []
    i = 0
    while f"vec/{i}/keys" in g:
        pairs.append((str(g[f"vec/{i}/pair_scene"]), int(g[f"vec/{i}/pair_id"])))
        i += 1
    assert pairs
    for i, pr in enumerate(pairs):
        d = augment.full_scene_supports(g["scenes"], [pr], device="cuda")
        ref_keys = [str(k) for k in g[f"vec/{i}/keys"]]
        _compare({k: d[k] for k in ref_keys}, g, f"vec/{i}/", g["scenes"][pr[0]])
    both = augment.full_scene_supports(g["scenes"], pairs, device="cuda")  # B > 1: the same rows, batch index = position
    n0 = g["scenes"][pairs[0][0]].shape[0]
    one = augment.full_scene_supports(g["scenes"], pairs[1:2], device="cuda")
    assert torch.equal(both["locs"][n0:, 1:], one["locs"][:, 1:]) and bool((both["locs"][n0:, 0] == 1).all())
    assert both["mask_offsets"].tolist()[1:] == np.cumsum([int(augment.full_scene_supports(
        g["scenes"], [p], device="cuda")["mask_offsets"][1]) for p in pairs]).tolist()


def _model():
    from tests.util import run_fs_episode

    z, m, emb, out, out2, cap = run_fs_episode("cuda")
    return m, emb


def test_batched_support_vectors_equal_per_support_calls(hip):
    from geoformer_amd import augment
    from geoformer_amd.fs_eval import support_vectors

    g = fs_test_golden()
    ts = _ts(g)
    m, _ = _model()
    R = int(g["run_num"])
    vec = support_vectors(m, g["scenes"], ts, cvfold=1, run_num=R, k_shot=1, chunk=4)
    vec1 = support_vectors(m, g["scenes"], ts, cvfold=1, run_num=R, k_shot=1, chunk=16, chunk_points=5000)
    for r in range(R):
        for c, pr in ((c, v[0]) for c, v in ts.support_sets[r].items()):
            with torch.no_grad():
                e = m.process_support(augment.full_scene_supports(g["scenes"], [tuple(pr)], device="cuda"),
                                      training=False)[0]
            assert (vec[r][c] - e).abs().max().item() < 1e-5, (r, c)
            assert (vec1[r][c] - e).abs().max().item() < 1e-5, (r, c)


def _val_scenes():
    """Small val scenes on the FS golden's scene (S8k, seed 7) and three others: the box instance takes a fold-1 class."""
    from geoformer_amd import augment, scene

    cls = augment.FOLD[1]
    out, combs = {}, {}
    for k, sd in enumerate((7, 8, 9, 10)):
        r = scene.make_raw_scene(8192, sd, n_boxes=1, room=(1.6, 1.6, 0.6))
        r[r[:, 7] >= 0, 6] = cls[k % 3]
        n = f"scene07{k:02d}_00"
        out[n] = r
        iid = int(r[:, 7].max())
        combs[n] = {"active_label": [cls[k % 3]], cls[k % 3]: [n, iid]}
    return out, combs


def _sequential(m, scenes, ts, vectors, run_num):
    """test_fs.py's do_test loop: one forward per (label, run), remember=(j, k) != (0, 0); per run the labels'
    proposals concatenated, NMS at 0.5, one evaluator per run (scenes without proposal left out)."""
    from geoformer_amd import augment, evaluation
    from geoformer_amd.postprocess import matrix_non_max_suppression

    evs = [evaluation.InstanceEvaluator(classes=1) for _ in range(run_num)]
    picks = [{} for _ in range(run_num)]
    for n in ts.names:
        ok, sups, q, infos = augment.test_merge_fs(scenes, ts, n, fix_support=True, cvfold=1, device="cuda")
        if not ok:
            continue
        cl = [[[], [], []] for _ in range(run_num)]
        for j, l in enumerate(infos["active_label"]):
            for k in range(run_num):
                with torch.no_grad():
                    o = m(None, q, training=False, remember=not (j == 0 and k == 0),
                          support_embeddings=vectors[k][l].unsqueeze(0))["proposal_scores"]
                if o is None or isinstance(o[0], list):
                    continue
                cl[k][0].append(o[1])
                cl[k][1].append(o[0])
                cl[k][2].append(torch.full((o[0].shape[0],), evaluation.BENCHMARK_SEMANTIC_LABELS[l], device="cuda"))
        r = torch.as_tensor(scenes[n], device="cuda")
        gt = evaluation.gt_ids_from_labels(r[:, 6].long(), r[:, 7].long())
        for k in range(run_num):
            if not cl[k][0]:
                continue
            masks, scores, labels = (torch.cat(x) for x in cl[k])
            pick = matrix_non_max_suppression(masks, scores, labels, final_score_thresh=0.5)
            evs[k].add_scene(n, gt, labels, scores, masks, pick)
            picks[k][n] = scores[pick]
    return [e.evaluate()[1] for e in evs], picks


def test_evaluate_fs_equals_sequential_loop(hip):
    from geoformer_amd.fs_eval import FSTestSet, evaluate_fs

    m, emb = _model()
    scenes, combs = _val_scenes()
    R = 3
    ts = FSTestSet.from_tables(combs, [])
    vectors = [{c: (emb[0] * f) for c in (5, 6, 8, 10, 14, 15, 16, 17, 19)} for f in (1.0, 0.5, 0.75)]
    res = evaluate_fs(m, scenes, ts, cvfold=1, run_num=R, fix_support=True, vectors=vectors)
    seq, seq_picks = _sequential(m, scenes, ts, vectors, R)
    multi = [n for n in ts.names if sum(n in seq_picks[k] and len(seq_picks[k][n]) > 0 for k in range(R)) >= 2]
    assert multi, "no scene has accepted proposals in two runs"
    for k in range(R):
        assert set(res["picks"][k]) == set(seq_picks[k]), k
        for n, s in seq_picks[k].items():
            got = res["picks"][k][n][0]
            assert len(got) == len(s), (k, n)
            if len(s):
                assert (torch.sort(got)[0] - torch.sort(s)[0]).abs().max().item() < 1e-5, (k, n)
        for key in ("all_ap", "all_ap_50%", "all_ap_25%"):
            assert np.isclose(res["runs"][k][key], seq[k][key], atol=1e-3, equal_nan=True), (k, key)
    for key in ("all_ap", "all_ap_50%", "all_ap_25%"):
        assert np.isclose(res["average"][key], np.mean([s[key] for s in seq]), atol=1e-3, equal_nan=True)


def test_evaluate_fs_block_supports_make_identical_runs(hip):
    from geoformer_amd.fs_eval import FSTestSet, evaluate_fs

    m, _ = _model()
    scenes, combs = _val_scenes()
    ts = FSTestSet.from_tables(combs, [])
    res = evaluate_fs(m, scenes, ts, cvfold=1, run_num=3, fix_support=False)
    for k in (1, 2):
        for key in ("all_ap", "all_ap_50%", "all_ap_25%"):
            assert np.array_equal(res["runs"][k][key], res["runs"][0][key], equal_nan=True)
        assert set(res["picks"][k]) == set(res["picks"][0])
        for n in res["picks"][0]:
            assert torch.equal(res["picks"][k][n][0], res["picks"][0][n][0])
    assert res["average"]["all_ap_std"] == 0.0 or np.isnan(res["average"]["all_ap_std"])
