"""Few-shot test-time evaluation (test_fs.py:33-259, datasets/scannetv2_fs_inst.py:80-183 and 568-700) on the GPU.

    test_set = FSTestSet.build(scenes_by_name, val_names, index, cvfold=1, k_shot=1, run_num=10)
    # or FSTestSet.from_tables(pickle.load(test_combinations), pickle.load(support_sets))
    res = evaluate_fs(model, scenes_by_name, test_set)
    print(evaluation.format_results(res["average"]))

Per val scene: the query comes from augment.test_merge_fs (csrc/augment.hip: gf_aug_test_query, and gf_aug_support_block
for the block supports of fix_support False).  The L active labels times R runs of the reference's loop -- one
forward(remember=(j, k) != (0, 0)) each -- are one fresh forward and one GeoFormerFS.requery_many over the other L*R - 1
embeddings.  Each run's proposals are concatenated over the labels (category = the label's nyu40 id), go through
postprocess.matrix_non_max_suppression with final_score_thresh 0.5 and into that run's InstanceEvaluator; a scene
without any proposal in run k is left out of run k, as in the reference.  The runs are averaged with
evaluation.average_over_runs.
"""
from __future__ import annotations

import random

import numpy as np
import torch

from . import augment, evaluation
from .postprocess import matrix_non_max_suppression

FOLD = augment.FOLD
SUPPORT_MIN_POINTS = 1000  # get_support_set: a support instance needs >= 1000 points of its own
NMS_FINAL_SCORE = 0.5  # test_fs.py:207 (not TEST_NMS_THRESH)
SUPPORT_CHUNK = 8  # full-scene supports per process_support call
SUPPORT_CHUNK_POINTS = 1 << 20  # and at most this many points per call (a larger scene goes alone)


def _check_fold(cvfold):
    if cvfold not in FOLD:
        raise ValueError(f"cvfold {cvfold}: only 0 and 1 are supported (the reference's util/eval.py evaluates any "
                         "other fold on fold 0's classes)")


def _host(sc):
    return sc.detach().cpu().numpy() if torch.is_tensor(sc) else np.asarray(sc)


class FSTestSet:
    """The two tables of the few-shot test: combinations {scene: {"active_label": [l, ...], l: [support scene, id]}}
    (test_combinations_fold{cv}.pkl) and support_sets, a list of run_num dicts {class: [[scene, id]] * k_shot}
    (support_sets/fullscene_fold{cv}_{k}shot_10sets.pkl).  names: the val scenes in the test loader's order."""

    def __init__(self, combinations, support_sets, names=None):
        self.combinations = {}
        for s, c in combinations.items():
            d = {"active_label": [int(l) for l in c["active_label"]]}
            for l in d["active_label"]:
                if l in c:
                    d[l] = [str(c[l][0]), int(c[l][1])]
            self.combinations[str(s)] = d
        self.support_sets = [{int(k): [[str(t[0]), int(t[1])] for t in v] for k, v in run.items()}
                             for run in (support_sets or [])]
        self.names = sorted(self.combinations, key=lambda n: n + ".npy") if names is None else [str(n) for n in names]

    @classmethod
    def from_tables(cls, test_combs, support_sets, names=None):
        """The reference's pickled tables as they are (np.int64 keys and ids accepted)."""
        return cls(test_combs, support_sets, names)

    @classmethod
    def build(cls, scenes_by_name, val_names, index, cvfold, k_shot, run_num, test_seed=567, support_sets=None):
        """Both generators of the reference with its random ordering: random is seeded with test_seed (init()); the
        support sets (unless given: the reference loads its pickle then) reseed with 10 * run per run and draw, per
        class of the fold and shot, random.choice(class2instances[class]) until the instance has >= 1000 points; the
        combinations then continue the same stream over the val scenes in sorted order, one draw per active label.
        index: augment.FSIndex of the tables."""
        _check_fold(cvfold)
        rng = random.Random(test_seed)
        host = {}

        def scene(name):
            if name not in host:
                host[name] = _host(scenes_by_name[name])
            return host[name]

        if support_sets is None:
            support_sets = []
            for run in range(run_num):
                rng.seed(10 * run)
                ss = {c: [] for c in FOLD[cvfold]}
                for c in FOLD[cvfold]:
                    cands = index.class2instances.get(c, [])
                    if not any(np.count_nonzero(scene(s)[:, 7].astype(np.int64) == i) >= SUPPORT_MIN_POINTS
                               for s, i in cands):
                        raise ValueError(f"FSTestSet.build: class {c} lists no instance with >= {SUPPORT_MIN_POINTS} "
                                         "points (the reference's loop would not end)")
                    for _ in range(k_shot):
                        while True:
                            s, i = rng.choice(cands)
                            if np.count_nonzero(scene(s)[:, 7].astype(np.int64) == i) >= SUPPORT_MIN_POINTS:
                                break
                        ss[c].append([s, i])
                support_sets.append(ss)
        names = sorted(val_names, key=lambda n: n + ".npy")
        combs = {}
        for name in names:
            label = scene(name)[:, 6].astype(np.int64)
            active = [int(l) for l in np.unique(label) if l != -100 and l in FOLD[cvfold]]
            combs[name] = {"active_label": active}
            for l in active:
                combs[name][l] = list(rng.choice(index.class2instances[l]))
        return cls(combs, support_sets, names)

    def combination(self, name):
        if name not in self.combinations:
            raise ValueError(f"FSTestSet: scene {name!r} is not in the test combinations")
        return self.combinations[name]

    def check(self, run_num, cvfold, k_shot=None, fix_support=True):
        """The reference's preconditions, as errors instead of its IndexError / silent fold-0 evaluation."""
        _check_fold(cvfold)
        if fix_support:
            if len(self.support_sets) < run_num:
                raise ValueError(f"FSTestSet: {len(self.support_sets)} support set(s) for run_num {run_num}")
            for r in range(run_num):
                for c in FOLD[cvfold]:
                    have = len(self.support_sets[r].get(c, []))
                    if have == 0 or (k_shot is not None and have < k_shot):
                        raise ValueError(f"FSTestSet: run {r}, class {c}: {have} support(s) for k_shot {k_shot}")


_CFG_DEFAULTS = {"run_num": 10, "k_shot": 1, "fix_support": True}  # the shipped test yaml's


def _cfg(model, name, value):
    if value is not None:
        return value
    if name in _CFG_DEFAULTS:
        return getattr(model.cfg, name, _CFG_DEFAULTS[name])
    return getattr(model.cfg, name)


@torch.no_grad()
def support_vectors(model, scene_of, test_set, *, cvfold=None, run_num=None, k_shot=None, scale=50,
                    full_scale=(128, 512), mode=4, chunk=SUPPORT_CHUNK, chunk_points=SUPPORT_CHUNK_POINTS):
    """load_set_support (test_fs.py:33-112): [run][class] -> [C] mean over the k_shot full-scene support embeddings, on
    the model's device.  The supports of a run go through process_support in batches of at most `chunk` scenes and
    `chunk_points` points (one scene larger than that goes alone)."""
    cvfold, run_num, k_shot = _cfg(model, "cvfold", cvfold), _cfg(model, "run_num", run_num), _cfg(model, "k_shot", k_shot)
    test_set.check(run_num, cvfold, k_shot)
    dev = next(model.parameters()).device
    model.eval()
    out = []
    for r in range(run_num):
        pairs = [(c, tuple(test_set.support_sets[r][c][i])) for c in FOLD[cvfold] for i in range(k_shot)]
        embs = []
        i = 0
        while i < len(pairs):
            j, pts = i, 0
            while j < len(pairs) and j - i < chunk:
                n = int(scene_of[pairs[j][1][0]].shape[0])
                if j > i and pts + n > chunk_points:
                    break
                pts += n
                j += 1
            d = augment.full_scene_supports(scene_of, [p for _, p in pairs[i:j]], scale=scale, full_scale=full_scale,
                                            mode=mode, device=dev)
            embs.append(model.process_support(d, training=False))
            i = j
        e = torch.cat(embs)
        out.append({c: e[ci * k_shot:(ci + 1) * k_shot].mean(dim=0) for ci, c in enumerate(FOLD[cvfold])})
    return out


def nms_and_evaluate(runs, gt_ids, cvfold, classes=None):
    """The tail of test_fs.py (:185-259) on recorded proposals: runs[k] is a list of (scene, proposals) where proposals
    is None (no proposal in run k: the scene is left out of run k) or (masks [n, N], scores [n], label_ids [n] nyu40);
    gt_ids[scene]: val_gt ids [N].  Per run and scene matrix NMS with final_score_thresh 0.5, ScanNet AP per run,
    average over the runs.  Device tensors keep the device paths, host arrays the numpy / CPU ones.
    Returns (per-run summaries, average, picks[k][scene] = picked row indices)."""
    if classes is None:
        _check_fold(cvfold)
    summaries, picks = [], []
    for preds in runs:
        ev = evaluation.InstanceEvaluator(classes=cvfold if classes is None else classes)
        pk = {}
        for name, pr in preds:
            if pr is None:
                continue
            masks, scores, labels = pr
            if not torch.is_tensor(masks):
                masks, scores, labels = torch.as_tensor(masks), torch.as_tensor(scores), torch.as_tensor(labels)
            if scores.shape[0] == 0:
                pick = torch.zeros(0, dtype=torch.int64, device=scores.device)
            else:
                pick = matrix_non_max_suppression(masks if masks.is_cuda else masks.float(), scores, labels,
                                                  final_score_thresh=NMS_FINAL_SCORE)
            pk[name] = pick
            if masks.is_cuda:
                ev.add_scene(name, gt_ids[name], labels, scores, masks, pick)
            else:
                ev.add_scene(name, np.asarray(gt_ids[name]), labels.numpy(), scores.numpy(), masks.numpy(),
                             pick.numpy())
        summaries.append(ev.evaluate()[1])
        picks.append(pk)
    return summaries, evaluation.average_over_runs(summaries), picks


@torch.no_grad()
def evaluate_fs(model, scene_of, test_set, *, cvfold=None, run_num=None, fix_support=None, classes=None, k_shot=None,
                names=None, scale=50, full_scale=None, full_scale_support=None, mode=4, vectors=None):
    """test_fs.py's do_test on the GPU.  Returns {"runs": per-run summaries, "average": their average, "picks":
    [run][scene] -> (scores, label ids) of the picked proposals, "vectors": the support vectors used}.  Defaults
    come from model.cfg (cvfold, run_num, k_shot, fix_support, full_scale, full_scale_support).  With fix_support
    False every run sees the same block supports (as in the reference, where all runs are identical): their
    embeddings are computed once and the label's proposals are shared by every run.  names: the scenes to test
    (default: test_set.names); vectors: precomputed support_vectors."""
    cfg = model.cfg
    cvfold, run_num = _cfg(model, "cvfold", cvfold), _cfg(model, "run_num", run_num)
    k_shot, fix_support = _cfg(model, "k_shot", k_shot), bool(_cfg(model, "fix_support", fix_support))
    full_scale = tuple(cfg.full_scale) if full_scale is None else tuple(full_scale)
    full_scale_support = (tuple(getattr(cfg, "full_scale_support", (64, 128))) if full_scale_support is None
                          else tuple(full_scale_support))
    test_set.check(run_num, cvfold, k_shot, fix_support and vectors is None)
    if fix_support and vectors is not None and len(vectors) < run_num:
        raise ValueError(f"evaluate_fs: {len(vectors)} run(s) of support vectors for run_num {run_num}")
    dev = next(model.parameters()).device
    model.eval()
    if fix_support and vectors is None:
        vectors = support_vectors(model, scene_of, test_set, cvfold=cvfold, run_num=run_num, k_shot=k_shot,
                                  scale=scale, full_scale=full_scale, mode=mode)
    bench = evaluation.BENCHMARK_SEMANTIC_LABELS
    runs = [[] for _ in range(run_num)]
    gt_ids = {}
    for name in (test_set.names if names is None else names):
        ok, sups, q, infos = augment.test_merge_fs(scene_of, test_set, name, fix_support=fix_support, cvfold=cvfold,
                                                   scale=scale, full_scale=full_scale,
                                                   full_scale_support=full_scale_support, mode=mode, device=dev)
        if not ok:
            continue
        active = infos["active_label"]
        if fix_support:
            embs = torch.stack([vectors[k][l] for l in active for k in range(run_num)]).to(dev)  # (j, k) order
            per = run_num
        else:
            embs = torch.cat([model.process_support(d, training=False) for d in sups])
            per = 1
        first = model(None, q, training=False, remember=False, support_embeddings=embs[0:1])["proposal_scores"]
        res = [first] + (model.requery_many(q, embs[1:]) if embs.shape[0] > 1 else [])
        raw = scene_of[name]
        raw_t = raw if torch.is_tensor(raw) and raw.is_cuda else torch.as_tensor(_host(raw), device=dev)
        gt_ids[name] = evaluation.gt_ids_from_labels(raw_t[:, 6].long(), raw_t[:, 7].long())
        for k in range(run_num):
            masks, scores, labels = [], [], []
            for j, l in enumerate(active):
                r = res[j * per + (k if fix_support else 0)]
                if r is None or isinstance(r[0], list):
                    continue
                masks.append(r[1])
                scores.append(r[0])
                labels.append(torch.full((r[0].shape[0],), bench[l], dtype=torch.int64, device=dev))
            runs[k].append((name, (torch.cat(masks), torch.cat(scores), torch.cat(labels)) if masks else None))
    summaries, avg, picks = nms_and_evaluate(runs, gt_ids, cvfold, classes)
    picked = []
    for k in range(run_num):
        d = {}
        for name, pr in runs[k]:
            if pr is not None:
                p = picks[k][name]
                d[name] = (pr[1][p], pr[2][p])
        picked.append(d)
    return {"runs": summaries, "average": avg, "picks": picked, "vectors": vectors}
