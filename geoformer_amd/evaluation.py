"""ScanNet v2 instance-segmentation evaluation (AP, AP50, AP25): the last stage of the reference's test loop
(test.py:98-148, test_fs.py:219-259, util/eval.py), written from the published ScanNet benchmark algorithm
(BenchmarkScripts/3d_evaluation/evaluate_semantic_instance.py).

The per-scene part -- every picked mask against every ground-truth instance and the void points over all N points -- is
one native call (gf_instance_overlaps, csrc/inst_eval.hip) on device tensors, followed by one small device-to-host copy
of its tables.  Host arrays take a numpy path with the same semantics (the CPU reference).  What is kept per scene is a
few KB: the instances' ids and sizes and, per kept prediction, its label, confidence, size and overlap row.  The
dataset-level matching and AP integration run on the host once per evaluation.

    ev = InstanceEvaluator(classes=0)                 # cvfold 0 / 1, or "all" (the 18 benchmark classes)
    ev.add_scene(name, gt_ids, label_ids, scores, masks, pick)
    ap, avgs = ev.evaluate(); print(ev.format_results(avgs))
    bx = BoxEvaluator(classes=0, kind="oriented")     # box AP: detection mAP@0.25 / mAP@0.5 over the instances' 3D boxes
    bx.add_scene(name, gt_ids, label_ids, scores, masks, pick, xyz)
    print(bx.format_results())
"""
from __future__ import annotations

import warnings
from typing import NamedTuple

import numpy as np

# ---- label tables of the ScanNet v2 benchmark --------------------------------------------------------------------------
# the 18 evaluated nyu40 ids and their names
VALID_CLASS_IDS = (3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39)
CLASS_NAMES = ("cabinet", "bed", "chair", "sofa", "table", "door", "window", "bookshelf", "picture", "counter", "desk",
               "curtain", "refrigerator", "shower curtain", "toilet", "sink", "bathtub", "otherfurniture")
# nyu40 id of each of the dataset's 20 semantic labels (0..19: wall, floor, then the 18 above)
BENCHMARK_SEMANTIC_LABELS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39)
# the few-shot folds: dataset semantic labels of the nine classes of each cvfold
FOLD_SEMANTIC_LABELS = {0: (2, 3, 4, 7, 9, 11, 12, 13, 18), 1: (5, 6, 8, 10, 14, 15, 16, 17, 19)}
FOLD_CLASS_IDS = {k: tuple(BENCHMARK_SEMANTIC_LABELS[s] for s in v) for k, v in FOLD_SEMANTIC_LABELS.items()}

DEFAULT_OVERLAPS = tuple(np.append(np.arange(0.5, 0.95, 0.05), 0.25))
MIN_REGION_SIZE = 100
DEFAULT_MAX_GT = 256  # capacity of the native call's instance tables before it is grown


def class_set(classes=0):
    """(nyu40 ids, names) of an evaluated class set: cvfold 0 or 1, "all", or an explicit sequence of nyu40 ids."""
    if isinstance(classes, str):
        if classes != "all":
            raise ValueError(f"classes: 0, 1, 'all' or a sequence of nyu40 ids, not {classes!r}")
        ids = VALID_CLASS_IDS
    elif isinstance(classes, (int, np.integer)):
        if int(classes) not in FOLD_CLASS_IDS:
            raise ValueError(f"cvfold {classes}: 0 or 1")
        ids = FOLD_CLASS_IDS[int(classes)]
    else:
        ids = tuple(int(c) for c in classes)
    ids = np.asarray(ids, dtype=np.int64)
    if len(ids) == 0 or len(set(ids.tolist())) != len(ids) or (ids <= 0).any():
        raise ValueError("classes: distinct positive nyu40 ids")
    name = dict(zip(VALID_CLASS_IDS, CLASS_NAMES))
    return ids, [name.get(int(i), str(int(i))) for i in ids]


def benchmark_label_ids(cls_final, cvfold):
    """nyu40 ids of the model's classes (4..12 in fold space) as test.py:65-68 maps them; on the tensor's device."""
    ids = FOLD_CLASS_IDS[int(cvfold)]
    if _is_tensor(cls_final):
        import torch

        return torch.tensor(ids, dtype=torch.int64, device=cls_final.device)[cls_final.long() - 4]
    return np.asarray(ids, dtype=np.int64)[np.asarray(cls_final, dtype=np.int64) - 4]


def gt_ids_from_labels(semantic_label, instance_label):
    """val_gt ids of a scene from its per-point dataset labels (semantic 0..19 or -100, instance 0..I-1 or -100), as
    data/scannetv2/prepare_data_inst_gttxt.py writes them: nyu40_id * 1000 + instance + 1, 0 where unannotated; an
    instance takes the semantic label of its first point (-100 counts as label 0).  numpy in, numpy out; a tensor stays
    on its device."""
    if _is_tensor(instance_label):
        import torch

        inst = instance_label.long()
        sem = semantic_label.to(inst.device).long()
        N = inst.shape[0]
        out = torch.zeros(N, dtype=torch.int64, device=inst.device)
        on = inst >= 0
        if N == 0 or not bool(on.any()):
            return out
        n_inst = int(inst.max()) + 1
        pos = torch.arange(N, device=inst.device)
        first = torch.full((n_inst,), N, dtype=torch.int64, device=inst.device)
        first.scatter_reduce_(0, inst[on], pos[on], "amin")
        s = sem[first.clamp(max=N - 1)]
        s = torch.where(s == -100, torch.zeros_like(s), s)
        bench = torch.tensor(BENCHMARK_SEMANTIC_LABELS, dtype=torch.int64, device=inst.device)
        code = bench[s] * 1000 + torch.arange(1, n_inst + 1, device=inst.device)
        out[on] = code[inst[on]]
        return out
    inst = np.asarray(instance_label).astype(np.int64)
    sem = np.asarray(semantic_label).astype(np.int64)
    out = np.zeros(inst.shape[0], dtype=np.int64)
    on = inst >= 0
    if not on.any():
        return out
    ids, first = np.unique(inst[on], return_index=True)
    s = sem[np.nonzero(on)[0][first]]
    s[s == -100] = 0
    code = np.zeros(int(ids.max()) + 1, dtype=np.int64)
    code[ids] = np.asarray(BENCHMARK_SEMANTIC_LABELS, dtype=np.int64)[s] * 1000 + ids + 1
    out[on] = code[inst[on]]
    return out


def _is_tensor(x):
    return type(x).__module__.startswith("torch") and hasattr(x, "device")


# ---- per-scene tables ----------------------------------------------------------------------------------------------------
def scene_overlaps_host(masks, gt_ids, class_ids, rows=None):
    """numpy statement of gf_instance_overlaps: (gt_id [G], gt_count [G], inter [n, G+1]) with the instances of the
    class set in ascending id order and the void points in the last column."""
    gt = np.asarray(gt_ids, dtype=np.int64)
    masks = np.asarray(masks)
    if masks.ndim != 2 or masks.shape[1] != gt.shape[0]:
        raise ValueError(f"masks {masks.shape} against {gt.shape[0]} points")
    valid = np.isin(gt // 1000, np.asarray(class_ids, dtype=np.int64))
    gt_id, slot, gt_count = np.unique(gt[valid], return_inverse=True, return_counts=True)
    G = len(gt_id)
    key = np.full(gt.shape[0], G, dtype=np.int64)
    key[valid] = slot
    m = masks if rows is None else masks[np.asarray(rows, dtype=np.int64)]
    r, p = np.nonzero(m)
    n = m.shape[0]
    inter = np.bincount(r * (G + 1) + key[p], minlength=n * (G + 1)).reshape(n, G + 1)
    return gt_id, gt_count.astype(np.int64), inter


class _Scene:
    """What a scene leaves behind: its instances (ids ascending, sizes) and the kept predictions in order (nyu40
    label, confidence, size, void points, overlap with every instance)."""

    __slots__ = ("name", "gt_id", "gt_count", "label", "conf", "count", "void", "inter")

    def __init__(self, name, gt_id, gt_count, inter, labels, conf, class_ids, min_region_size):
        count = inter.sum(1)
        keep = np.isin(labels, class_ids) & (count >= min_region_size)
        self.name = name
        self.gt_id = np.asarray(gt_id, dtype=np.int64)
        self.gt_count = np.asarray(gt_count, dtype=np.int64)
        self.label = labels[keep]
        self.conf = conf[keep]
        self.count = count[keep]
        self.void = inter[keep, -1]
        self.inter = np.ascontiguousarray(inter[keep, :-1])

    def by_class(self, cid):
        """(instances, predictions) of one class in the form the matching reads:
        instances: [(id, size, [(pred key, pred size, confidence, intersection), ...])]  (predictions in order)
        predictions: [(key, confidence, size, void points, [(instance id, instance size, intersection), ...])]"""
        gcols = np.nonzero(self.gt_id // 1000 == cid)[0]
        prows = np.nonzero(self.label == cid)[0]
        sub = self.inter[np.ix_(prows, gcols)]
        keys = [(self.name, int(k)) for k in prows]
        gts = []
        for j, g in enumerate(gcols):
            hit = np.nonzero(sub[:, j])[0]
            gts.append((int(self.gt_id[g]), int(self.gt_count[g]),
                        [(keys[i], int(self.count[prows[i]]), float(self.conf[prows[i]]), int(sub[i, j])) for i in hit]))
        preds = []
        for i, pr in enumerate(prows):
            hit = np.nonzero(sub[i])[0]
            preds.append((keys[i], float(self.conf[pr]), int(self.count[pr]), int(self.void[pr]),
                          [(int(self.gt_id[gcols[j]]), int(self.gt_count[gcols[j]]), int(sub[i, j])) for j in hit]))
        return gts, preds


# ---- dataset-level matching and AP -------------------------------------------------------------------------------------
def _average_precision(y_true, y_score, hard_fn):
    """Area under the precision-recall curve with one point per distinct score (plus the artificial (r=0, p=1) end),
    integrated with the [-0.5, 0, 0.5] step widths of the benchmark."""
    order = np.argsort(y_score)
    ys = y_score[order]
    csum = np.cumsum(y_true[order])
    _, first = np.unique(ys, return_index=True)
    n_true = csum[-1] if len(csum) else 0
    below = np.append(csum, 0)[first - 1]  # true examples scored strictly below each threshold
    tp = n_true - below
    fp = len(ys) - first - tp
    fn = below + hard_fn
    precision = np.append(tp / (tp + fp), 1.0)
    recall = np.append(tp / (tp + fn), 0.0)
    widths = np.convolve(np.concatenate(([recall[0]], recall, [0.0])), [-0.5, 0, 0.5], "valid")
    return np.dot(precision, widths)


def _ap_table(scenes, n_classes, overlaps, min_region_size):
    """scenes: per scene a list over classes of (instances, predictions) as _Scene.by_class gives them.  Greedy matching
    per overlap threshold in prediction order, a prediction matched once per threshold across the whole set."""
    ap = np.zeros((n_classes, len(overlaps)))
    for oi, th in enumerate(overlaps):
        visited = set()
        for li in range(n_classes):
            y_true, y_score = [], []
            hard_fn = 0
            has_gt = has_pred = False
            for sc in scenes:
                gts, preds = sc[li]
                gts = [g for g in gts if g[0] >= 1000 and g[1] >= min_region_size]
                has_gt |= len(gts) > 0
                has_pred |= len(preds) > 0
                for gid, gsize, cands in gts:
                    score = None
                    for key, psize, conf, inter in cands:
                        if key in visited or not inter / (gsize + psize - inter) > th:
                            continue
                        if score is None:
                            score = conf
                            visited.add(key)
                        else:  # a second match of this instance: the lower-scored one is a false positive
                            y_true.append(0.0)
                            y_score.append(min(score, conf))
                            score = max(score, conf)
                    if score is None:
                        hard_fn += 1
                    else:
                        y_true.append(1.0)
                        y_score.append(score)
                for key, conf, psize, void, cands in preds:
                    if any(inter / (gsize + psize - inter) > th for _, gsize, inter in cands):
                        continue
                    ignore = void
                    for gid, gsize, inter in cands:
                        if gid < 1000:  # a group
                            ignore += inter
                        if gsize < min_region_size:  # a small instance
                            ignore += inter
                    if ignore / psize <= th:
                        y_true.append(0.0)
                        y_score.append(conf)
            if has_gt and has_pred:
                ap[li, oi] = _average_precision(np.asarray(y_true, dtype=np.float64),
                                                np.asarray(y_score, dtype=np.float64), hard_fn)
            elif has_gt:
                ap[li, oi] = 0.0
            else:
                ap[li, oi] = float("nan")
    return ap


def _averages(ap, names, overlaps):
    """The benchmark's summary of an AP table [C, n_overlaps]: mean over classes (ignoring nan) of AP over the
    thresholds other than 0.25, of AP50 and of AP25, and the same per class."""
    aps = np.asarray(ap)[None]
    ov = np.asarray(overlaps)
    o50 = np.where(np.isclose(ov, 0.5))
    o25 = np.where(np.isclose(ov, 0.25))
    rest = np.where(np.logical_not(np.isclose(ov, 0.25)))
    with warnings.catch_warnings():  # (nanmean of an all-nan slice: a class set with no instance at all)
        warnings.simplefilter("ignore", RuntimeWarning)
        avgs = {"all_ap": np.nanmean(aps[0, :, rest]), "all_ap_50%": np.nanmean(aps[0, :, o50]),
                "all_ap_25%": np.nanmean(aps[0, :, o25]), "classes": {}}
        for li, name in enumerate(names):
            avgs["classes"][name] = {"ap": np.average(aps[0, li, rest]), "ap50%": np.average(aps[0, li, o50]),
                                     "ap25%": np.average(aps[0, li, o25])}
    return avgs


def average_over_runs(runs):
    """Mean (and the std of the three overall numbers) of several evaluate() summaries: test_fs.py's run_num loop."""
    if not runs:
        raise ValueError("average_over_runs: no runs")
    out = {}
    for k in ("all_ap", "all_ap_50%", "all_ap_25%"):
        v = np.array([r[k] for r in runs])
        out[k] = np.mean(v)
        out[k + "_std"] = np.std(v)
    out["classes"] = {name: {k: np.mean(np.array([r["classes"][name][k] for r in runs])) for k in ("ap", "ap50%", "ap25%")}
                      for name in runs[0]["classes"]}
    return out


def format_results(avgs):
    """The summary as a printable table (per class AP / AP50 / AP25, the average and, for a run average, the std)."""
    lines = ["#" * 64, f"{'what':<15}:{'AP':>15}{'AP_50%':>15}{'AP_25%':>15}", "#" * 64]
    for name, c in avgs["classes"].items():
        lines.append(f"{name:<15}:{c['ap']:>15.3f}{c['ap50%']:>15.3f}{c['ap25%']:>15.3f}")
    lines.append("-" * 64)
    lines.append(f"{'average':<15}:{avgs['all_ap']:>15.3f}{avgs['all_ap_50%']:>15.3f}{avgs['all_ap_25%']:>15.3f}")
    if "all_ap_std" in avgs:
        lines.append(f"{'std':<15}:{avgs['all_ap_std']:>15.3f}{avgs['all_ap_50%_std']:>15.3f}"
                     f"{avgs['all_ap_25%_std']:>15.3f}")
    return "\n".join(lines)


class InstanceEvaluator:
    """AP / AP50 / AP25 of instance predictions over a set of scenes (ScanNet v2 benchmark rules).

    classes: cvfold 0 or 1 (nine classes each), "all" (the 18 benchmark classes) or a sequence of nyu40 ids.
    min_region_size: predictions and instances smaller than this many points are ignored.
    overlaps: IoU thresholds; AP averages all but 0.25, AP50 / AP25 are the 0.5 / 0.25 columns."""

    def __init__(self, classes=0, min_region_size=MIN_REGION_SIZE, overlaps=DEFAULT_OVERLAPS):
        self.class_ids, self.class_names = class_set(classes)
        self.min_region_size = int(min_region_size)
        self.overlaps = tuple(float(o) for o in overlaps)
        self.scenes = []
        self._dev_classes = {}
        self.max_gt = DEFAULT_MAX_GT

    def add_scene(self, name, gt_ids, label_ids, scores, masks, pick=None):
        """One scene's predictions: masks [n_rows, N] (nonzero = member), label_ids [n_rows] nyu40 ids (e.g.
        benchmark_label_ids(cls_final, cvfold)), scores [n_rows], pick: the rows to evaluate, in order (the NMS result;
        default all rows), gt_ids [N] val_gt ids (gt_ids_from_labels).  Device tensors: the native overlap call and one
        device-to-host copy; host arrays: the numpy path."""
        if any(s.name == name for s in self.scenes):
            raise ValueError(f"scene {name!r} was added already")
        if _is_tensor(masks) and masks.is_cuda:
            gt_id, gt_count, inter, labels, conf = self._tables_device(gt_ids, label_ids, scores, masks, pick)
        else:
            gt_id, gt_count, inter = scene_overlaps_host(masks, gt_ids, self.class_ids, pick)
            sel = slice(None) if pick is None else np.asarray(pick, dtype=np.int64)
            labels = np.asarray(label_ids).astype(np.int64)[sel]
            conf = np.asarray(scores)[sel]
        self.scenes.append(_Scene(name, gt_id, gt_count, inter, np.asarray(labels, dtype=np.int64),
                                  np.asarray(conf), self.class_ids, self.min_region_size))

    def _tables_device(self, gt_ids, label_ids, scores, masks, pick):
        import torch

        from . import pointops

        dev = masks.device
        if masks.dtype != torch.int32:
            masks = (masks != 0).int()
        masks = masks.contiguous()
        gt = torch.as_tensor(gt_ids, device=dev).to(torch.int64).contiguous()
        cls = self._dev_classes.get(dev)
        if cls is None:
            cls = self._dev_classes[dev] = torch.tensor(self.class_ids, dtype=torch.int32, device=dev)
        labels = torch.as_tensor(label_ids, device=dev)
        scores = torch.as_tensor(scores, device=dev)
        rows = None
        if pick is not None:
            rows = torch.as_tensor(pick, device=dev).to(torch.int32).contiguous()
            labels, scores = labels[rows.long()], scores[rows.long()]
        n = masks.shape[0] if rows is None else rows.shape[0]
        sdt = scores.dtype if scores.dtype in (torch.float32, torch.float64) else torch.float32
        sw = n * (2 if sdt == torch.float64 else 1)
        while True:
            buf, lay = pointops.instance_overlaps_packed(masks, gt, cls, rows, self.max_gt, extra_words=2 * n + sw)
            e = lay["extra"]
            if n:  # the predictions' labels and scores ride along in the same copy
                buf[e:e + 2 * n].view(torch.int64).copy_(labels.to(torch.int64))
                buf[e + 2 * n:e + 2 * n + sw].view(sdt).copy_(scores.to(sdt))
            h = buf.cpu().numpy()
            G = int(h[0])
            if G <= self.max_gt:
                break
            self.max_gt = G  # the instance tables were too small: nothing was written past them, run again
        gt_id = h[lay["id"]:lay["id"] + 2 * G].view(np.int64)
        gt_count = h[lay["count"]:lay["count"] + G].astype(np.int64)
        inter = h[lay["inter"]:lay["inter"] + n * (G + 1)].reshape(n, G + 1).astype(np.int64)
        labels = h[e:e + 2 * n].view(np.int64)
        conf = h[e + 2 * n:e + 2 * n + sw].view(np.float64 if sdt == torch.float64 else np.float32)
        return gt_id, gt_count, inter, labels, conf

    def evaluate(self):
        """(ap [C, n_overlaps], summary dict with all_ap, all_ap_50%, all_ap_25% and classes[name][ap | ap50% | ap25%])."""
        scenes = [[s.by_class(int(c)) for c in self.class_ids] for s in self.scenes]
        ap = _ap_table(scenes, len(self.class_ids), self.overlaps, self.min_region_size)
        return ap, _averages(ap, self.class_names, self.overlaps)

    def format_results(self, avgs=None):
        return format_results(self.evaluate()[1] if avgs is None else avgs)

    average_over_runs = staticmethod(average_over_runs)


# ---- the reference's interface (util/eval.py), with the class set as a keyword instead of the global cfg -------------
def assign_instances_for_scan(scene_name, pred_info, gt_ids, *, classes=0, min_region_size=MIN_REGION_SIZE):
    """(gt2pred, pred2gt) of one scene in the reference's dict shapes; pred_info: {"conf", "label_id", "mask"}."""
    ids, names = class_set(classes)
    gt_id, gt_count, inter = scene_overlaps_host(pred_info["mask"], gt_ids, ids)
    name_of = dict(zip(ids.tolist(), names))
    gt2pred = {nm: [] for nm in names}
    col = {}
    for g, (i, c) in enumerate(zip(gt_id.tolist(), gt_count.tolist())):
        col[g] = {"instance_id": i, "label_id": i // 1000, "vert_count": c, "med_dist": -1, "dist_conf": 0.0,
                  "matched_pred": []}
        gt2pred[name_of[i // 1000]].append(col[g])
    pred2gt = {nm: [] for nm in names}
    n_kept = 0
    for i in range(inter.shape[0]):
        label = int(pred_info["label_id"][i])
        count = int(inter[i].sum())
        if label not in name_of or count < min_region_size:
            continue
        pred = {"filename": f"{scene_name}_{n_kept:03d}", "pred_id": n_kept, "label_id": label, "vert_count": count,
                "confidence": pred_info["conf"][i], "void_intersection": int(inter[i, -1])}
        matched = []
        for g in range(len(gt_id)):
            if gt_id[g] // 1000 == label and inter[i, g] > 0:
                matched.append(dict(col[g], intersection=int(inter[i, g])))
                col[g]["matched_pred"].append(dict(pred, intersection=int(inter[i, g])))
        pred["matched_gt"] = matched
        pred2gt[name_of[label]].append(pred)
        n_kept += 1
    return gt2pred, pred2gt


def evaluate_matches(matches, *, classes=0, min_region_size=MIN_REGION_SIZE, overlaps=DEFAULT_OVERLAPS):
    """AP [1, C, n_overlaps] of {scene: {"gt": gt2pred, "pred": pred2gt}} as assign_instances_for_scan builds them."""
    _, names = class_set(classes)
    scenes = []
    for m in matches.values():
        per = []
        for nm in names:
            gts = [(g["instance_id"], g["vert_count"],
                    [(p["filename"], p["vert_count"], float(p["confidence"]), p["intersection"]) for p in g["matched_pred"]])
                   for g in m["gt"][nm]]
            preds = [(p["filename"], float(p["confidence"]), p["vert_count"], p["void_intersection"],
                      [(g["instance_id"], g["vert_count"], g["intersection"]) for g in p["matched_gt"]])
                     for p in m["pred"][nm]]
            per.append((gts, preds))
        scenes.append(per)
    return _ap_table(scenes, len(names), tuple(overlaps), min_region_size)[None]


def compute_averages(aps, *, classes=0, overlaps=DEFAULT_OVERLAPS):
    """The summary dict of an AP array [1, C, n_overlaps] (evaluate_matches' shape)."""
    _, names = class_set(classes)
    return _averages(np.asarray(aps)[0], names, overlaps)


# ---- semantic segmentation: predictions, confusion matrices, IoU -------------------------------------------------------
# The semantic head is the model's foreground filter (geoformer.py:423-429: pred >= 4, or pred == 3 across folds) and the
# only thing trained in the first prepare_epochs.  Its classes are the training labels of
# datasets/scannetv2_inst.py:314-323: wall, floor, "unannotated" (raw -100, trained as a class), "candidate" (every
# class of the other fold) and the train fold's nine classes.
SEMANTIC_FG_CLASS = 4         # classes >= 4: the fold's instance classes
SEMANTIC_CANDIDATE_CLASS = 3  # the other fold's classes
DATASET_LABEL_NAMES = ("wall", "floor") + CLASS_NAMES  # raw dataset labels 0..19 (BENCHMARK_SEMANTIC_LABELS' order)
IGNORE_LABEL = -100


def semantic_label_lut(train_fold):
    """(lut int32 [20], map_ignore, map_other) of raw ScanNet labels for a train fold, as
    datasets/scannetv2_inst.py:314-323 relabels a scene: 0 -> 0, 1 -> 1, the fold's classes -> 4 + i, -100 -> 2
    (map_ignore), everything else -> 3 (map_other)."""
    fold = FOLD_SEMANTIC_LABELS[int(train_fold)]
    lut = np.full(len(BENCHMARK_SEMANTIC_LABELS), SEMANTIC_CANDIDATE_CLASS, dtype=np.int32)
    lut[0], lut[1] = 0, 1
    for i, c in enumerate(fold):
        lut[c] = SEMANTIC_FG_CLASS + i
    return lut, 2, SEMANTIC_CANDIDATE_CLASS


def SEMANTIC_CLASS_NAMES(train_fold):
    """Names of the semantic head's 13 classes for a train fold, in class order."""
    return ("wall", "floor", "unannotated", "candidate") + tuple(
        DATASET_LABEL_NAMES[c] for c in FOLD_SEMANTIC_LABELS[int(train_fold)])


def semantic_preds_host(scores):
    """numpy statement of the native arg-max: the first maximal class of every row of scores [N, C] (start from class 0,
    replace on strict '>' in ascending class order), int32 [N].  A NaN wins only in column 0.  On rows without ties or
    NaNs this is scores.max(1)[1]."""
    s = np.asarray(scores, dtype=np.float32)
    if s.ndim != 2 or s.shape[1] < 1:
        raise ValueError(f"scores {s.shape}: expected [N, C]")
    mx = s[:, 0].copy()
    arg = np.zeros(s.shape[0], dtype=np.int32)
    for k in range(1, s.shape[1]):
        w = s[:, k] > mx
        mx[w] = s[w, k]
        arg[w] = k
    return arg


def map_semantic_labels(labels, n_classes, lut=None, ignore_label=IGNORE_LABEL, map_ignore=-1, map_other=-1):
    """The confusion matrix's row of every label, int64: map_ignore for ignore_label, lut[label] inside the table (the
    identity over 0..n_classes-1 without one), map_other outside; a mapped value outside 0..n_classes-1 becomes
    n_classes (ignored)."""
    g = np.asarray(labels).astype(np.int64)
    table = np.arange(n_classes, dtype=np.int64) if lut is None else np.asarray(lut, dtype=np.int64)
    inside = (g >= 0) & (g < len(table))
    m = np.full(g.shape, int(map_other), dtype=np.int64)
    m[inside] = table[g[inside]]
    m[g == ignore_label] = int(map_ignore)
    m[(m < 0) | (m >= n_classes)] = n_classes
    return m


def semantic_confusion_host(scores, labels, offsets=None, *, lut=None, ignore_label=IGNORE_LABEL, map_ignore=-1,
                            map_other=-1):
    """numpy statement of gf_semantic_confusion: (preds int32 [N], conf int64 [S, C+1, C]) of S scenes packed one after
    the other (offsets [S+1], default one scene); conf[s, row, pred] with row the mapped label, C for ignored ones."""
    preds = semantic_preds_host(scores)
    N, C = np.asarray(scores).shape
    off = np.array([0, N], dtype=np.int64) if offsets is None else np.asarray(offsets).astype(np.int64)
    if off.ndim != 1 or len(off) < 1 or off[0] != 0 or off[-1] != N or (np.diff(off) < 0).any():
        raise ValueError(f"offsets {off.tolist()[:8]}...: ascending from 0 to N = {N}")
    S = len(off) - 1
    rows = map_semantic_labels(labels, C, lut, ignore_label, map_ignore, map_other)
    if rows.shape != (N,):
        raise ValueError(f"labels {rows.shape} against {N} points")
    sc = np.repeat(np.arange(S, dtype=np.int64), np.diff(off))
    bins = (C + 1) * C
    conf = np.bincount(sc * bins + rows * C + preds, minlength=S * bins).reshape(S, C + 1, C).astype(np.int64)
    return preds, conf


def _ratio(a, b):
    return float(a) / float(b) if b else float("nan")


def _filter_quality(tp, n_pred, n_gt):
    return {"precision": _ratio(tp, n_pred), "recall": _ratio(tp, n_gt), "iou": _ratio(tp, n_pred + n_gt - tp)}


def semantic_metrics(conf, names=None, fg_class=SEMANTIC_FG_CLASS, candidate_class=SEMANTIC_CANDIDATE_CLASS):
    """The summary of a confusion matrix [C+1, C] (row = ground truth, C = ignored; column = prediction).  Points whose
    ground truth is ignored count nowhere (ScanNet's evaluate_semantic_label.py).  iou [C] = tp / (tp + fp + fn), nan
    for a class in neither prediction nor ground truth; miou: nan-mean over all classes, miou_fold over fg_class..C-1;
    acc = trace / points; macc: nan-mean of the per-class recall; foreground / candidate: precision, recall and IoU of
    the model's two point filters, pred >= fg_class against gt >= fg_class and pred == candidate_class against gt ==
    candidate_class (the recall is the share of those points the instance stage is shown)."""
    conf = np.asarray(conf, dtype=np.int64)
    C = conf.shape[1]
    if conf.shape != (C + 1, C):
        raise ValueError(f"confusion matrix {conf.shape}: expected [C+1, C]")
    m = conf[:C]
    tp = np.diag(m)
    n_gt, n_pred = m.sum(1), m.sum(0)
    denom = n_gt + n_pred - tp
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = np.where(denom > 0, tp / denom, np.nan)
        recall = np.where(n_gt > 0, tp / n_gt, np.nan)

    def nanmean(v):
        v = v[~np.isnan(v)]
        return float(v.mean()) if v.size else float("nan")

    names = [str(c) for c in range(C)] if names is None else list(names)
    res = {"classes": {n: {"iou": float(iou[c]), "recall": float(recall[c]), "points": int(n_gt[c])}
                       for c, n in enumerate(names)},
           "iou": iou, "miou": nanmean(iou), "miou_fold": nanmean(iou[fg_class:]),
           "acc": _ratio(tp.sum(), m.sum()), "macc": nanmean(recall),
           "points": int(m.sum()), "ignored": int(conf[C].sum()),
           "foreground": _filter_quality(m[fg_class:, fg_class:].sum(), m[:, fg_class:].sum(), m[fg_class:].sum())}
    if 0 <= candidate_class < C:
        c = candidate_class
        res["candidate"] = _filter_quality(tp[c], n_pred[c], n_gt[c])
    else:
        res["candidate"] = _filter_quality(0, 0, 0)
    return res


def format_semantic_results(res):
    """The summary as a printable table, in the style of format_results."""
    lines = ["#" * 64, f"{'what':<15}:{'IoU':>15}{'recall':>15}{'points':>15}", "#" * 64]
    for name, c in res["classes"].items():
        lines.append(f"{name:<15}:{c['iou']:>15.3f}{c['recall']:>15.3f}{c['points']:>15d}")
    lines.append("-" * 64)
    lines.append(f"{'mIoU':<15}:{res['miou']:>15.3f}{'mAcc':>10}{res['macc']:>10.3f}{'acc':>5}{res['acc']:>10.3f}")
    lines.append(f"{'mIoU (fold)':<15}:{res['miou_fold']:>15.3f}{'ignored':>15}{res['ignored']:>15d}")
    lines.append(f"{'filter':<15}:{'precision':>15}{'recall':>15}{'IoU':>15}")
    for key in ("foreground", "candidate"):
        f = res[key]
        lines.append(f"{key:<15}:{f['precision']:>15.3f}{f['recall']:>15.3f}{f['iou']:>15.3f}")
    return "\n".join(lines)


class SemanticEvaluator:
    """mIoU / accuracy of the semantic head and the quality of its foreground filter over a set of scenes.

        ev = SemanticEvaluator(n_classes=13, train_fold=0)
        preds = ev.add_batch(outputs["semantic_scores"], batch["labels"], batch["offsets"], names)
        res = ev.evaluate(); print(ev.format_results(res))

    raw_labels: the labels are raw dataset labels (0..19, -100) and go through semantic_label_lut(train_fold); False:
    they are training labels already (0..n_classes-1, -100 ignored).  Device tensors are counted by the native call
    into matrices that stay on the device: nothing crosses to the host before evaluate() / confusion() /
    scene_confusions().  Host arrays take the numpy path.  keep_scenes=False keeps the dataset total only."""

    def __init__(self, n_classes=13, train_fold=0, raw_labels=True, keep_scenes=True, fg_class=SEMANTIC_FG_CLASS,
                 candidate_class=SEMANTIC_CANDIDATE_CLASS):
        self.n_classes = int(n_classes)
        self.train_fold = int(train_fold)
        self.raw_labels = bool(raw_labels)
        self.keep_scenes = bool(keep_scenes)
        self.fg_class, self.candidate_class = int(fg_class), int(candidate_class)
        if self.raw_labels:
            self.lut, self.map_ignore, self.map_other = semantic_label_lut(self.train_fold)
        else:
            self.lut, self.map_ignore, self.map_other = None, -1, -1
        names = SEMANTIC_CLASS_NAMES(self.train_fold)
        self.class_names = list(names) if len(names) == self.n_classes else [str(c) for c in range(self.n_classes)]
        self.names = []      # scene names in the order added
        self._host = []      # [S, C+1, C] per host batch (keep_scenes) ...
        self._device = []    # ... (position in self.names, device tensor) per device batch
        self._total_host = np.zeros((self.n_classes + 1, self.n_classes), dtype=np.int64)
        self._total_dev = {}  # device -> running total (keep_scenes=False)
        self._dev_lut = {}

    def _map_kw(self):
        return {"ignore_label": IGNORE_LABEL, "map_ignore": self.map_ignore, "map_other": self.map_other}

    def add_batch(self, scores, labels, offsets=None, names=None, offsets_host=None):
        """One batch of S scenes packed one after the other: scores [N, n_classes], labels [N], offsets [S+1] (default:
        one scene), names: S scene names (default: their running numbers).  offsets_host: the caller's host copy of
        device offsets (int32), which lets the native call refuse a malformed table before it launches.  Returns preds
        int32 [N], where the scores live."""
        S = 1 if offsets is None else int(offsets.shape[0]) - 1
        names = [f"scene{len(self.names) + i:04d}" for i in range(S)] if names is None else list(names)
        if len(names) != S:
            raise ValueError(f"add_batch: {len(names)} names for {S} scenes")
        if scores.shape[1] != self.n_classes:
            raise ValueError(f"add_batch: scores {tuple(scores.shape)} for {self.n_classes} classes")
        if _is_tensor(scores) and scores.is_cuda:
            preds = self._add_device(scores, labels, offsets, offsets_host, S, len(self.names))
        else:
            host = [x.detach().cpu().numpy() if _is_tensor(x) else x for x in (scores, labels, offsets)]
            preds, conf = semantic_confusion_host(host[0], host[1], host[2], lut=self.lut, **self._map_kw())
            if self.keep_scenes:
                self._host.append((len(self.names), conf))
            else:
                self._total_host += conf.sum(0)
        self.names += names
        return preds

    def _add_device(self, scores, labels, offsets, offsets_host, S, at):
        import torch

        from . import pointops

        dev = scores.device
        lut = None
        if self.lut is not None:
            lut = self._dev_lut.get(dev)
            if lut is None:
                lut = self._dev_lut[dev] = torch.from_numpy(self.lut).to(dev)
        if offsets is None:
            offsets_host = torch.tensor([0, scores.shape[0]], dtype=torch.int32)
            offsets = offsets_host.to(dev)
        elif not offsets.is_cuda:
            offsets_host = offsets.to(torch.int32).contiguous()
            offsets = offsets_host.to(dev)
        if offsets.dtype != torch.int32:
            offsets = offsets.to(torch.int32)
        labels = torch.as_tensor(labels).to(dev, torch.int64).contiguous()
        conf = torch.zeros((S, self.n_classes + 1, self.n_classes), dtype=torch.int64, device=dev)
        preds = pointops.semantic_confusion(scores.contiguous(), labels, offsets.contiguous(), conf, lut=lut,
                                            offsets_host=offsets_host, **self._map_kw())
        if self.keep_scenes:
            self._device.append((at, conf))
        elif dev in self._total_dev:
            self._total_dev[dev] += conf.sum(0)
        else:
            self._total_dev[dev] = conf.sum(0)
        return preds

    def _collect(self):
        """Every device matrix to the host (one copy per device), merged with the host ones in scene order."""
        if self._device:
            import torch

            by_dev = {}
            for at, conf in self._device:
                by_dev.setdefault(conf.device, []).append((at, conf))
            for items in by_dev.values():
                h = torch.cat([c for _, c in items]).cpu().numpy()
                k = 0
                for at, c in items:
                    self._host.append((at, h[k:k + c.shape[0]]))
                    k += c.shape[0]
            self._device = []
            self._host.sort(key=lambda e: e[0])
        for dev in list(self._total_dev):
            self._total_host += self._total_dev.pop(dev).cpu().numpy()

    def scene_confusions(self):
        """{scene name: confusion matrix [C+1, C]} of the scenes added so far (keep_scenes=True)."""
        if not self.keep_scenes:
            raise ValueError("scene_confusions: the evaluator was made with keep_scenes=False")
        self._collect()
        out = {}
        for at, conf in self._host:
            for i in range(conf.shape[0]):
                out[self.names[at + i]] = conf[i]
        return out

    def confusion(self):
        """The dataset's confusion matrix [C+1, C]."""
        self._collect()
        total = self._total_host.copy()
        for _, conf in self._host:
            total += conf.sum(0)
        return total

    def evaluate(self):
        """semantic_metrics of the dataset total (classes named by SEMANTIC_CLASS_NAMES(train_fold))."""
        return semantic_metrics(self.confusion(), self.class_names, self.fg_class, self.candidate_class)

    def format_results(self, res=None):
        return format_semantic_results(self.evaluate() if res is None else res)


# ---- panoptic segmentation: things from the label map, stuff from the semantic head; PQ / SQ / RQ -------------------
# Written from the published definition (Kirillov et al., "Panoptic Segmentation", CVPR 2019) and the matching rules of
# its public evaluation: a predicted and a ground-truth segment of one class match iff their IoU, with the prediction's
# void points taken out of the union, exceeds 0.5 (which makes the matching unique).  The per-scene contingency tables
# come from gf_panoptic_overlaps (csrc/panoptic.hip) or from panoptic_overlaps_host, its numpy statement.
DEFAULT_STUFF_IDS = (1, 2)  # nyu40 wall, floor: classes 0 and 1 of the semantic head
STUFF_NAMES = {1: "wall", 2: "floor"}


class PanopticTable(NamedTuple):
    """One scene's contingency table.  Rows: the p thing rows (rank order of pick), one row per stuff class
    (class_ids order), the unlabelled row; columns: the G ground-truth segments in ascending key order, void last."""
    gt_id: object     # int64 [G]: the id of a thing instance, nyu40 id * 1000 of a stuff segment
    inter: object     # int64 [p + n_stuff + 1, G + 1]
    label_id: object  # int64 [p]: nyu40 class of every thing row
    class_ids: object  # int64 [C]: the evaluated classes
    is_stuff: object  # bool [C]


def panoptic_class_tables(classes=0, stuff=DEFAULT_STUFF_IDS, stuff_of_sem=None):
    """(class_ids int64 [C], is_stuff bool [C], stuff_of_sem int32 [L], names) of a panoptic class set: the stuff classes
    first, then the thing classes of class_set(classes).  stuff_of_sem: semantic class -> index into class_ids of a stuff
    class or -1; default: semantic class j is the j-th stuff class (wall, floor: the semantic head's classes 0, 1)."""
    stuff = tuple(int(c) for c in stuff)
    things, thing_names = class_set(classes)
    ids = np.concatenate([np.asarray(stuff, dtype=np.int64), things])
    if len(set(ids.tolist())) != len(ids) or (ids <= 0).any():
        raise ValueError("panoptic classes: distinct positive nyu40 ids, no class both stuff and thing")
    is_stuff = np.arange(len(ids)) < len(stuff)
    sos = np.arange(len(stuff), dtype=np.int32) if stuff_of_sem is None else np.asarray(stuff_of_sem, dtype=np.int32)
    names = [STUFF_NAMES.get(c, str(c)) for c in stuff] + list(thing_names)
    return ids, is_stuff, sos, names


def panoptic_overlaps_host(owner, sem, gt_ids, offsets=None, *, class_ids, is_stuff, stuff_of_sem, P, ids=None,
                           max_gt=None):
    """numpy statement of gf_panoptic_overlaps: (pan int32 [N] or None without ids, G int32 [S], gt_id int64 [S, max_gt],
    inter int64 [S, R, max_gt + 1]) of S scenes packed one after the other (offsets [S+1], default one scene), with
    R = P + n_stuff + 1 rows (things by owner, stuff classes in class_ids order, unlabelled) and the void points in the
    last column.  max_gt: default the largest G of the batch; a scene with G > max_gt reports G alone (zeros)."""
    owner = np.asarray(owner).astype(np.int64)
    sem = np.asarray(sem).astype(np.int64)
    gt = np.asarray(gt_ids).astype(np.int64)
    N = owner.shape[0]
    if owner.shape != (N,) or sem.shape != (N,) or gt.shape != (N,):
        raise ValueError(f"owner {owner.shape}, sem {sem.shape}, gt_ids {gt.shape}: one value per point")
    off = np.array([0, N], dtype=np.int64) if offsets is None else np.asarray(offsets).astype(np.int64)
    if off.ndim != 1 or len(off) < 1 or off[0] != 0 or off[-1] != N or (np.diff(off) < 0).any():
        raise ValueError(f"offsets {off.tolist()[:8]}...: ascending from 0 to N = {N}")
    S = len(off) - 1
    cls = np.asarray(class_ids, dtype=np.int64)
    st = np.asarray(is_stuff).astype(bool)
    sos = np.asarray(stuff_of_sem, dtype=np.int64).reshape(-1)
    C, L, P = len(cls), len(sos), int(P)
    n_stuff = int(st.sum())
    R = P + n_stuff + 1
    srank = np.where(st, np.cumsum(st) - 1, -1)  # rank among the stuff classes in class_ids order
    # predicted rows
    row = np.full(N, R - 1, dtype=np.int64)
    label = np.zeros(N, dtype=np.int64)
    thing = (owner >= 0) & (owner < P)
    c = np.full(N, -1, dtype=np.int64)
    ins = ~thing & (sem >= 0) & (sem < L)
    c[ins] = sos[sem[ins]]
    c[(c < 0) | (c >= C)] = -1
    stuff = c >= 0
    stuff[stuff] = srank[c[stuff]] >= 0
    row[thing] = owner[thing]
    row[stuff] = P + srank[c[stuff]]
    label[stuff] = cls[c[stuff]] * 1000
    pan = None
    if ids is not None:
        label[thing] = np.asarray(ids).astype(np.int64)[thing]
        pan = label.astype(np.int32)
    # ground-truth keys
    q = gt // 1000
    order = np.argsort(cls, kind="stable")
    pos = np.searchsorted(cls[order], q)
    hit = (pos < C) & (cls[order][np.minimum(pos, C - 1)] == q)
    rank = np.where(hit, pos, -1)  # rank of q among the class ids
    at = order[np.minimum(pos, C - 1)]  # index into class_ids
    key = np.where(hit, rank * 1000 + np.where(st[at], 0, gt - q * 1000), -1)
    sorted_cls = cls[order]
    Gs = np.zeros(S, dtype=np.int32)
    uniq, cols = [], []
    for s in range(S):
        k = key[off[s]:off[s + 1]]
        u, inv = np.unique(k[k >= 0], return_inverse=True)
        col = np.full(k.shape[0], -1, dtype=np.int64)
        col[k >= 0] = inv
        Gs[s] = len(u)
        uniq.append(u)
        cols.append(col)
    max_gt = int(Gs.max()) if max_gt is None and S else int(max_gt or 0)
    gt_id = np.zeros((S, max_gt), dtype=np.int64)
    inter = np.zeros((S, R, max_gt + 1), dtype=np.int64)
    for s in range(S):
        G = int(Gs[s])
        if G > max_gt:
            continue
        gt_id[s, :G] = sorted_cls[uniq[s] // 1000] * 1000 + uniq[s] % 1000
        col = np.where(cols[s] >= 0, cols[s], max_gt)
        inter[s] = np.bincount(row[off[s]:off[s + 1]] * (max_gt + 1) + col,
                               minlength=R * (max_gt + 1)).reshape(R, max_gt + 1)
    return pan, Gs, gt_id, inter


def panoptic_tables(Gs, gt_id, inter, label_ids, class_ids, is_stuff, P):
    """One PanopticTable per scene from the batch tables of gf_panoptic_overlaps / panoptic_overlaps_host: the thing
    rows beyond a scene's own p = len(label_ids[s]) are dropped (points there mean an owner without a table row)."""
    cls = np.asarray(class_ids, dtype=np.int64)
    st = np.asarray(is_stuff).astype(bool)
    out = []
    for s in range(len(Gs)):
        G = int(Gs[s])
        lab = np.asarray(label_ids[s], dtype=np.int64).reshape(-1)
        p = len(lab)
        if p > P or inter[s, p:P].any():
            raise ValueError(f"scene {s}: owners beyond its {p} picked instances")
        it = np.asarray(inter[s], dtype=np.int64)
        it = np.concatenate([it[:p], it[P:]])
        out.append(PanopticTable(np.asarray(gt_id[s, :G], dtype=np.int64), np.concatenate([it[:, :G], it[:, -1:]], 1),
                                 lab, cls, st))
    return out


def _panoptic_scene_counts(table):
    """(tp, fp, fn int64 [C], iou float64 [C]) of one scene, per class of table.class_ids."""
    cls = np.asarray(table.class_ids, dtype=np.int64)
    st = np.asarray(table.is_stuff).astype(bool)
    inter = np.asarray(table.inter, dtype=np.int64)
    lab = np.asarray(table.label_id, dtype=np.int64)
    C, p, G = len(cls), len(lab), inter.shape[1] - 1
    if inter.shape[0] != p + int(st.sum()) + 1 or len(table.gt_id) != G:
        raise ValueError(f"panoptic table {inter.shape} for {p} thing rows, {int(st.sum())} stuff classes, "
                         f"{len(table.gt_id)} segments")
    pred_cls = np.concatenate([lab, cls[st]])  # (the unlabelled row is no segment)
    size_r = inter[:-1].sum(1)
    void_r = inter[:-1, G]
    size_g = inter[:, :G].sum(0)
    gt_cls = np.asarray(table.gt_id, dtype=np.int64) // 1000
    bad = (size_r[:p] > 0) & ~np.isin(lab, cls)
    if bad.any():
        raise ValueError(f"thing row {int(np.nonzero(bad)[0][0])} has class {int(lab[bad][0])}, outside the evaluated set")
    I = inter[:-1, :G]
    union = size_r[:, None] + size_g[None, :] - I - void_r[:, None]
    match = (pred_cls[:, None] == gt_cls[None, :]) & (2 * I > union) & (size_r[:, None] > 0) & (size_g[None, :] > 0)
    tp, fp, fn = (np.zeros(C, dtype=np.int64) for _ in range(3))
    iou = np.zeros(C, dtype=np.float64)
    index = {int(c): i for i, c in enumerate(cls)}
    for r, g in zip(*np.nonzero(match)):
        i = index[int(gt_cls[g])]
        tp[i] += 1
        iou[i] += float(I[r, g]) / float(union[r, g])
    for g in np.nonzero((size_g > 0) & ~match.any(0))[0]:
        fn[index[int(gt_cls[g])]] += 1
    for r in np.nonzero((size_r > 0) & ~match.any(1) & ~(2 * void_r > size_r))[0]:
        fp[index[int(pred_cls[r])]] += 1
    return tp, fp, fn, iou


def _pq_summary(tp, fp, fn, iou, class_ids, is_stuff, names=None):
    tp, fp, fn = (np.asarray(a, dtype=np.int64) for a in (tp, fp, fn))
    iou = np.asarray(iou, dtype=np.float64)
    st = np.asarray(is_stuff).astype(bool)
    denom = tp + 0.5 * fp + 0.5 * fn
    seen = (tp + fp + fn) > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        pq = np.where(seen, iou / denom, np.nan)
        sq = np.where(seen, np.where(tp > 0, iou / np.maximum(tp, 1), 0.0), np.nan)
        rq = np.where(seen, tp / denom, np.nan)

    def mean(v, sel):
        v = v[sel & seen]
        return float(v.mean()) if v.size else float("nan")

    names = [STUFF_NAMES.get(int(c), dict(zip(VALID_CLASS_IDS, CLASS_NAMES)).get(int(c), str(int(c))))
             for c in class_ids] if names is None else list(names)
    res = {"class_ids": np.asarray(class_ids, dtype=np.int64), "is_stuff": st, "tp": tp, "fp": fp, "fn": fn,
           "iou_sum": iou, "classes": {}}
    every = np.ones(len(st), dtype=bool)
    for tag, sel in (("", every), ("_th", ~st), ("_st", st)):
        res["pq" + tag], res["sq" + tag], res["rq" + tag] = mean(pq, sel), mean(sq, sel), mean(rq, sel)
    for i, n in enumerate(names):
        res["classes"][n] = {"pq": float(pq[i]), "sq": float(sq[i]), "rq": float(rq[i]), "tp": int(tp[i]),
                             "fp": int(fp[i]), "fn": int(fn[i]), "stuff": bool(st[i])}
    return res


def panoptic_quality(tables, names=None):
    """PQ / SQ / RQ of a set of scenes' PanopticTables (one class set): per class PQ = sum of the matched IoUs /
    (TP + FP / 2 + FN / 2), SQ = that sum / TP (0 without a match), RQ = TP / (TP + FP / 2 + FN / 2); a class with no
    TP, FP or FN is nan and left out of the means.  Keys: pq, sq, rq (all classes), *_th (things), *_st (stuff),
    classes[name], and the per-class arrays tp, fp, fn, iou_sum.  A predicted segment more than half void is no FP; a
    pair at IoU 0.5 exactly is no match (decided in integers)."""
    tables = list(tables)
    if not tables:
        raise ValueError("panoptic_quality: no scene")
    cls, st = np.asarray(tables[0].class_ids, dtype=np.int64), np.asarray(tables[0].is_stuff).astype(bool)
    tot = [np.zeros(len(cls), dtype=np.int64) for _ in range(3)] + [np.zeros(len(cls), dtype=np.float64)]
    for t in tables:
        if not (np.array_equal(np.asarray(t.class_ids, dtype=np.int64), cls)
                and np.array_equal(np.asarray(t.is_stuff).astype(bool), st)):
            raise ValueError("panoptic_quality: the scenes' class sets differ")
        for a, b in zip(tot, _panoptic_scene_counts(t)):
            a += b
    return _pq_summary(*tot, cls, st, names)


def format_panoptic_results(res):
    """The summary as a printable table, in the style of format_results."""
    lines = ["#" * 64, f"{'what':<15}:{'PQ':>10}{'SQ':>10}{'RQ':>10}{'TP':>6}{'FP':>6}{'FN':>6}", "#" * 64]
    for name, c in res["classes"].items():
        lines.append(f"{name:<15}:{c['pq']:>10.3f}{c['sq']:>10.3f}{c['rq']:>10.3f}{c['tp']:>6d}{c['fp']:>6d}{c['fn']:>6d}")
    lines.append("-" * 64)
    for what, tag in (("all", ""), ("things", "_th"), ("stuff", "_st")):
        lines.append(f"{what:<15}:{res['pq' + tag]:>10.3f}{res['sq' + tag]:>10.3f}{res['rq' + tag]:>10.3f}")
    return "\n".join(lines)


class PanopticEvaluator:
    """PQ / SQ / RQ of panoptic labellings over a set of scenes.

        ev = PanopticEvaluator(classes=0, stuff=(1, 2))
        pan = ev.add_batch(owner, ids, sem, gt_ids, offsets, label_ids, names)   # S scenes packed one after the other
        res = ev.evaluate(); print(ev.format_results(res))

    classes: the thing classes (cvfold 0 / 1, "all" or nyu40 ids); stuff: the nyu40 ids of the stuff classes;
    stuff_of_sem: semantic class -> index of its stuff class among `stuff`, or -1 (default: class j is stuff[j]).
    Device tensors are counted by gf_panoptic_overlaps (one device-to-host copy of the tables per batch), host arrays
    by panoptic_overlaps_host."""

    def __init__(self, classes=0, stuff=DEFAULT_STUFF_IDS, stuff_of_sem=None):
        self.class_ids, self.is_stuff, self.stuff_of_sem, self.class_names = panoptic_class_tables(classes, stuff,
                                                                                                   stuff_of_sem)
        self.n_stuff = int(self.is_stuff.sum())
        self.max_gt = DEFAULT_MAX_GT
        self.names = []
        self.tables = []
        self._dev = {}

    def device_tables(self, dev):
        """(class_ids, is_stuff, stuff_of_sem) as int32 tensors on `dev`."""
        t = self._dev.get(dev)
        if t is None:
            import torch

            t = self._dev[dev] = tuple(torch.as_tensor(np.asarray(a).astype(np.int32), device=dev)
                                       for a in (self.class_ids, self.is_stuff, self.stuff_of_sem))
        return t

    def add_batch(self, owner, ids, sem, gt_ids, offsets=None, label_ids=None, names=None, offsets_host=None):
        """One batch of S scenes packed one after the other: owner / ids [N] (the label map), sem [N] (the semantic
        head's classes), gt_ids [N] (val_gt ids, gt_ids_from_labels), offsets [S+1] (default one scene), label_ids: per
        scene the nyu40 class of every picked instance in rank order (InstanceTable.label_id).  Returns pan int32 [N],
        where the inputs live."""
        S = 1 if offsets is None else int(offsets.shape[0]) - 1
        names = [f"scene{len(self.names) + i:04d}" for i in range(S)] if names is None else list(names)
        label_ids = [np.asarray(l.detach().cpu() if _is_tensor(l) else l, dtype=np.int64).reshape(-1)
                     for l in (label_ids if label_ids is not None else [[]] * S)]
        if len(names) != S or len(label_ids) != S:
            raise ValueError(f"add_batch: {len(names)} names and {len(label_ids)} label tables for {S} scenes")
        if set(names) & set(self.names) or len(set(names)) != S:
            raise ValueError("add_batch: a scene was added already")
        P = max([len(l) for l in label_ids] + [0])
        if _is_tensor(owner) and owner.is_cuda:
            import torch

            from . import pointops

            dev = owner.device
            cls, st, sos = self.device_tables(dev)
            if offsets is None:
                offsets_host = torch.tensor([0, owner.shape[0]], dtype=torch.int32)
                offsets = offsets_host.to(dev)
            elif not offsets.is_cuda:
                offsets_host = offsets.to(torch.int32).contiguous()
                offsets = offsets_host.to(dev)
            i32 = lambda a: torch.as_tensor(a, device=dev).to(torch.int32).contiguous()  # noqa: E731
            gt = torch.as_tensor(gt_ids, device=dev).to(torch.int64).contiguous()
            pan, Gs, gt_id, inter, self.max_gt = pointops.panoptic_overlaps(
                i32(owner), i32(ids), i32(sem), gt, i32(offsets), cls, st, sos, self.n_stuff, P, max_gt=self.max_gt,
                offsets_host=offsets_host)
        else:
            h = lambda a: a.detach().cpu().numpy() if _is_tensor(a) else (None if a is None else np.asarray(a))  # noqa: E731
            pan, Gs, gt_id, inter = panoptic_overlaps_host(h(owner), h(sem), h(gt_ids), h(offsets),
                                                           class_ids=self.class_ids, is_stuff=self.is_stuff,
                                                           stuff_of_sem=self.stuff_of_sem, P=P, ids=h(ids))
        self.tables += panoptic_tables(Gs, gt_id, inter, label_ids, self.class_ids, self.is_stuff, P)
        self.names += names
        return pan

    def add_scene(self, name, owner, ids, sem, gt_ids, label_id):
        """One scene: add_batch with a single scene."""
        return self.add_batch(owner, ids, sem, gt_ids, None, [label_id], [name])

    def scene_tables(self):
        """{scene name: PanopticTable} of the scenes added so far."""
        return dict(zip(self.names, self.tables))

    def evaluate(self):
        """panoptic_quality of the scenes added so far."""
        return panoptic_quality(self.tables, self.class_names)

    def format_results(self, res=None):
        return format_panoptic_results(self.evaluate() if res is None else res)


# ---- box AP: detection mAP over the instances' 3D boxes (csrc/boxes.hip) ------------------------------------------------
BOX_KINDS = ("aligned", "oriented")
BOX_OVERLAPS = (0.25, 0.5)


class _BoxScene:
    """What a scene leaves behind for the box AP: its instances (ids ascending, point counts) and its predictions in
    pick order (nyu40 label, confidence, point count, IoU with every instance's box)."""

    __slots__ = ("name", "gt_id", "gt_count", "label", "conf", "count", "iou")

    def __init__(self, name, gt_id, gt_count, label, conf, count, iou):
        self.name = name
        self.gt_id = np.asarray(gt_id, dtype=np.int64)
        self.gt_count = np.asarray(gt_count, dtype=np.int64)
        self.label = np.asarray(label, dtype=np.int64)
        self.conf = np.asarray(conf, dtype=np.float64)
        self.count = np.asarray(count, dtype=np.int64)
        self.iou = np.asarray(iou, dtype=np.float64).reshape(self.label.shape[0], self.gt_id.shape[0])

    def tables(self):
        return {k: getattr(self, k) for k in self.__slots__}


def _box_ap(scenes, cid, threshold, min_points):
    """(AP, recall) of class cid at one IoU threshold over the scenes, or (nan, nan) without an instance of the class.
    Predictions in descending score order (stable: ties keep scene order, then pick rank); a prediction is a true
    positive when its highest IoU among its own scene's boxes of the class (the lowest index among equals) is above the
    threshold and that box is unclaimed; AP is the area under the monotone precision envelope (VOC 2010, all points)."""
    conf, where, cand, n_gt = [], [], [], 0
    for si, s in enumerate(scenes):
        g = np.nonzero((s.gt_id // 1000 == cid) & (s.gt_count >= min_points))[0]
        cand.append(g)
        n_gt += g.shape[0]
        for r in np.nonzero((s.label == cid) & (s.count >= min_points))[0]:
            conf.append(s.conf[r])
            where.append((si, r))
    if n_gt == 0:
        return float("nan"), float("nan")
    order = np.argsort(-np.asarray(conf, dtype=np.float64), kind="stable")
    claimed = [np.zeros(g.shape[0], dtype=bool) for g in cand]
    tp = np.zeros(order.shape[0])
    for k, j in enumerate(order):
        si, r = where[j]
        if cand[si].shape[0] == 0:
            continue
        row = scenes[si].iou[r, cand[si]]
        b = int(np.argmax(row))  # the first of the highest
        if row[b] > threshold and not claimed[si][b]:
            claimed[si][b] = True
            tp[k] = 1.0
    ctp = np.cumsum(tp)
    rec = ctp / n_gt
    prec = ctp / np.arange(1, order.shape[0] + 1)
    mrec = np.concatenate([[0.0], rec, [1.0]])
    mpre = np.maximum.accumulate(np.concatenate([[0.0], prec, [0.0]])[::-1])[::-1]
    i = np.nonzero(mrec[1:] != mrec[:-1])[0]
    return float(np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1])), float(rec[-1]) if rec.shape[0] else 0.0


def format_box_results(res):
    """BoxEvaluator.evaluate's dict as a printable table: per class AP and recall at every threshold, then the means."""
    ov = [f"{t:g}" for t in res["overlaps"]]
    head = "".join(f"{'AP@' + o:>12}{'AR@' + o:>12}" for o in ov)
    w = 15 + 1 + 24 * len(ov)
    lines = ["#" * w, f"{'box ' + res['kind']:<15}:{head}", "#" * w]
    for name, c in res["classes"].items():
        lines.append(f"{name:<15}:" + "".join(f"{c['ap@' + o]:>12.3f}{c['recall@' + o]:>12.3f}" for o in ov))
    lines.append("-" * w)
    lines.append(f"{'mean':<15}:" + "".join(f"{res['mAP@' + o]:>12.3f}{res['mAR@' + o]:>12.3f}" for o in ov))
    return "\n".join(lines)


class BoxEvaluator:
    """Box AP of instance predictions over a set of scenes: detection mAP over the 3D boxes of the predicted masks
    against the boxes of the ground-truth instances (the ScanNet detection protocol of VoteNet: mAP@0.25 / mAP@0.5).

    classes: as InstanceEvaluator.  kind: "aligned" (axis-aligned boxes) or "oriented" (upright boxes of least footprint
    among `angles` headings, postprocess.instance_boxes).  overlaps: the IoU thresholds.  min_points: predictions and
    instances with fewer points are dropped.  The protocol is _box_ap's."""

    def __init__(self, classes=0, kind="aligned", overlaps=BOX_OVERLAPS, angles=90, min_points=1):
        from . import postprocess

        if kind not in BOX_KINDS:
            raise ValueError(f"BoxEvaluator: kind must be one of {BOX_KINDS}, got {kind!r}")
        postprocess.box_angle_table(angles)  # (checks the range)
        self.class_ids, self.class_names = class_set(classes)
        self.kind = kind
        self.overlaps = tuple(float(o) for o in overlaps)
        self.angles = int(angles) if kind == "oriented" else 1
        self.min_points = int(min_points)
        self.scenes = []
        self._dev_classes = {}

    def add_scene(self, name, gt_ids, label_ids, scores, masks, pick, xyz):
        """One scene's predictions: masks [n_rows, N] (nonzero = member; [] without proposals), label_ids [n_rows] nyu40
        ids, scores [n_rows], pick: the rows to evaluate, in order (None: all rows), gt_ids [N] val_gt ids
        (gt_ids_from_labels), xyz [N, 3].  The ground-truth boxes are those of the ids >= 1000 whose class is in the
        class set, in ascending id order.  Device tensors (xyz on the GPU): one gf_instance_boxes_batched call for both
        sets of boxes, one gf_box_iou_batched call and one device-to-host copy of the IoU block with the counts; host
        arrays: the numpy statements, with the same tables."""
        if any(s.name == name for s in self.scenes):
            raise ValueError(f"scene {name!r} was added already")
        if _is_tensor(xyz) and xyz.is_cuda:
            self.scenes.append(_BoxScene(name, *self._tables_device(gt_ids, label_ids, scores, masks, pick, xyz)))
        else:
            self.scenes.append(_BoxScene(name, *self._tables_host(gt_ids, label_ids, scores, masks, pick, xyz)))

    def _tables_host(self, gt_ids, label_ids, scores, masks, pick, xyz):
        from . import postprocess

        h = postprocess._np
        gt = np.asarray(h(gt_ids), dtype=np.int64).reshape(-1)
        valid = (gt >= 1000) & np.isin(gt // 1000, self.class_ids)
        gt_id, slot = np.unique(gt[valid], return_inverse=True)
        group = np.full(gt.shape[0], -1, np.int32)
        group[valid] = slot
        n = len(masks)
        pick = np.arange(n) if pick is None else np.asarray(h(pick), dtype=np.int64).reshape(-1)
        k = 2 if self.kind == "oriented" else 1
        pred = postprocess.instance_boxes_host(masks if n else [], pick, xyz, self.angles)
        inst = postprocess.id_boxes_host(group, gt_id.shape[0], xyz, self.angles)
        labels = np.asarray(h(label_ids), dtype=np.int64).reshape(-1)[pick]
        conf = np.asarray(h(scores), dtype=np.float64).reshape(-1)[pick]
        return gt_id, inst[0], labels, conf, pred[0], postprocess.box_iou_host(pred[k], inst[k])

    def _tables_device(self, gt_ids, label_ids, scores, masks, pick, xyz):
        import torch

        from . import postprocess

        dev = xyz.device
        cls = self._dev_classes.get(dev)
        if cls is None:
            cls = self._dev_classes[dev] = torch.tensor(self.class_ids, dtype=torch.int64, device=dev)
        gt = torch.as_tensor(gt_ids, device=dev).to(torch.int64).reshape(-1)
        valid = (gt >= 1000) & torch.isin(torch.div(gt, 1000, rounding_mode="floor"), cls)
        gt_id, slot = torch.unique(gt[valid], return_inverse=True)  # (ascending; its size is read back)
        group = torch.full((gt.shape[0],), -1, dtype=torch.int32, device=dev)
        group[valid] = slot.to(torch.int32)
        G = int(gt_id.shape[0])
        n = len(masks)
        pick = torch.arange(n, device=dev) if pick is None else torch.as_tensor(pick, device=dev).to(torch.int64).reshape(-1)
        P = int(pick.shape[0])
        _, count, aligned, oriented = postprocess._boxes_packed([("rows", masks if n else [], pick, xyz),
                                                                 ("ids", group, G, xyz)], self.angles)
        rows = oriented if self.kind == "oriented" else aligned
        iou = postprocess.box_iou_batched([rows[:P]], [rows[P:P + G]])[0]
        f64 = lambda t: torch.as_tensor(t, device=dev).to(torch.float64).reshape(-1)  # noqa: E731
        labels = f64(label_ids)[pick] if P else f64([])
        conf = f64(scores)[pick] if P else f64([])
        # the IoU block, the counts and what else the host keeps of the scene cross in one copy
        h = torch.cat([iou.reshape(-1), count.to(torch.float64), gt_id.to(torch.float64), labels, conf]).cpu().numpy()
        cut = np.cumsum([0, P * G, P, G, G, P, P])
        part = [h[cut[i]:cut[i + 1]] for i in range(6)]
        return part[3], part[2], part[4], part[5], part[1], part[0]

    def scene_tables(self):
        """Per scene, in the order added, the kept tables as a dict of numpy arrays (and the name)."""
        return [s.tables() for s in self.scenes]

    def evaluate(self):
        """{"kind", "overlaps", "ap" [C, T], "recall" [C, T], "mAP@t" / "mAR@t" per threshold t (means over the classes
        that have ground truth; nan without any), "classes": {name: {"ap@t", "recall@t"}}}; a class without ground
        truth is nan and left out of the means."""
        C, T = len(self.class_ids), len(self.overlaps)
        ap, rec = np.full((C, T), np.nan), np.full((C, T), np.nan)
        for ci, cid in enumerate(self.class_ids):
            for ti, t in enumerate(self.overlaps):
                ap[ci, ti], rec[ci, ti] = _box_ap(self.scenes, int(cid), t, self.min_points)
        res = {"kind": self.kind, "overlaps": self.overlaps, "ap": ap, "recall": rec, "classes": {}}
        has = ~np.isnan(ap[:, 0]) if T else np.zeros(C, dtype=bool)
        for ti, t in enumerate(self.overlaps):
            res[f"mAP@{t:g}"] = float(ap[has, ti].mean()) if has.any() else float("nan")
            res[f"mAR@{t:g}"] = float(rec[has, ti].mean()) if has.any() else float("nan")
        for ci, name in enumerate(self.class_names):
            res["classes"][name] = {f"{k}@{t:g}": float(v[ci, ti]) for ti, t in enumerate(self.overlaps)
                                    for k, v in (("ap", ap), ("recall", rec))}
        return res

    def format_results(self, res=None):
        return format_box_results(self.evaluate() if res is None else res)
