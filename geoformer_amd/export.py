"""Scene labels on disk: the ScanNet benchmark's instance-prediction files and one .npz per scene.

    labels = postprocess.label_points(masks, scores, label_ids, pick, xyz)          # or batch_eval.label_batches
    write_scannet_predictions("out", "scene0011_00", labels)                        # exclusive masks (owner == r)
    label_ids, scores, masks = read_scannet_predictions("out", "scene0011_00")

``<out_dir>/<name>.txt`` holds one ``predicted_masks/<name>_<rrr>.txt <label_id> <score>`` line per kept instance in
rank order, the mask file one ``0`` / ``1`` per line for each of the scene's N points: the benchmark's submission format,
and what util/visualize.py:212-227 reads (relative path, label, score).  Scores are printed as ``%.6f``.

    write_scannet_semantic("out/semantic", "scene0011_00", preds, train_fold=0)     # one benchmark label id per point
    label_ids = read_scannet_semantic("out/semantic", "scene0011_00")

    write_png("out/render/scene0011_00_input_0.png", image[0])                      # uint8 [H, W, 3] of render.render
    write_ply("out/scene0011_00.ply", xyz, rgb)                                     # the coloured points, for a viewer
"""
from __future__ import annotations

import os

import numpy as np

from .postprocess import InstanceTable, SceneLabels

MASK_DIR = "predicted_masks"
SCORE_FORMAT = "%.6f"
_DIGITS = np.array([b"0\n", b"1\n"])


def write_scannet_predictions(out_dir, name, labels, masks=None):
    """Write scene `name`: the kept instances of labels (SceneLabels, host or device) in rank order.  masks None: the
    exclusive masks owner == r (every point in at most one file); masks [p, N] in rank order (the picked masks, e.g.
    SceneLabels.masks of label_batches(keep_masks=True)): the full ones.  Returns the path of the scene's .txt."""
    labels = labels.to_host()
    t = labels.table
    owner = labels.owner
    if masks is not None:
        masks = masks.detach().cpu().numpy() if hasattr(masks, "detach") else np.asarray(masks)
        if masks.shape != (len(t.kept), owner.shape[0]):
            raise ValueError(f"write_scannet_predictions: masks {masks.shape} for {len(t.kept)} ranks over "
                             f"{owner.shape[0]} points")
    os.makedirs(os.path.join(out_dir, MASK_DIR), exist_ok=True)
    lines = []
    for r in np.nonzero(np.asarray(t.kept))[0]:
        rel = f"{MASK_DIR}/{name}_{int(r):03d}.txt"
        m = (owner == r) if masks is None else (masks[r] != 0)
        with open(os.path.join(out_dir, rel), "wb") as f:
            f.write(_DIGITS[m.astype(np.intp)].tobytes())
        lines.append(f"{rel} {int(t.label_id[r])} {SCORE_FORMAT % float(t.score[r])}\n")
    path = os.path.join(out_dir, f"{name}.txt")
    with open(path, "w") as f:
        f.writelines(lines)
    return path


def read_scannet_predictions(out_dir, name):
    """(label_ids int64 [k], scores fp32 [k], masks uint8 [k, N]) of a written scene, in file order."""
    with open(os.path.join(out_dir, f"{name}.txt")) as f:
        rows = [line.rstrip().split() for line in f if line.strip()]
    label_ids = np.array([int(r[1]) for r in rows], dtype=np.int64)
    scores = np.array([float(r[2]) for r in rows], dtype=np.float32)
    masks = []
    for r in rows:
        with open(os.path.join(out_dir, r[0]), "rb") as f:
            raw = np.frombuffer(f.read(), dtype=np.uint8)
        if raw.size % 2 or (raw[1::2] != ord("\n")).any() or ((raw[0::2] != ord("0")) & (raw[0::2] != ord("1"))).any():
            raise ValueError(f"{r[0]}: not one 0 / 1 per line")
        masks.append(raw[0::2] - ord("0"))
    if masks and any(m.shape != masks[0].shape for m in masks):
        raise ValueError(f"{name}: mask files of different lengths")
    return label_ids, scores, (np.stack(masks) if masks else np.zeros((0, 0), np.uint8))


def semantic_benchmark_ids(train_fold):
    """nyu40 id of each class of the semantic head (int64 [13]): wall 1, floor 2, the fold's nine classes their benchmark
    ids, "unannotated" and "candidate" 0 (no benchmark class)."""
    from .evaluation import BENCHMARK_SEMANTIC_LABELS, FOLD_SEMANTIC_LABELS

    fold = FOLD_SEMANTIC_LABELS[int(train_fold)]
    return np.array([BENCHMARK_SEMANTIC_LABELS[0], BENCHMARK_SEMANTIC_LABELS[1], 0, 0]
                    + [BENCHMARK_SEMANTIC_LABELS[c] for c in fold], dtype=np.int64)


def write_scannet_semantic(out_dir, name, preds, train_fold):
    """Write ``<out_dir>/<name>.txt`` of the ScanNet semantic-label benchmark: one nyu40 label id per line for each of
    the scene's points, from the semantic head's classes preds [N] (host or device) by semantic_benchmark_ids.  Returns
    the path."""
    preds = preds.detach().cpu().numpy() if hasattr(preds, "detach") else np.asarray(preds)
    table = semantic_benchmark_ids(train_fold)
    if preds.ndim != 1 or (preds.size and (preds.min() < 0 or preds.max() >= len(table))):
        raise ValueError(f"write_scannet_semantic: classes 0..{len(table) - 1} of [N] points expected")
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, f"{name}.txt")
    np.savetxt(path, table[preds.astype(np.int64)], fmt="%d")
    return path


def read_scannet_semantic(out_dir, name):
    """The label ids int64 [N] of a write_scannet_semantic file."""
    with open(os.path.join(out_dir, f"{name}.txt")) as f:
        return np.array([int(line) for line in f if line.strip()], dtype=np.int64)


def save_labels(path, labels, panoptic=None):
    """One .npz with ids, owner and the instance table (and the masks when the labels carry them); panoptic: the
    scene's panoptic ids [N] (batch_eval.panoptic_batches), stored as `panoptic` only when given."""
    labels = labels.to_host()
    arrays = {"ids": labels.ids, "owner": labels.owner}
    if panoptic is not None:
        arrays["panoptic"] = panoptic.detach().cpu().numpy() if hasattr(panoptic, "detach") else np.asarray(panoptic)
    arrays.update({f"table_{k}": v for k, v in labels.table._asdict().items()})
    if labels.masks is not None:
        arrays["masks"] = labels.masks
    np.savez_compressed(path, **arrays)


def load_labels(path):
    """SceneLabels of a save_labels file."""
    with np.load(path) as z:
        table = InstanceTable(*[z[f"table_{k}"] for k in InstanceTable._fields])
        return SceneLabels(z["owner"], z["ids"], table, z["masks"] if "masks" in z.files else None)


_PNG_MAGIC = b"\x89PNG\r\n\x1a\n"


def _host_array(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def write_png(path, image, level=6):
    """Write image uint8 [H, W, 3] (host or device; render.render's, one view) as an 8-bit RGB PNG: IHDR, one IDAT of
    the rows with filter 0, IEND, written with zlib and struct alone.  Returns the path."""
    import struct
    import zlib

    im = _host_array(image)
    if im.ndim != 3 or im.shape[2] != 3 or im.dtype != np.uint8 or 0 in im.shape:
        raise ValueError(f"write_png: expected uint8 [H, W, 3], got {im.dtype} {im.shape}")
    H, W = im.shape[:2]
    rows = np.zeros((H, 1 + 3 * W), np.uint8)  # a filter byte (0: none) ahead of every row
    rows[:, 1:] = im.reshape(H, 3 * W)

    def chunk(kind, data):
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(_PNG_MAGIC + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0))
                + chunk(b"IDAT", zlib.compress(rows.tobytes(), level)) + chunk(b"IEND", b""))
    return path


def read_png(path):
    """uint8 [H, W, 3] of an 8-bit RGB PNG without interlacing (what write_png writes; all five row filters are
    understood).  Every chunk's CRC is checked."""
    import struct
    import zlib

    with open(path, "rb") as f:
        data = f.read()
    if data[:8] != _PNG_MAGIC:
        raise ValueError(f"{path}: not a PNG file")
    at, head, idat, ended = 8, None, [], False
    while at + 12 <= len(data) and not ended:
        n, kind = struct.unpack(">I4s", data[at:at + 8])
        body = data[at + 8:at + 8 + n]
        if len(body) != n or struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] != zlib.crc32(kind + body) & 0xFFFFFFFF:
            raise ValueError(f"{path}: chunk {kind!r} is truncated or fails its CRC")
        if kind == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat.append(body)
        ended = kind == b"IEND"
        at += 12 + n
    if head is None or not ended:
        raise ValueError(f"{path}: no IHDR or no IEND")
    W, H, depth, colour, _, _, interlace = head
    if (depth, colour, interlace) != (8, 2, 0):
        raise ValueError(f"{path}: only 8-bit RGB without interlacing is read (depth {depth}, colour type {colour})")
    raw = np.frombuffer(zlib.decompress(b"".join(idat)), np.uint8)
    if raw.size != H * (1 + 3 * W):
        raise ValueError(f"{path}: {raw.size} bytes of image data for {W} x {H}")
    raw = raw.reshape(H, 1 + 3 * W)
    if not raw[:, 0].any():
        return raw[:, 1:].reshape(H, W, 3).copy()
    out = np.zeros((H + 1, 3 * W + 3), np.int64)  # a row above and a pixel to the left, zeros
    for y in range(H):
        ft, row, cur, up = int(raw[y, 0]), raw[y, 1:].astype(np.int64), out[y + 1], out[y]
        if ft in (0, 2):
            cur[3:] = (row + (up[3:] if ft == 2 else 0)) & 255
            continue
        if ft not in (1, 3, 4):
            raise ValueError(f"{path}: row filter {ft}")
        for i in range(3 * W):
            a, b, c = cur[i], up[i + 3], up[i]
            if ft == 1:
                pred = a
            elif ft == 3:
                pred = (a + b) >> 1
            else:
                p = a + b - c
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                pred = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
            cur[i + 3] = (row[i] + pred) & 255
    return out[1:, 3:].astype(np.uint8).reshape(H, W, 3)


def write_ply(path, xyz, rgb):
    """Write the points as a binary little-endian PLY vertex cloud (x y z float32, red green blue uchar), for a viewer.
    xyz [N, 3], rgb uint8 [N, 3], host or device.  Returns the path."""
    p = _host_array(xyz).astype("<f4").reshape(-1, 3)
    c = _host_array(rgb)
    if c.dtype != np.uint8 or c.shape != p.shape:
        raise ValueError(f"write_ply: rgb: expected uint8 {p.shape}, got {c.dtype} {c.shape}")
    rec = np.zeros(p.shape[0], dtype=[("xyz", "<f4", 3), ("rgb", "u1", 3)])
    rec["xyz"], rec["rgb"] = p, c
    head = ("ply\nformat binary_little_endian 1.0\n" f"element vertex {p.shape[0]}\n"
            "property float x\nproperty float y\nproperty float z\n"
            "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
    with open(path, "wb") as f:
        f.write(head.encode("ascii") + rec.tobytes())
    return path


def read_ply(path):
    """(xyz float32 [N, 3], rgb uint8 [N, 3]) of a write_ply file."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header\n")
    lines = data[:end].decode("ascii", "replace").split("\n") if end >= 0 else []
    props = [ln.split()[1:] for ln in lines if ln.startswith("property ")]
    want = [["float", "x"], ["float", "y"], ["float", "z"], ["uchar", "red"], ["uchar", "green"], ["uchar", "blue"]]
    count = [int(ln.split()[2]) for ln in lines if ln.startswith("element vertex ")]
    if lines[:2] != ["ply", "format binary_little_endian 1.0"] or props != want or len(count) != 1:
        raise ValueError(f"{path}: not a binary little-endian PLY of x y z red green blue vertices")
    rec = np.frombuffer(data[end + len(b"end_header\n"):], dtype=[("xyz", "<f4", 3), ("rgb", "u1", 3)])
    if rec.shape[0] != count[0]:
        raise ValueError(f"{path}: {rec.shape[0]} vertices in the body, {count[0]} in the header")
    return rec["xyz"].astype(np.float32), rec["rgb"].copy()


def load_scannet_segments(path):
    """The over-segmentation of a ScanNet scene: field ``segIndices`` of ``<scene>_vh_clean_2.0.010000.segs.json`` (what
    data/scannetv2/prepare_data_inst.py:50-57 reads) as int32 [N], one segment id per mesh vertex."""
    import json

    with open(path) as f:
        seg = np.asarray(json.load(f)["segIndices"])
    if seg.ndim != 1 or not (seg.size == 0 or np.issubdtype(seg.dtype, np.integer)):
        raise ValueError(f"{path}: segIndices is not a list of integers")
    seg = seg.astype(np.int64)
    if seg.size and (seg.max() > np.iinfo(np.int32).max or seg.min() < np.iinfo(np.int32).min):
        raise ValueError(f"{path}: segment ids must fit int32")
    return seg.astype(np.int32)


def save_scannet_segments(path, ids):
    """Write an over-segmentation (int [N], one id per point, negative = none; pointops.oversegment's or any other) as
    ``{"segIndices": [...]}``, the field load_scannet_segments reads back unchanged."""
    import json

    seg = ids.detach().cpu().numpy() if hasattr(ids, "detach") else np.asarray(ids)
    if seg.ndim != 1 or not (seg.size == 0 or np.issubdtype(seg.dtype, np.integer)):
        raise ValueError(f"save_scannet_segments: expected an integer array [N], got {seg.dtype} {seg.shape}")
    with open(path, "w") as f:
        json.dump({"segIndices": [int(v) for v in seg]}, f)


BOX_FORMAT = "%.9g"  # float32 extents and their float64 means survive the text to well below a micrometre


def write_boxes(path, boxes, label_ids, scores):
    """One text line per box of a postprocess.Boxes: ``cx cy cz du dv dz yaw label_id score`` -- the centre, the sizes
    along the box's own axes (du along (cos yaw, sin yaw), dv across it, dz along z), the heading in radians about z,
    the label id and the score (SCORE_FORMAT).  label_ids, scores: one per box.  Returns the path."""
    h = lambda a: _host_array(a)  # noqa: E731
    center, size, yaw = (np.asarray(h(a), dtype=np.float64) for a in (boxes.center, boxes.size, boxes.yaw))
    center, size, yaw = center.reshape(-1, 3), size.reshape(-1, 3), yaw.reshape(-1)
    labels = np.asarray(h(label_ids), dtype=np.int64).reshape(-1)
    scores = np.asarray(h(scores), dtype=np.float64).reshape(-1)
    if not (labels.shape[0] == scores.shape[0] == yaw.shape[0] == center.shape[0] == size.shape[0]):
        raise ValueError(f"write_boxes: {center.shape[0]} boxes, {labels.shape[0]} labels, {scores.shape[0]} scores")
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(path, "w") as f:
        for c, s, y, l, sc in zip(center, size, yaw, labels, scores):
            nums = " ".join(BOX_FORMAT % v for v in (*c, *s, y))
            f.write(f"{nums} {int(l)} {SCORE_FORMAT % sc}\n")
    return path

