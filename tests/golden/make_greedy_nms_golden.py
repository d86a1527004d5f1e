"""Generates tests/golden/greedy_nms.npz: the picks of the REFERENCE's util.utils_3d.non_max_suppression_gpu
(util/utils_3d.py:76-93) on CPU tensors.  Run in the build container only (needs the reference tree):

    python tests/golden/make_greedy_nms_golden.py [reference root]

Cases (`names`); per case <name>_scores, <name>_thr (the thresholds) and <name>_pick_<k> (the picks at threshold k):
  mask cases      <name>_bits = np.packbits of the 0/1 masks [n, N], <name>_shape = (n, N).  The [n, n] IoUs are NOT
                  stored: ious_from_masks below is the expression both sides use (fp32 on exact integer counts, so the
                  bits are the same wherever it runs).
                    one      n = 1
                    half     n = 2, I = 1, d = 1 and 2: IoU exactly 0.5; at threshold 0.5 both are kept (strict >)
                    chain3   n = 3 over 64 points, iou(A,B) = iou(B,C) = 0.6, iou(A,C) = 1/3
                    r65 / r200 / r1024   random runs of the points (the generator of tests/test_gpu_batched_eval.py),
                             distinct scores, (n, N) = (65, 700), (200, 3000), (1024, 4096)
  matrix cases    <name>_ious = the explicit fp32 [n, n] matrix
                    chain    A > B > C, iou(A,B) = iou(B,C) = 0.6, iou(A,C) = 0.1 at 0.3: picks [0, 2] (B is dead and
                             suppresses nothing)
                    nonsym   a non-symmetric 3 x 3 matrix (the row index is the pick)
                    empty    n = 0
Every random case must keep at least 2 proposals and fewer than half at every threshold (a kernel that keeps everything,
or only the first, must not pass); asserted here and again in the tests.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
THRESHOLDS = (0.05, 0.3, 0.5)
RANDOM_CASES = (("r65", 65, 700), ("r200", 200, 3000), ("r1024", 1024, 4096))


def ious_from_masks(masks):
    """fp32 IoUs of 0/1 masks [n, N] as test.py:79-83 writes them: I / ((d_i + d_j) - I), d = the diagonal of I."""
    m = torch.as_tensor(masks).float()
    inter = m @ m.t()
    d = torch.diagonal(inter)
    return inter / ((d[:, None] + d[None, :]) - inter)


def run_masks(rng, n, N):
    """n overlapping proposals over N points: random runs (IoUs spread over [0, 1]), every third with a hole."""
    masks = np.zeros((n, N), np.uint8)
    for i in range(n):
        ln = int(rng.integers(N // 50 + 1, N // 4 + 2))
        s = int(rng.integers(0, N - ln + 1))
        masks[i, s:s + ln] = 1
        if i % 3 == 0:
            masks[i, s + ln // 3:s + ln // 3 + ln // 10] = 0
    scores = ((rng.permutation(n) + 1) / (n + 1)).astype(np.float32)
    return masks, scores


def main():
    sys.path.insert(0, REF)
    from util.utils_3d import non_max_suppression_gpu  # the reference's function, on CPU tensors

    out, names = {}, []

    def add(name, scores, thresholds, masks=None, ious=None):
        names.append(name)
        scores = np.asarray(scores, np.float32)
        out[f"{name}_scores"] = scores
        out[f"{name}_thr"] = np.asarray(thresholds, np.float64)
        if masks is not None:
            out[f"{name}_bits"] = np.packbits(masks.astype(np.uint8))
            out[f"{name}_shape"] = np.asarray(masks.shape, np.int64)
            iou_t = ious_from_masks(masks)
        else:
            out[f"{name}_ious"] = np.asarray(ious, np.float32)
            iou_t = torch.from_numpy(out[f"{name}_ious"])
        kept = []
        for k, thr in enumerate(thresholds):
            pick = non_max_suppression_gpu(iou_t, torch.from_numpy(scores), thr) if len(scores) else torch.zeros(0).long()
            out[f"{name}_pick_{k}"] = pick.numpy().astype(np.int64)
            kept.append(int(pick.numel()))
        print(name, "kept", kept, "of", len(scores))
        return kept

    m = np.zeros((1, 64), np.uint8)
    m[0, 5:20] = 1
    add("one", [0.7], THRESHOLDS, masks=m)
    m = np.zeros((2, 64), np.uint8)
    m[0, 0] = 1
    m[1, 0:2] = 1
    assert add("half", [0.9, 0.8], THRESHOLDS, masks=m) == [1, 1, 2]
    m = np.zeros((3, 64), np.uint8)
    m[0, 0:32], m[1, 8:40], m[2, 16:48] = 1, 1, 1
    assert add("chain3", [0.9, 0.8, 0.7], THRESHOLDS, masks=m) == [1, 1, 2]
    rng = np.random.default_rng(3)
    for name, n, N in RANDOM_CASES:
        masks, scores = run_masks(rng, n, N)
        kept = add(name, scores, THRESHOLDS, masks=masks)
        assert all(2 <= k < n / 2 for k in kept), (name, kept)
    chain = [[1.0, 0.6, 0.1], [0.6, 1.0, 0.6], [0.1, 0.6, 1.0]]
    assert add("chain", [0.9, 0.8, 0.7], (0.3,), ious=chain) == [2]
    assert out["chain_pick_0"].tolist() == [0, 2]
    # row 2 (the best score) suppresses 0 but not 1; read by columns it would suppress 1 and not 0
    nonsym = [[1.0, 0.0, 0.1], [0.0, 1.0, 0.9], [0.9, 0.1, 1.0]]
    add("nonsym", [0.5, 0.4, 0.9], (0.5,), ious=nonsym)
    assert out["nonsym_pick_0"].tolist() == [2, 1]
    add("empty", np.zeros(0, np.float32), (0.3,), ious=np.zeros((0, 0), np.float32))
    out["names"] = np.asarray(names)
    path = os.path.join(HERE, "greedy_nms.npz")
    np.savez_compressed(path, **out)
    print("greedy_nms.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
