"""The cases of tests/golden/greedy_nms.npz (tests/golden/make_greedy_nms_golden.py: picks of the reference's
non_max_suppression_gpu), loaded once and shared by the host and GPU tests."""
import functools
import os
from typing import NamedTuple

import numpy as np
import torch

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RANDOM = ("r65", "r200", "r1024")


class Case(NamedTuple):
    name: str
    masks: object  # uint8 [n, N] or None (a matrix case)
    ious: object  # fp32 torch [n, n]
    scores: object  # fp32 torch [n]
    thresholds: tuple
    picks: tuple  # one int64 list per threshold


def ious_from_masks(masks):
    """The generator's expression: fp32 I / ((d_i + d_j) - I) on exact integer counts."""
    m = torch.as_tensor(masks).float()
    inter = m @ m.t()
    d = torch.diagonal(inter)
    return inter / ((d[:, None] + d[None, :]) - inter)


@functools.lru_cache(maxsize=None)
def cases():
    z = np.load(os.path.join(G, "greedy_nms.npz"))
    out = {}
    for name in [str(x) for x in z["names"]]:
        scores = torch.from_numpy(z[f"{name}_scores"])
        thr = tuple(float(t) for t in z[f"{name}_thr"])
        picks = tuple(z[f"{name}_pick_{k}"].tolist() for k in range(len(thr)))
        if f"{name}_bits" in z.files:
            n, N = (int(v) for v in z[f"{name}_shape"])
            masks = np.unpackbits(z[f"{name}_bits"])[:n * N].reshape(n, N)
            ious = ious_from_masks(masks)
        else:
            masks, ious = None, torch.from_numpy(z[f"{name}_ious"])
        out[name] = Case(name, masks, ious, scores, thr, picks)
    for name in RANDOM:  # neither "keep everything" nor "keep the first" may pass
        n = out[name].scores.shape[0]
        assert all(2 <= len(p) < n / 2 for p in out[name].picks), name
    return out


def case_ids():
    return ["one", "half", "chain3", "r65", "r200", "r1024", "chain", "nonsym", "empty"]
