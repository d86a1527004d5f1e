"""Generates tests/golden/matrix_nms_sizes.npz: the picks of the REFERENCE's util.utils_3d.matrix_non_max_suppression
(util/utils_3d.py:95-141) on CPU tensors, for the matrix NMS cases of tests/proposal_cases.py.  Run where the reference
tree is at hand:

    python tests/golden/make_matrix_nms_golden.py <reference root>

Cases (`names`): the hand-built cases with distinct scores (one, pair, chain3, chain3x, dup3) and the 3-class random runs
r16 ... r1024 (tests/proposal_cases.py::golden_case_ids).  Per case:
    <name>_bits  = np.packbits of the 0/1 masks [n, N], <name>_shape = (n, N), <name>_scores fp32, <name>_cats int64,
and per kernel k in (gaussian, linear):
    <name>_<k>_thr    the case's sweep thresholds (float64, tests/proposal_cases.py::nms_sweep: midpoints of the usable
                      gaps between the float64 decayed scores, and 0.05 / 0.5 where usable),
    <name>_<k>_count  how many proposals the reference kept at each threshold,
    <name>_<k>_picks  the kept indices of all thresholds one after the other (int32, rank order).
Data only: nothing of the reference's program text is stored.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import proposal_cases as pc  # noqa: E402


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    sys.path.insert(0, sys.argv[1])
    from util.utils_3d import matrix_non_max_suppression  # the reference's function, on CPU tensors

    out, names = {}, pc.golden_case_ids()
    for name in names:
        c = pc.nms_cases()[name]
        out[f"{name}_bits"] = np.packbits(c.masks)
        out[f"{name}_shape"] = np.asarray(c.masks.shape, np.int64)
        out[f"{name}_scores"] = c.scores
        out[f"{name}_cats"] = c.cats
        masks, scores, cats = torch.from_numpy(c.masks.astype(np.int32)), torch.from_numpy(c.scores), torch.from_numpy(c.cats)
        for kernel in pc.KERNELS:
            thr, _ = pc.nms_sweep(name, kernel)
            picks = [matrix_non_max_suppression(masks, scores, cats, kernel=kernel, sigma=pc.SIGMA,
                                                final_score_thresh=t).numpy() for t in thr]
            out[f"{name}_{kernel}_thr"] = np.asarray(thr, np.float64)
            out[f"{name}_{kernel}_count"] = np.asarray([len(p) for p in picks], np.int32)
            out[f"{name}_{kernel}_picks"] = np.concatenate(picks).astype(np.int32) if picks else np.zeros(0, np.int32)
            print(name, kernel, "kept", [len(p) for p in picks], "of", c.n)
    out["names"] = np.asarray(names)
    path = os.path.join(HERE, "matrix_nms_sizes.npz")
    np.savez_compressed(path, **out)
    print("matrix_nms_sizes.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
