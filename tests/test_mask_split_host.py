"""Host side of the mask splitting (DBSCAN per picked mask): the statement postprocess.mask_components_host against
sklearn and by literal values, postprocess.split_masks on CPU tensors, the MaskSplit / split= validation of batch_eval,
the command-line flag and the derived binding."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests.mask_split_cases import (HAND_CASES, LATTICE_EPS, LATTICE_K, brute_rows, lattice_cloud, ring_inputs,
                                    sklearn_ids)


@pytest.mark.parametrize("seed", range(40))
def test_statement_is_sklearn_dbscan(seed):
    """Complete symmetric rows (brute force, k = 32 against a maximum degree of 19, no row truncated): the statement
    equals sklearn.cluster.DBSCAN on the mask's points, clusters named by their smallest core index, for every
    min_samples; at min_samples 3 and 5 the case has border points, so their rule is compared too."""
    from geoformer_amd import postprocess

    xyz, member = lattice_cloud(seed)
    I, deg = brute_rows(xyz)
    assert deg.max() < LATTICE_K - 1 and deg.max() <= 18
    masks = member.astype(np.int32)[None]
    for min_samples in (1, 3, 5, 8):
        comp, tab = postprocess.mask_components_host(masks, np.zeros(1, np.int64), I, deg, min_samples, 1)
        assert comp.dtype == np.int32 and tab.dtype == np.int32
        want = sklearn_ids(xyz, member, LATTICE_EPS, min_samples)
        assert comp[0].tolist() == want.tolist()
        ids, size = np.unique(want[want >= 0], return_counts=True)
        assert tab[0, :3].tolist() == [member.sum(), len(ids), size.sum()]
        assert tab[0, 3:].tolist() == ([ids[np.argmax(size)], size.max()] if len(ids) else [-1, 0])
        if min_samples in (3, 5):
            cnt = 1 + (member[np.where(I >= 0, I, 0)] & (I >= 0))[:, 1:].sum(1)
            border = member & (cnt < min_samples) & (want >= 0)
            assert border.sum() > 0


@pytest.mark.parametrize("name", sorted(HAND_CASES))
def test_statement_by_literal_values(name):
    from geoformer_amd import postprocess

    c = HAND_CASES[name]()
    comp, tab = postprocess.mask_components_host(c["masks"], c["pick"], c["I"], c["deg"], c["min_samples"],
                                                 c["min_points"])
    assert comp.tolist() == c["comp"].tolist()
    assert tab.tolist() == c["tab"].tolist()


def test_keep_largest_by_literal_values():
    from geoformer_amd import postprocess

    c = HAND_CASES["picks"]()  # pick = [1, 7, -1, 1, 0]: both rows picked, row 1 twice
    masks = c["masks"] * 3  # (the values of a kept point are the input's)
    out = postprocess.mask_keep_largest_host(masks, c["pick"], c["comp"], c["tab"])
    assert out[0].tolist() == [3] * 100 and out[1].tolist() == [3] * 50 + [0] * 50
    c = HAND_CASES["min_points_edge"]()
    out = postprocess.mask_keep_largest_host(c["masks"], c["pick"], c["comp"], c["tab"])
    assert out.tolist() == [[1, 1, 1, 1, 0, 0, 0, 0, 1, 1, 0]]
    none = postprocess.mask_keep_largest_host(c["masks"], c["pick"], np.full_like(c["comp"], -1),
                                              np.asarray([[11, 0, 0, -1, 0]], np.int32))
    assert not none.any()
    same = postprocess.mask_keep_largest_host(c["masks"], np.zeros(0, np.int64), c["comp"][:0], c["tab"][:0])
    assert same.tolist() == c["masks"].tolist()


def test_statement_arguments():
    from geoformer_amd import postprocess

    masks, pick, I, deg = ring_inputs(10, 2, 0.6)
    for kw in (dict(min_samples=0), dict(min_points=0)):
        with pytest.raises(ValueError):
            postprocess.mask_components_host(masks, pick, I, deg, **kw)
    with pytest.raises(ValueError):
        postprocess.mask_components_host(masks, pick, I[:-1], deg)
    comp, tab = postprocess.mask_components_host(masks, pick[:0], I, deg)
    assert comp.shape == (0, 10) and tab.shape == (0, 5)
    comp, tab = postprocess.mask_components_host(masks[:, :0], pick, I[:0], deg[:0])
    assert comp.shape == (2, 0) and tab.tolist() == [[0, 0, 0, -1, 0]] * 2


def _two_blobs():
    """60 + 55 lattice points in two blobs 1 m apart and 6 stray points; masks: both blobs and the strays / the first blob
    / nothing; 4 proposals of which the NMS picked rows 2, 0 and 3."""
    g = np.stack(np.meshgrid(np.arange(5) * 0.05, np.arange(4) * 0.05, np.arange(3) * 0.05, indexing="ij"), -1).reshape(-1, 3)
    stray = np.c_[np.arange(6) * 0.5, np.full(6, 3.0), np.zeros(6)]
    xyz = np.concatenate([g, g[:55] + [1.0, 0.0, 0.0], stray]).astype(np.float32)
    masks = np.zeros((4, len(xyz)), np.int32)
    masks[0] = 1
    masks[1, 10:40] = 1
    masks[2, :60] = 1
    scores = torch.tensor([0.9, 0.8, 0.7, 0.6])
    cls = torch.tensor([5, 6, 7, 8])
    return torch.from_numpy(xyz), torch.from_numpy(masks), scores, cls, torch.tensor([2, 0, 3])


def test_split_masks_on_cpu_tensors():
    from geoformer_amd import postprocess

    xyz, masks, scores, cls, pick = _two_blobs()
    kw = dict(radius=0.08, k=16, min_samples=1, min_points=10)
    c1, s1, m1, p1 = postprocess.split_masks(masks, scores, cls, pick, xyz, mode="largest", **kw)
    assert c1 is cls and s1 is scores and torch.equal(p1, pick) and m1.dtype == torch.int32 and m1.shape == masks.shape
    assert m1[0].tolist() == [1] * 60 + [0] * 61  # both blobs and the strays: the larger blob
    assert torch.equal(m1[1], masks[1])          # a row the NMS did not pick is left alone
    assert torch.equal(m1[2], masks[2]) and not m1[3].any()
    c2, s2, m2, p2 = postprocess.split_masks(masks, scores, cls, pick, xyz, mode="split", **kw)
    # by pick rank, then cluster id: row 2 (one cluster), row 0 (clusters 0 and 60), row 3 (none)
    assert m2.dtype == torch.int32 and m2.shape == (3, 121) and p2.tolist() == [0, 1, 2] and p2.dtype == torch.int64
    assert c2.tolist() == [7, 5, 5] and s2.tolist() == scores[[2, 0, 0]].tolist()
    assert m2[0].tolist() == masks[2].tolist()
    assert m2[1].tolist() == [1] * 60 + [0] * 61 and m2[2].tolist() == [0] * 60 + [1] * 55 + [0] * 6
    parents = [2, 0, 0]
    for row, parent in zip(m2, parents):  # a subset of its parent; rows of one parent are disjoint
        assert not (row & ~masks[parent]).any()
    assert not (m2[1] & m2[2]).any()
    # min_points = 1: every stray point is a cluster of its own
    _, _, m3, p3 = postprocess.split_masks(masks, scores, cls, pick, xyz, mode="split", **dict(kw, min_points=1))
    assert m3.shape[0] == 1 + 8 and m3[3:].sum(1).tolist() == [1] * 6 and p3.tolist() == list(range(9))
    # nothing kept at all
    c4, s4, m4, p4 = postprocess.split_masks(masks, scores, cls, pick, xyz, mode="split", **dict(kw, min_points=500))
    assert m4.shape == (0, 121) and c4.shape == s4.shape == p4.shape == (0,)
    # a scene without proposals passes through
    empty = torch.zeros(0, dtype=torch.int64)
    for mode in ("largest", "split"):
        assert postprocess.split_masks([], [], [], empty, xyz, mode=mode) == ([], [], [], empty)
    with pytest.raises(ValueError):
        postprocess.split_masks(masks, scores, cls, pick, xyz, mode="biggest")


def test_dbscan_on_a_cpu_tensor():
    from geoformer_amd import pointops

    xyz, member = lattice_cloud(3)
    x = xyz[member]
    for min_samples in (1, 4):
        got, flag = pointops.dbscan(torch.from_numpy(x), LATTICE_EPS, min_samples=min_samples, return_flag=True)
        assert flag is None and got.dtype == torch.int32
        assert got.tolist() == sklearn_ids(x, np.ones(len(x), bool), LATTICE_EPS, min_samples).tolist()
    assert pointops.dbscan(torch.zeros((0, 3)), 0.1).shape == (0,)
    with pytest.raises(RuntimeError):
        pointops.dbscan(torch.from_numpy(x), 0.1, min_samples=0)


def test_mask_split_validation():
    from geoformer_amd import batch_eval, postprocess

    assert batch_eval.MaskSplit().params == postprocess.SPLIT_DEFAULTS
    assert postprocess.SPLIT_DEFAULTS == dict(radius=0.1, k=16, min_samples=1, min_points=50, mode="largest")
    ms = batch_eval.MaskSplit(radius=0.08, mode="split")
    assert ms.params["radius"] == 0.08 and ms.params["mode"] == "split" and ms.params["min_points"] == 50
    assert "radius=0.08" in repr(ms)
    with pytest.raises(TypeError):
        batch_eval.MaskSplit(radius=0.1, eps=0.25)
    with pytest.raises(ValueError):
        batch_eval.MaskSplit(mode="biggest")
    assert batch_eval._mask_split(None) is None and batch_eval._mask_split(ms) is ms
    assert batch_eval._mask_split("largest").params["mode"] == "largest"
    assert batch_eval._mask_split("split").params["mode"] == "split"
    for bad in ("biggest", 3, True):
        with pytest.raises(ValueError):
            batch_eval._mask_split(bad)
    # predict_batches refuses a bad value before it touches the model
    with pytest.raises(ValueError):
        next(batch_eval.predict_batches(None, [], 1, split="biggest"))
    # the splitter of a scene is split_masks with the parameters
    xyz, masks, scores, cls, pick = _two_blobs()
    got = batch_eval.MaskSplit(radius=0.08, min_points=10).of_scene(cls, scores, masks, pick, xyz)
    want = postprocess.split_masks(masks, scores, cls, pick, xyz, radius=0.08, min_points=10)
    assert torch.equal(got[2], want[2]) and got[0] is cls and got[1] is scores


def test_command_line_flag():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "predict_scenes.py")
    spec = importlib.util.spec_from_file_location("predict_scenes_cli", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ap = mod.build_parser()
    assert ap.parse_args(["--synthetic", "1"]).split_masks is None
    assert ap.parse_args(["--synthetic", "1", "--split-masks", "largest"]).split_masks == "largest"
    assert ap.parse_args(["--split-masks", "split", "a.npy"]).split_masks == "split"
    with pytest.raises(SystemExit):
        ap.parse_args(["--split-masks", "biggest"])


def test_binding_is_derived_from_the_header():
    from ctypes import c_int, c_size_t, c_void_p

    from geoformer_amd import _abi

    fns = _abi.functions()
    assert fns["gf_mask_components_scratch_bytes"] == (c_size_t, [c_int, c_int])
    assert fns["gf_mask_components"] == (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int,
                                                 c_int, c_void_p, c_void_p, c_void_p, c_void_p])
    assert fns["gf_mask_keep_largest"] == (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                                   c_void_p])
    assert _abi.const("GF_MSP_TABLE_INTS") == 5  # an enumerator: the parser reads those with a written value too
    assert _abi.const("GF_ERR_INVALID_ARG") == -1
    assert _abi.parse("enum { GF_A = 3, GF_B = 0x10, GF_C };\n", "probe.h").consts == {"GF_A": 3, "GF_B": 16}
