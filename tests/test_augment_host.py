"""CPU: the numpy restatement of trainMerge (tests/augment_numpy.py), which the GPU tests use as their yardstick, against
the reference's own trainMerge (tests/golden/train_merge.npz, make_train_merge_golden.py)."""
import os

import numpy as np
import pytest
import torch

from tests import augment_numpy as an

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_merge.npz")


def golden_case(name):
    z = np.load(GOLDEN)
    p = name + "/"
    c = {k[len(p):]: z[k] for k in z.files if k.startswith(p)}
    for k in [k for k in c if k.startswith("dtype_")]:  # (stored compactly: the reference's dtypes restored)
        c[k[6:]] = c[k[6:]].astype(str(c.pop(k)))
    c["raw"] = np.concatenate([c.pop("raw_xyzrgb"), c.pop("raw_labinst")], 1).astype(np.float64)
    off = np.concatenate([[0], np.cumsum(c["sizes"])])
    c["scenes"] = [c["raw"][off[i]:off[i + 1]] for i in range(len(c["sizes"]))]
    return c


@pytest.mark.parametrize("name", ["crop", "plain"])
def test_restatement_matches_reference_trainmerge(name):
    c = golden_case(name)
    np.random.seed(int(c["numpy_seed"]))
    torch.manual_seed(int(c["torch_seed"]))
    b, used, diag = an.train_merge_numpy(c["scenes"], None, max_npoint=int(c["max_npoint"]), cvfold=int(c["cvfold"]))
    assert not an.compare(b, c), an.compare(b, c)
    # both generators end where the reference left them
    st = np.random.get_state()
    assert (st[1] == c["np_state_key"]).all() and st[2] == int(c["np_state_pos"])
    assert st[3] == c["np_state_gauss"][0] and st[4] == c["np_state_gauss"][1]
    assert (torch.get_rng_state().numpy() == c["torch_state"]).all()
    # the blurred grids (recorded around the reference's elastic)
    i = 0
    for s in range(len(c["scenes"])):
        for p in range(2):
            for a in range(3):
                ref = c[f"blurred_{i}"]
                got = diag["blurred"][s][p][a]
                assert got.shape == ref.shape
                assert np.abs(got - ref).max() <= 1e-6 * max(np.abs(ref).max(), 1e-30)
                i += 1
    if name == "crop":
        assert any(ch >= 1 for ch in used["chosen"]), used["chosen"]  # a scene took several crop iterations


def test_restatement_replays_its_draws():
    c = golden_case("crop")
    np.random.seed(int(c["numpy_seed"]))
    torch.manual_seed(int(c["torch_seed"]))
    b, used, _ = an.train_merge_numpy(c["scenes"], None, max_npoint=int(c["max_npoint"]))
    b2, _, _ = an.train_merge_numpy(c["scenes"], used, max_npoint=int(c["max_npoint"]))
    assert not an.compare(b2, b, tol=0.0)


@pytest.mark.parametrize("seed", range(40))
def test_cropped_inst_label_closed_form(seed):
    """getCroppedInstLabel's mapping on id sets with holes: the closed form the kernel uses == the reference's loop."""
    rng = np.random.default_rng(seed)
    n_ids = int(rng.integers(1, 30))
    ids = np.sort(rng.choice(int(rng.integers(n_ids, 4 * n_ids + 2)), n_ids, replace=False))
    pts = np.concatenate([rng.choice(ids, 200), np.full(int(rng.integers(0, 20)), -100)])
    rng.shuffle(pts)
    want = an.cropped_inst_label_loop(pts)
    m = an.cropped_inst_map(ids)
    got = np.array([m[int(v)] if v >= 0 else -100 for v in pts])
    assert (got == want).all()
    assert sorted(set(m.values())) == list(range(n_ids))


def test_raw_scene_covers_the_remap():
    from geoformer_amd import augment, scene

    r = scene.make_raw_scene(30_000, 5)
    lab, ins = r[:, 6].astype(int), r[:, 7].astype(int)
    assert r.dtype == np.float64 and r.shape[1] == 8
    assert {0, 1, -100} <= set(lab)
    assert set(lab) & set(augment.FOLD[0]) and set(lab) & set(augment.FOLD[1])
    ids = np.unique(ins[ins >= 0])
    assert ids.size >= 2 and ids.max() + 1 > ids.size  # ids with holes
    assert (scene.make_raw_scene(5_000, 6, instances=False)[:, 7] == -100).all()


def test_instance_free_scene_counts_zero():
    """The deviation: a scene without instances adds 0 (the reference: int(max) + 1 = -99) to the running total."""
    from geoformer_amd import scene

    scenes = [scene.make_raw_scene(3000, 61, instances=False), scene.make_raw_scene(3000, 62)]
    np.random.seed(0)
    torch.manual_seed(0)
    b, _, _ = an.train_merge_numpy(scenes, None, voxelise=False)
    second = b["instance_labels"][b["offsets"][1]:]
    assert (b["instance_labels"][:b["offsets"][1]] == -100).all()
    assert second[second >= 0].min() == 0
    assert b["instance_pointnum"].size == second[second >= 0].max() + 1
