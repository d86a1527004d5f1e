"""GPU: training-batch augmentation and collate (geoformer_amd/augment.py, csrc/augment.hip) against the reference's own
trainMerge (tests/golden/train_merge.npz) and the numpy restatement (tests/augment_numpy.py)."""
import numpy as np
import pytest
import torch

from tests import augment_numpy as an
from tests.test_augment_host import golden_case


def _host(b):
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in b.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["crop", "plain"])
def test_reference_mode_matches_reference_trainmerge(hip, name):
    from geoformer_amd import augment

    c = golden_case(name)
    np.random.seed(int(c["numpy_seed"]))
    torch.manual_seed(int(c["torch_seed"]))
    b, draws = augment.train_merge(c["scenes"], max_npoint=int(c["max_npoint"]), cvfold=int(c["cvfold"]),
                                   rng="reference", device="cuda", return_draws=True)
    for k in ("locs", "voxel_locs", "p2v_map", "v2p_map", "labels", "instance_labels", "instance_pointnum", "offsets",
              "feats", "locs_float", "instance_infos", "pc_mins", "pc_maxs"):
        assert b[k].is_cuda and b[k].dtype == torch.from_numpy(c[k]).dtype, (k, b[k].dtype, c[k].dtype)
    assert not an.compare(_host(b), c), an.compare(_host(b), c)
    st = np.random.get_state()
    assert (st[1] == c["np_state_key"]).all() and st[2] == int(c["np_state_pos"])
    assert st[3] == c["np_state_gauss"][0] and st[4] == c["np_state_gauss"][1]
    assert (torch.get_rng_state().numpy() == c["torch_state"]).all()
    i = 0
    for s in range(len(c["scenes"])):
        for p in range(2):
            for a in range(3):
                ref, got = c[f"blurred_{i}"], draws["blurred"][s][p][a]
                assert got.shape == ref.shape and np.abs(got - ref).max() <= 1e-6 * np.abs(ref).max()
                i += 1


def _scenes():
    from geoformer_amd import scene

    # (the scene without instances in the middle: the deviation, 0 instances, is part of every comparison)
    return [scene.make_raw_scene(6000, 301), scene.make_raw_scene(3000, 303, instances=False),
            scene.make_raw_scene(4500, 302)]


@pytest.mark.gpu
def test_device_mode_is_deterministic(hip):
    from geoformer_amd import augment

    sc = _scenes()
    a = _host(augment.train_merge(sc, rng="device", seed=11, batch_index=3, device="cuda"))
    b = _host(augment.train_merge([torch.from_numpy(x).cuda() for x in sc], rng="device", seed=11, batch_index=3,
                                  device="cuda"))
    c = _host(augment.train_merge(sc, rng="device", seed=11, batch_index=4, device="cuda"))
    for k in an.INT_KEYS + an.FLOAT_KEYS:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    assert not np.array_equal(a["locs_float"][:100], c["locs_float"][:100])


@pytest.mark.gpu
@pytest.mark.parametrize("max_npoint,cvfold", [(250000, 0), (3000, 1)])
def test_device_mode_matches_restatement_on_its_draws(hip, max_npoint, cvfold):
    from geoformer_amd import augment

    sc = _scenes()
    b, draws = augment.train_merge(sc, rng="device", seed=5, batch_index=1, max_npoint=max_npoint, cvfold=cvfold,
                                   device="cuda", return_draws=True)
    want, _, diag = an.train_merge_numpy(sc, draws, max_npoint=max_npoint, cvfold=cvfold)
    got = _host(b)
    assert not an.compare(got, want), an.compare(got, want)
    for s in range(len(sc)):
        for p in range(2):
            assert tuple(draws["bb"][s][p]) == tuple(diag["bb"][s][p])
            for a in range(3):
                ref = diag["blurred"][s][p][a]
                assert np.abs(draws["blurred"][s][p][a] - ref).max() <= 1e-6 * np.abs(ref).max()
    if max_npoint < 250000:
        # the first candidate that fits is taken, and every kept coordinate lies inside its full_scale
        off = got["offsets"]
        for s, ch in enumerate(draws["chosen"]):
            n = off[s + 1] - off[s]
            assert n <= max_npoint and (ch >= 0) == (sc[s].shape[0] > max_npoint)
            if ch < 0:
                continue
            fs = np.array([512 - 32 * ch, 512 - 32 * ch, 512])
            loc = got["locs"][off[s]:off[s + 1], 1:]
            assert (loc >= 0).all() and (loc < fs).all()


@pytest.mark.gpu
def test_philox_normals_moments(hip):
    from geoformer_amd import augment, scene

    sc = [scene.make_raw_scene(20000, 401 + i) for i in range(4)]
    vals = []
    bi = 0
    while sum(v.size for v in vals) < 1_000_000:
        _, d = augment.train_merge(sc, rng="device", seed=99, batch_index=bi, device="cuda", return_draws=True)
        vals += [g.ravel().astype(np.float64) for sd in d["noise"] for pas in sd for g in pas]
        bi += 1
    x = np.concatenate(vals)
    n = x.size
    assert abs(x.mean()) < 5 / np.sqrt(n), x.mean()
    assert abs(x.var() - 1.0) < 5 * np.sqrt(2.0 / n), x.var()
    assert np.abs(x).max() < augment.NORMAL_MAX


@pytest.mark.gpu
def test_train_feeder_yields_train_merge_batches(hip):
    from geoformer_amd import augment

    sc = _scenes() + _scenes()[::-1]
    dev_sc = [torch.from_numpy(x).cuda() for x in sc]
    for src in (sc, dev_sc):
        got = [_host(b) for b in augment.TrainFeeder(src, batch_size=2, seed=21, device="cuda", reserve_points=20000)]
        assert len(got) == 3
        for i, g in enumerate(got):
            want = _host(augment.train_merge(sc[2 * i:2 * i + 2], rng="device", seed=21, batch_index=i, device="cuda"))
            for k in an.INT_KEYS + an.FLOAT_KEYS:
                assert np.array_equal(np.asarray(g[k]), np.asarray(want[k])), (i, k)
            assert g["id"] == [2 * i, 2 * i + 1]


@pytest.mark.gpu
def test_training_step_on_augmented_batches(hip, oracle):
    from geoformer_amd import augment
    from tests.test_training_step import _setup, _step

    cfg, m, crit, _ = _setup("cuda")
    c = golden_case("crop")
    golden = {k: c[k] for k in ("locs", "voxel_locs", "p2v_map", "v2p_map", "locs_float", "feats", "labels",
                                 "instance_labels", "instance_pointnum", "instance_infos", "offsets", "pc_mins",
                                 "pc_maxs")}
    golden = {k: torch.from_numpy(v).cuda() for k, v in golden.items()}
    golden["spatial_shape"], golden["id"] = c["spatial_shape"], [0, 1]
    loss_golden, _, _ = _step(m, crit, golden, 1)
    np.random.seed(int(c["numpy_seed"]))
    torch.manual_seed(int(c["torch_seed"]))
    b = augment.train_merge(c["scenes"], max_npoint=int(c["max_npoint"]), rng="reference", device="cuda")
    loss_ours, _, _ = _step(m, crit, b, 1)
    assert np.isfinite(loss_golden) and abs(loss_ours - loss_golden) <= 1e-5 * max(1.0, abs(loss_golden))
    from geoformer_amd import scene

    src = [scene.make_raw_scene(2500, 501), scene.make_raw_scene(2000, 502)]
    fb = next(iter(augment.TrainFeeder(src, batch_size=2, seed=3, device="cuda")))
    loss, _, norms = _step(m, crit, fb, 1)
    assert np.isfinite(loss) and norms and all(np.isfinite(v) for v in norms.values())
