"""GPU: few-shot training episodes (geoformer_amd/augment.py train_merge_fs / FSTrainFeeder, csrc/augment.hip) against
the reference's own trainMergeFS (tests/golden/train_merge_fs.npz) and the numpy restatement
(tests/augment_fs_numpy.py)."""
import numpy as np
import pytest
import torch

from tests import augment_fs_numpy as afn
from tests.test_augment_fs_host import fs_golden, seed_all, states_match


def _host(b):
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in b.items()}


def _index(g):
    from geoformer_amd import augment

    return augment.FSIndex.from_tables(g["c2s"], g["c2i"], g["counts"])


def _same(a, b):
    for k in set(a) | set(b):
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["crop", "episode"])
def test_reference_mode_matches_reference_trainmergefs(hip, name):
    from geoformer_amd import augment

    g = fs_golden()
    c = g["cases"][name]
    seed_all(int(c["seed"]))
    sup, q, infos = augment.train_merge_fs(g["scenes"], _index(g), int(c["batch"]), rng="reference",
                                           max_npoint=int(c["max_npoint"]), device="cuda")
    assert infos == c["infos"]
    for part, got in (("support", sup), ("query", q)):
        assert list(got) == c[part + "_keys"], (part, list(got))
        for k, v in got.items():
            if torch.is_tensor(v):
                assert v.is_cuda and str(v.dtype).replace("torch.", "") == c[part + "_dtypes"][k], (part, k, v.dtype)
            else:
                assert str(v.dtype) == c[part + "_dtypes"][k], (part, k)
        bad = afn.compare(_host(got), c[part])
        assert not bad, (part, bad)
    assert states_match(c)


@pytest.mark.gpu
def test_device_mode_is_deterministic(hip):
    from geoformer_amd import augment

    g = fs_golden()
    idx = _index(g)
    res = [augment.train_merge_fs(g["scenes"], idx, 4, rng="device", seed=9, batch_index=2, device="cuda")]
    resident = {k: torch.from_numpy(v).cuda() for k, v in g["scenes"].items()}
    res.append(augment.train_merge_fs(resident, idx, 4, rng="device", seed=9, batch_index=2, device="cuda"))
    other = augment.train_merge_fs(g["scenes"], idx, 4, rng="device", seed=9, batch_index=3, device="cuda")
    assert res[0][2] == res[1][2]
    for part in (0, 1):
        _same(_host(res[0][part]), _host(res[1][part]))
    a, b = _host(res[0][1]), _host(other[1])
    assert res[0][2] != other[2] or not np.array_equal(a["locs_float"][:50], b["locs_float"][:50])


@pytest.mark.gpu
@pytest.mark.parametrize("max_npoint", [250000, 500])
def test_device_mode_matches_restatement_on_its_draws(hip, max_npoint):
    from geoformer_amd import augment

    g = fs_golden()
    sup, q, infos, draws = augment.train_merge_fs(g["scenes"], _index(g), 5, rng="device", seed=4, batch_index=1,
                                                  max_npoint=max_npoint, device="cuda", return_draws=True)
    ws, wq, _, _ = afn.train_merge_fs_numpy(g["scenes"], None, None, None, 5, infos=infos, draws=draws,
                                            max_npoint=max_npoint)
    assert not afn.compare(_host(sup), ws), afn.compare(_host(sup), ws)
    assert not afn.compare(_host(q), wq), afn.compare(_host(q), wq)
    if max_npoint < 250000:
        assert max(draws["chosen"]) >= 0


@pytest.mark.gpu
def test_episode_invariants(hip):
    from geoformer_amd import augment

    g = fs_golden()
    for bi in range(3):
        sup, q, infos = augment.train_merge_fs(g["scenes"], _index(g), 6, rng="device", seed=17, batch_index=bi,
                                               max_npoint=600, device="cuda")
        q, sup = _host(q), _host(sup)
        assert set(np.unique(q["labels"])) <= {0, 1}
        assert (q["instance_labels"][q["labels"] == 0] == -100).all()
        pn, o = [], q["batch_offsets"]
        for s, inf in enumerate(infos):
            il = q["instance_labels"][o[s]:o[s + 1]]
            ids = np.unique(il[il >= 0])
            assert (ids == np.arange(ids.size)).all()  # scene-local ids 0..n-1
            pn += [int((il == i).sum()) for i in ids]
            so = sup["batch_offsets"]
            raw = g["scenes"][inf["support_scene"]]
            assert so[s + 1] - so[s] == raw.shape[0]
            assert sup["support_masks"][so[s]:so[s + 1]].sum() == (raw[:, 7] == inf["support_instance_id"]).sum() > 0
        assert q["instance_pointnum"].tolist() == pn
        assert (sup["locs"][:, 0] == np.repeat(np.arange(6), np.diff(sup["batch_offsets"]))).all()


@pytest.mark.gpu
def test_feeder_yields_train_merge_fs_episodes(hip):
    from geoformer_amd import augment

    g = fs_golden()
    idx = _index(g)
    resident = {k: torch.from_numpy(v).cuda() for k, v in g["scenes"].items()}
    for src in (g["scenes"], resident):
        got = list(augment.FSTrainFeeder(src, idx, batch_size=3, seed=23, device="cuda", episodes=3, max_npoint=700))
        assert len(got) == 3
        for i, (sup, q, infos) in enumerate(got):
            ws, wq, winf = augment.train_merge_fs(g["scenes"], idx, 3, rng="device", seed=23, batch_index=i,
                                                  max_npoint=700, device="cuda")
            assert infos == winf and list(q) == list(wq) and list(sup) == list(ws)
            _same(_host(q), _host(wq))
            _same(_host(sup), _host(ws))


@pytest.mark.gpu
def test_fs_training_step_fed_by_the_feeder(hip):
    from geoformer_amd import augment
    from tests.test_training_step import _fs_setup, _fs_step

    cfg, m, crit, _, _ = _fs_setup("cuda")  # geoformer_fs_scannet.yaml, batch 2, frozen backbone
    g = fs_golden()
    feeder = augment.FSTrainFeeder({k: torch.from_numpy(v).cuda() for k, v in g["scenes"].items()}, _index(g),
                                   batch_size=2, seed=31, device="cuda", episodes=2)
    trainable = {n for n, p in m.named_parameters() if p.requires_grad}
    assert sum(p.numel() for n, p in m.named_parameters() if n in trainable) == 42706
    for sup, q, _ in feeder:
        loss, info, norms = _fs_step(m, crit, sup, q)
        assert np.isfinite(loss) and {"focal_loss", "dice_loss", "loss"} <= set(info)
        assert norms and set(norms) <= trainable and all(np.isfinite(v) for v in norms.values())
