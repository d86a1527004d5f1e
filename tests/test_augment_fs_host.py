"""CPU: the few-shot episode's numpy restatement (tests/augment_fs_numpy.py), the class tables of FSIndex.build and the
host choice sampler against the reference's own trainMergeFS and table builders (tests/golden/train_merge_fs.npz,
make_train_merge_fs_golden.py)."""
import os
import random

import numpy as np
import pytest
import torch

from tests import augment_fs_numpy as afn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_merge_fs.npz")


def fs_golden():
    """{"scenes": {name: raw [N,8]}, "c2s", "c2i", "counts", "cases": {name: case}}; a case holds its seed, batch,
    max_npoint, the generators' final states, "infos", "support" / "query" dicts (reference dtypes restored, key order
    in "support_keys" / "query_keys")."""
    z = np.load(GOLDEN)
    raw = np.concatenate([z["raw_xyzrgb"], z["raw_labinst"]], 1).astype(np.float64)
    off = np.concatenate([[0], np.cumsum(z["sizes"])])
    names = [str(n) for n in z["names"]]
    scenes = {n: raw[off[i]:off[i + 1]] for i, n in enumerate(names)}
    g = {"scenes": scenes, "counts": {n: int(c) for n, c in zip(names, z["counts"])},
         "c2s": {c: [str(s) for s in z[f"c2s_{c}"]] for c in range(20)},
         "c2i": {c: [[str(s), i] for s, i in zip(z[f"c2i_{c}_scene"], z[f"c2i_{c}_id"])] for c in range(20)},
         "cases": {}}
    for name in ("crop", "episode"):
        p = name + "/"
        c = {k[len(p):]: z[k] for k in z.files if k.startswith(p) and "/" not in k[len(p):]}
        c["infos"] = [{"sampled_class": int(k), "query_scene": str(q), "support_scene": str(s),
                       "support_instance_id": i}
                      for k, q, s, i in zip(c.pop("info_class"), c.pop("info_query"), c.pop("info_support"),
                                            c.pop("info_id"))]
        for part in ("support", "query"):
            q = p + part + "/"
            d = {k[len(q):]: z[k] for k in z.files if k.startswith(q)}
            for k in [k for k in d if k.startswith("dtype_")]:
                if k[6:] in d:
                    d[k[6:]] = d[k[6:]].astype(str(d[k]))
            if part == "support":  # the support scenes' raw rows (not stored twice)
                rows = np.concatenate([scenes[i["support_scene"]] for i in c["infos"]])
                d["feats"] = rows[:, 3:6].astype(str(d["dtype_feats"]))
                d["locs_float"] = rows[:, :3].astype(str(d["dtype_locs_float"]))
            c[part] = {k: v for k, v in d.items() if not k.startswith("dtype_")}
            c[part + "_dtypes"] = {k[6:]: str(v) for k, v in d.items() if k.startswith("dtype_")}
            c[part + "_keys"] = [str(k) for k in c[part + "_keys"]]
        g["cases"][name] = c
    return g


def seed_all(seed):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)


def states_match(c):
    """The three generators are where the reference left them (torch: untouched)."""
    rs = random.getstate()
    st = np.random.get_state()
    return (list(rs[1]) == c["random_state"].tolist() and rs[2] is None and (st[1] == c["np_state_key"]).all()
            and st[2] == int(c["np_state_pos"]) and st[3] == c["np_state_gauss"][0] and st[4] == c["np_state_gauss"][1]
            and (torch.get_rng_state().numpy() == c["torch_state"]).all())


@pytest.mark.parametrize("name", ["crop", "episode"])
def test_restatement_matches_reference_trainmergefs(name):
    g = fs_golden()
    c = g["cases"][name]
    seed_all(int(c["seed"]))
    sup, q, infos, used = afn.train_merge_fs_numpy(g["scenes"], g["c2s"], g["c2i"], g["counts"], int(c["batch"]),
                                                   max_npoint=int(c["max_npoint"]))
    assert infos == c["infos"]
    assert set(sup) == set(c["support_keys"]) and set(q) == set(c["query_keys"])
    assert not afn.compare(sup, c["support"]), afn.compare(sup, c["support"])
    assert not afn.compare(q, c["query"]), afn.compare(q, c["query"])
    assert states_match(c)
    if name == "crop":
        assert min(used["chosen"]) >= 1  # every query took several crop iterations
        off = c["query"]["batch_offsets"]
        assert any(c["query"]["labels"][off[i]:off[i + 1]].sum() == 0 for i in range(int(c["batch"])))
        assert (c["query"]["instance_pointnum"].size
                == sum(len(np.unique(c["query"]["instance_labels"][off[i]:off[i + 1]][
                    c["query"]["instance_labels"][off[i]:off[i + 1]] >= 0])) for i in range(int(c["batch"]))))
    else:
        qs = [i["query_scene"] for i in infos]
        assert len(set(qs)) < len(qs)  # a scene drawn twice


def test_golden_covers_the_support_retry():
    """The episode case drew a listed support scene with <= 100 nonzero labels and drew again: replaying its random
    state, some support draw lands on such a scene."""
    g = fs_golden()
    c = g["cases"]["episode"]
    small = {s for v in g["c2i"].values() for s, _ in v if g["counts"][s] <= 100}
    assert small
    random.seed(int(c["seed"]))
    hits = 0
    for _ in range(int(c["batch"])):
        cls = random.choice((2, 3, 4, 7, 9, 11, 12, 13, 18))
        random.choice(g["c2s"][cls])
        while True:
            s, _ = random.choice(g["c2i"][cls])
            if g["counts"][s] > 100:
                break
            hits += s in small
    assert hits >= 1


def test_fsindex_build_reproduces_reference_tables():
    from geoformer_amd import augment

    g = fs_golden()
    idx = augment.FSIndex.build(g["scenes"])
    for c in range(20):
        assert set(idx.class2scans[c]) == set(g["c2s"][c]), c  # (the reference lists them in glob order)
        assert [(s, int(i)) for s, i in idx.class2instances[c]] == [(s, int(i)) for s, i in g["c2i"][c]], c
    assert idx.counts == g["counts"]
    c2s, c2i, counts = afn.tables(g["scenes"])
    assert all(set(c2s[c]) == set(g["c2s"][c]) and [(s, int(i)) for s, i in c2i[c]] == [(s, int(i)) for s, i in
                                                                                           g["c2i"][c]]
               for c in range(20)) and counts == g["counts"]
    # device tensors on the CPU are accepted as well
    idx2 = augment.FSIndex.build({k: torch.from_numpy(v) for k, v in g["scenes"].items()})
    assert idx2.class2instances == idx.class2instances and idx2.counts == idx.counts


@pytest.mark.parametrize("name", ["crop", "episode"])
def test_host_sampler_consumes_random_like_the_reference(name):
    from geoformer_amd import augment

    g = fs_golden()
    c = g["cases"][name]
    idx = augment.FSIndex.from_tables(g["c2s"], g["c2i"], g["counts"])
    random.seed(int(c["seed"]))
    infos = augment.sample_episode(idx, int(c["batch"]), 0, "reference")
    assert infos == c["infos"]
    assert list(random.getstate()[1]) == c["random_state"].tolist()


def test_device_sampler_is_keyed_and_leaves_random_alone():
    from geoformer_amd import augment

    g = fs_golden()
    idx = augment.FSIndex.from_tables(g["c2s"], g["c2i"], g["counts"])
    random.seed(3)
    before = random.getstate()
    a = augment.sample_episode(idx, 8, 0, "device", seed=11, batch_index=2)
    assert a == augment.sample_episode(idx, 8, 0, "device", seed=11, batch_index=2)
    assert a != augment.sample_episode(idx, 8, 0, "device", seed=11, batch_index=3)
    assert random.getstate() == before
    for inf in a:
        assert inf["query_scene"] in idx.class2scans[inf["sampled_class"]]
        assert [inf["support_scene"], inf["support_instance_id"]] in idx.class2instances[inf["sampled_class"]]
        assert idx.counts[inf["support_scene"]] > augment.SUPPORT_MIN_LABELLED
    # the choices spread over the whole range
    hits = np.bincount([augment.choice_index(9, 5, b, 0, 0) for b in range(900)], minlength=9)
    assert hits.min() > 60, hits


def test_sampler_refuses_a_class_without_support():
    from geoformer_amd import augment

    g = fs_golden()
    c2i = {c: [t for t in v if g["counts"][t[0]] <= 100] if c == 2 else v for c, v in g["c2i"].items()}
    idx = augment.FSIndex.from_tables(g["c2s"], c2i, g["counts"])
    with pytest.raises(ValueError, match="support"):
        for b in range(50):
            augment.sample_episode(idx, 8, 0, "device", seed=1, batch_index=b)
