"""Host side of the over-segment pooling of the eval forward: the host statement (postprocess.segment_pool_host), the
input helpers (scene.grid_segments, export.load_scannet_segments), the "segments" key of batch_eval's host batches and
the CPU branch of GeoFormer.generate_proposal.  No GPU."""
import json

import numpy as np
import pytest
import torch


def test_host_statement_by_literal_values():
    from geoformer_amd import postprocess

    # seven foreground points: segment 5 = {0, 3, 4}, segment 9 = {1, 6}, a point without a segment (2), a singleton (5)
    seg = np.array([5, 9, -1, 5, 5, 2_000_000_000, 9], np.int64)
    x = np.array([[1.0, 2.0, 3.0, 2.0, 6.0, -4.5, 4.0],
                  [0.5, -1.0, 7.0, 0.5, 0.5, 0.1, -3.0],
                  [-8.0, 0.0, -0.0, 4.0, 1.0, 1e-30, 1.0]], np.float32)
    want = np.array([[3.0, 3.0, 3.0, 3.0, 3.0, -4.5, 3.0],
                     [0.5, -2.0, 7.0, 0.5, 0.5, 0.1, -2.0],
                     [-1.0, 0.5, -0.0, -1.0, -1.0, 1e-30, 0.5]], np.float32)
    got = postprocess.segment_pool_host(x, seg)
    assert got.dtype == np.float32 and got.shape == (3, 7)
    assert got.tobytes() == want.tobytes()  # (bit for bit: -0.0 of the point without a segment, 1e-30 of the singleton)
    assert postprocess.segment_pool_host(torch.from_numpy(x), torch.from_numpy(seg).int()).tobytes() == want.tobytes()
    # ids are compared inside one scene only: the id 5 of a second scene is another segment
    other = postprocess.segment_pool_host(np.array([[10.0, 20.0]], np.float32), np.array([5, 5]))
    assert other.tolist() == [[15.0, 15.0]] and got[0, 0] == 3.0
    with pytest.raises(ValueError):
        postprocess.segment_pool_host(x, seg[:6])
    with pytest.raises(ValueError):
        postprocess.segment_pool_host(x, seg.astype(np.float32))
    assert postprocess.segment_pool_host(np.zeros((2, 0), np.float32), np.zeros(0, np.int32)).shape == (2, 0)


def test_grid_segments():
    from geoformer_amd import scene

    raw = scene.make_raw_scene(9000, 41, n_boxes=2, room=(1.6, 1.6, 0.6))
    seg = scene.grid_segments(raw)
    assert seg.dtype == np.int32 and seg.shape == (raw.shape[0],)
    lab, inst = raw[:, 6].astype(np.int64), raw[:, 7].astype(np.int64)
    assert (lab < 0).any() and np.array_equal(seg < 0, lab < 0) and (seg[lab < 0] == -1).all()
    ids = np.unique(seg[seg >= 0])
    assert np.array_equal(ids, np.arange(ids.size)) and ids.size > 10  # dense from 0
    for s in ids:
        m = seg == s
        assert np.unique(lab[m]).size == 1 and np.unique(inst[m]).size == 1
        cells = np.floor(raw[m, :3] / 0.25)
        assert (cells == cells[0]).all()
    assert np.array_equal(seg, scene.grid_segments(raw.copy()))  # deterministic
    fine = scene.grid_segments(raw, cell=0.1)
    assert fine.max() > seg.max()  # smaller cells, more segments
    assert np.array_equal(scene.grid_segments(raw[:0]), np.zeros(0, np.int32))


def test_load_scannet_segments_round_trip(tmp_path):
    from geoformer_amd import export

    seg = np.array([7, 7, 12, 0, 2147483647, 12, 3], np.int64)
    path = tmp_path / "scene0000_00_vh_clean_2.0.010000.segs.json"
    path.write_text(json.dumps({"params": {"kThresh": "0.0001"}, "sceneId": "scene0000_00", "segIndices": seg.tolist()}))
    got = export.load_scannet_segments(str(path))
    assert got.dtype == np.int32 and np.array_equal(got, seg)
    path.write_text(json.dumps({"segIndices": [1, 2 ** 31]}))
    with pytest.raises(ValueError):
        export.load_scannet_segments(str(path))
    path.write_text(json.dumps({"segIndices": [0.5, 1.0]}))
    with pytest.raises(ValueError):
        export.load_scannet_segments(str(path))


def test_collate_batches_segments_key():
    from geoformer_amd import batch_eval, scene

    items = [(f"s{i}", scene.make_raw_scene(700 + 100 * i, 60 + i, n_boxes=1, room=(1.6, 1.6, 0.6))) for i in range(3)]
    segs = {"s0": scene.grid_segments(items[0][1]), "s2": np.arange(items[2][1].shape[0], dtype=np.int64)[::-1].copy()}
    _, plain = batch_eval.collate_batches(items, 2)
    chunks, got = batch_eval.collate_batches(items, 2, segments=segs)
    assert [len(c) for c in chunks] == [2, 1]
    for p, g in zip(plain, got):
        assert set(g) == set(p) | {"segments"} and "segments" not in p
        assert g["segments"].dtype == torch.int32 and g["segments"].shape == (int(g["offsets"][-1]),)
        for k in p:
            assert np.array_equal(np.asarray(p[k]), np.asarray(g[k])), k
    n0 = items[0][1].shape[0]
    assert np.array_equal(got[0]["segments"][:n0].numpy(), segs["s0"])
    assert (got[0]["segments"][n0:] == -1).all()  # s1 is not in the mapping
    assert np.array_equal(got[1]["segments"].numpy(), segs["s2"])
    # exactly today's keys without the argument
    assert set(plain[0]) == {"locs", "locs_float", "feats", "labels", "instance_labels", "offsets", "spatial_shape",
                             "pc_mins", "pc_maxs"}
    big = np.zeros(n0, np.int64)
    big[3] = 2 ** 31
    with pytest.raises(ValueError):
        batch_eval.collate_batches(items, 2, segments={"s0": big})
    big[3] = 2 ** 31 - 1
    batch_eval.collate_batches(items, 2, segments={"s0": big})
    with pytest.raises(ValueError):
        batch_eval.collate_batches(items, 2, segments={"s0": big[:-1]})
    with pytest.raises(ValueError):
        batch_eval.collate_batches(items, 2, segments={"s0": big.astype(np.float32)})


def _proposal_case():
    """Synthetic logits of 3 queries over 400 foreground points of a 1000-point scene.  Query 0 is positive on segments
    0..3; on segment 4 (100 points) its mean is negative while 30 members are positive: pooled, the segment leaves the
    mask, unpooled those 30 points are in."""
    rng = np.random.default_rng(5)
    n_fg, N, ncls = 400, 1000, 13
    fg = np.sort(rng.choice(N, n_fg, replace=False))
    seg_fg = np.repeat(np.arange(5), [60, 70, 80, 90, 100])[rng.permutation(n_fg)]
    x = rng.normal(-6.0, 0.5, (3, n_fg))
    x[0, seg_fg < 4] = rng.normal(4.0, 0.5, int((seg_fg < 4).sum()))
    four = np.nonzero(seg_fg == 4)[0]
    x[0, four[:30]] = 2.0
    x[0, four[30:]] = -3.0
    x[1, seg_fg == 1] = 3.0
    segments = np.full(N, -1, np.int32)
    segments[fg] = seg_fg
    segments[np.setdiff1d(np.arange(N), fg)[:50]] = 4  # the part of a segment outside the foreground plays no role
    cls = rng.normal(0, 1, (3, ncls))
    cls[:, 6] += 8.0
    sem = torch.softmax(torch.tensor(rng.normal(0, 1, (n_fg, ncls)), dtype=torch.float32), 1)
    return (torch.tensor(x, dtype=torch.float32), torch.tensor(cls, dtype=torch.float32)[None], torch.from_numpy(fg),
            torch.from_numpy(segments), torch.from_numpy(seg_fg.astype(np.int32)), sem, N, n_fg)


def test_generate_proposal_cpu_pools_with_the_host_statement():
    from geoformer_amd import postprocess
    from geoformer_amd.model import GeoFormer, load_config

    m = GeoFormer(load_config("test_geoformer_scannet.yaml"))
    x, cls, fg, segments, seg_fg, sem, N, n_fg = _proposal_case()
    kw = dict(sem_prob=sem, score_thresh=0.5, npoint_thresh=50)
    offs, offs_ = torch.tensor([0, N]), torch.tensor([0, n_fg])
    with torch.no_grad():
        got = m.generate_proposal([x], cls, fg, offs, offs_, segments=segments, **kw)
        pooled = torch.from_numpy(postprocess.segment_pool_host(x, seg_fg))
        want = m.generate_proposal([pooled], cls, fg, offs, offs_, **kw)
        raw = m.generate_proposal([x], cls, fg, offs, offs_, **kw)
        with pytest.raises(TypeError):
            m.generate_proposal([x], cls, fg, offs, offs_, segments=segments.long(), **kw)
    assert torch.is_tensor(got[0]) and got[0].shape[0] >= 1
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and torch.equal(g, w)
    # the case is built so that pooling matters: segment 4 leaves query 0's mask as a whole
    four = fg[seg_fg == 4]
    assert raw[2].shape == got[2].shape and not torch.equal(raw[2], got[2])
    assert int(raw[2][0, four].sum()) == 30 and int(got[2][0, four].sum()) == 0
    assert not torch.equal(raw[1], got[1])
    # every returned mask is constant over each segment's foreground points
    for s in range(5):
        col = got[2][:, fg[seg_fg == s]]
        assert ((col.sum(1) == 0) | (col.sum(1) == col.shape[1])).all()
    # with grad enabled (training) the key is ignored
    with_grad = m.generate_proposal([x], cls, fg, offs, offs_, segments=segments, **kw)
    assert all(torch.equal(a, b) for a, b in zip(with_grad, raw))
