"""Host side of the geometric over-segmentation: the statement (postprocess.oversegment_host and its two stages) by
literal values on hand-made inputs, the segs.json round trip, and collate_batches(segments="geometric") on host
batches."""
import numpy as np
import pytest
import torch

from tests.oversegment_cases import RULE_CASES


@pytest.mark.parametrize("name", sorted(RULE_CASES))
def test_rule_by_literal_values(name):
    from geoformer_amd import postprocess

    xyz, n4, I, deg, kw, want = RULE_CASES[name]()
    got, ambiguous = postprocess.smooth_components_host(xyz, n4, I, deg, margins=(1e-4, 1e-5), **kw)
    assert got.dtype == np.int32 and got.tolist() == want.tolist()
    assert ambiguous == 0  # no case sits on a threshold
    # the decision counted as ambiguous when the margin reaches its threshold
    _, wide = postprocess.smooth_components_host(xyz, n4, I, deg, margins=(1.0, 1.0), **kw)
    assert wide > 0


def test_plane_end_to_end():
    """One tilted 6 x 6 lattice through all four stages: the normal by the sign rule, sigma = 0, one segment with id 0;
    the rows the function builds itself are the ones it is given."""
    from geoformer_amd import postprocess

    u, v = [a.reshape(-1) for a in np.meshgrid(np.arange(6) * 0.02, np.arange(6) * 0.02, indexing="ij")]
    e1, e2 = np.array([0.6, 0.0, 0.8]), np.array([0.0, 1.0, 0.0])  # the plane's normal: +-(0.8, 0, -0.6)
    xyz = (u[:, None] * e1 + v[:, None] * e2).astype(np.float32)
    I, deg = postprocess.knn_radius_host(xyz, 16, 0.05)
    assert (I[:, 0] == np.arange(36)).all() and deg.min() >= 5 and deg.max() <= 15
    d2 = ((xyz[I[7, :deg[7] + 1]] - xyz[7]) ** 2).sum(1)
    assert (np.diff(d2) >= -1e-9).all() and np.sqrt(d2.max()) <= 0.05 + 1e-6
    n4 = postprocess.point_normals_host(xyz, I, deg)
    assert np.allclose(n4[:, :3], [0.8, 0.0, -0.6], atol=1e-5) and (n4[:, 3] >= 0).all() and (n4[:, 3] < 1e-9).all()
    ids = postprocess.oversegment_host(xyz, I, deg, radius=0.05)
    assert ids.dtype == np.int32 and (ids == 0).all()
    assert (postprocess.oversegment_host(xyz, k=16, radius=0.05) == 0).all()
    # a normal whose first component vanishes: the second decides the sign
    n4y = postprocess.point_normals_host(xyz[:, [1, 0, 2]].copy(), I, deg)
    assert np.allclose(n4y[:, :3], [0.0, 0.8, -0.6], atol=1e-5)


def test_degenerate_points_get_no_segment():
    """Five copies of one point (covariance 0: sigma = -1), a pair (deg < 2: invalid) and one point alone."""
    from geoformer_amd import postprocess

    xyz = np.array([[0.0, 0.0, 0.0]] * 5 + [[1.0, 0.0, 0.0], [1.01, 0.0, 0.0], [3.0, 3.0, 3.0]], np.float32)
    I, deg = postprocess.knn_radius_host(xyz, 8, 0.05)
    assert deg.tolist() == [4] * 5 + [1, 1, 0]
    n4 = postprocess.point_normals_host(xyz, I, deg)
    assert (n4[:, 3] == -1).all() and not n4[:, :3].any()
    assert (postprocess.oversegment_host(xyz, I, deg, min_points=1) == -1).all()


def test_empty_and_single():
    from geoformer_amd import pointops, postprocess

    for n in (0, 1):
        xyz = np.zeros((n, 3), np.float32)
        ids, amb = postprocess.oversegment_host(xyz, return_ambiguous=True)
        assert ids.dtype == np.int32 and ids.tolist() == [-1] * n and amb == 0
        got = pointops.oversegment(torch.from_numpy(xyz))  # a CPU tensor runs the host statement
        assert got.dtype == torch.int32 and got.tolist() == [-1] * n
    with pytest.raises(ValueError):
        postprocess.smooth_components_host(np.zeros((1, 3)), np.zeros((1, 4)), np.zeros((1, 1), np.int32),
                                           np.zeros(1, np.int32), min_points=0)


def test_generated_room():
    """The rule on a generated room: a dozen segments (walls, ceiling, the floor around the box, the box's faces), few
    points without one -- and nothing like the two segments the rule gives without its flatness gate."""
    from geoformer_amd import postprocess, scene

    sc = scene.make_small_scene(8192, seed=7)
    xyz, sp = sc["xyz"].astype(np.float32), sc["spacing"]
    I, deg = postprocess.knn_radius_host(xyz, 16, 3 * sp)
    ids = postprocess.oversegment_host(xyz, I, deg, radius=3 * sp, offset=0.5 * sp)
    kept, size = np.unique(ids[ids >= 0], return_counts=True)
    assert 8 <= len(kept) <= 16 and size.min() >= 8 and (ids < 0).mean() < 0.05
    assert (ids[kept] == kept).all()  # an id is a member of its own segment (its smallest flat point)
    open_gate = postprocess.oversegment_host(xyz, I, deg, radius=3 * sp, offset=0.5 * sp, flatness=1.0)
    assert len(np.unique(open_gate[open_gate >= 0])) <= 3


def test_scannet_segments_round_trip(tmp_path):
    from geoformer_amd import export

    ids = np.array([5, -1, 0, 2 ** 31 - 1, -7, 5, 3], np.int32)
    path = tmp_path / "scene0000_00_vh_clean_2.0.010000.segs.json"
    export.save_scannet_segments(path, ids)
    got = export.load_scannet_segments(path)
    assert got.dtype == np.int32 and got.tolist() == ids.tolist()
    export.save_scannet_segments(path, torch.from_numpy(ids[:0]))
    assert export.load_scannet_segments(path).shape == (0,)
    with pytest.raises(ValueError):
        export.save_scannet_segments(path, ids.astype(np.float32))


def test_collate_batches_geometric():
    from geoformer_amd import batch_eval, postprocess, scene

    items = [(f"s{i}", scene.make_raw_scene(1500, 40 + i, n_boxes=1, room=(1.2, 1.0, 0.5))) for i in range(3)]
    plain = batch_eval.collate_batches(items, 2)[1]
    params = dict(radius=0.12, offset=0.02)
    for seg_arg, kw in (("geometric", {}), (batch_eval.GeometricSegments(**params), params)):
        chunks, batches = batch_eval.collate_batches(items, 2, segments=seg_arg)
        assert [len(c) for c in chunks] == [2, 1]
        for b, p in zip(batches, plain):
            seg, off = b["segments"], b["offsets"].tolist()
            assert seg.dtype == torch.int32 and seg.shape == (off[-1],)
            assert set(b) - {"segments"} == set(p) and torch.equal(b["locs"], p["locs"])
            for s in range(len(off) - 1):  # scene-local ids of the scene's own points
                want = postprocess.oversegment_host(b["locs_float"][off[s]:off[s + 1]], **kw)
                assert seg[off[s]:off[s + 1]].tolist() == want.tolist()
    assert (batches[0]["segments"] >= 0).any()
    # a mapping gives what it gave before
    n0, n1, n2 = (r.shape[0] for _, r in items)
    segs = {"s0": np.arange(n0) % 7, "s2": -np.ones(n2, np.int64)}
    by_name = batch_eval.collate_batches(items, 2, segments=segs)[1]
    assert by_name[0]["segments"].tolist() == (np.arange(n0) % 7).tolist() + [-1] * n1
    assert by_name[1]["segments"].tolist() == [-1] * n2 and by_name[0]["segments"].dtype == torch.int32
    assert all("segments" not in b for b in plain)
    with pytest.raises(ValueError):
        batch_eval.collate_batches(items, 2, segments="geometry")
    with pytest.raises(TypeError):
        batch_eval.GeometricSegments(radius=0.1, cell=0.25)
