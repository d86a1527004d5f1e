"""frames.FuserHost and frames.concat without a GPU: the statement of the streaming map against frames.fuse_host of the
concatenated frames (every field as bits), its numbering, its failures and its limits."""
import numpy as np
import pytest
import torch

from geoformer_amd import frames, postprocess
from tests import frames_cases as fc
from tests import frames_stream_cases as sc

INPUTS = {"u16": dict(kind="u16", stride=1, edge=None), "f32": dict(kind="f32", stride=2, edge=0.05)}


def _stream(fr, sizes, cell, stride, edge, origin=None):
    fz = frames.FuserHost(cell, stride, edge=edge, origin=origin)
    cells = [fz.add(c) for c in sc.chunks(fr, sizes)]
    return fz, torch.cat(cells)


@pytest.mark.parametrize("color", [True, False])
@pytest.mark.parametrize("split", sorted(sc.SPLITS))
@pytest.mark.parametrize("inp", sorted(INPUTS))
def test_chunks_equal_the_concatenation(inp, split, color):
    a = INPUTS[inp]
    fr = sc.dense4(a["kind"], color)
    kept = {}
    for cell, min_obs in ((0.02, 1), (sc.COARSE, 1), (sc.COARSE, 3)):
        fz, cells = _stream(fr, sc.SPLITS[split], cell, a["stride"], a["edge"])
        want = frames.fuse_host(frames.concat(sc.chunks(fr, sc.SPLITS[split])), cell, a["stride"], edge=a["edge"],
                                min_obs=min_obs, origin=fz.origin)
        got = fz.snapshot(min_obs, cells)
        assert sc.same_fused(got, want)
        assert got.xyz.shape[0] > 100 and (got.count >= min_obs).all()
        assert fz.pixels == int((cells >= 0).sum()) and fz.cells == int(cells.max()) + 1
        kept[cell, min_obs] = got.xyz.shape[0]
    assert kept[sc.COARSE, 3] < kept[sc.COARSE, 1] < kept[0.02, 1]  # min_obs = 3 drops cells, and keeps some
    if inp == "u16":
        assert abs(kept[0.02, 1] - sc.DENSE4_CELLS) < 20 and fz.pixels == sc.DENSE4_PIXELS  # (the origin moves a few)


def test_explicit_origin_and_the_default_one():
    fr = sc.dense4()
    first = frames.backproject_host(sc.sub(fr, 0, 1))[0]
    fz = frames.FuserHost()
    assert fz.origin is None
    fz.add(sc.sub(fr, 0, 1))
    o = fz.origin
    assert o.dtype == np.float32 and (o == first.min(0) - np.float32(64.0)).all()
    fz.add(sc.sub(fr, 1, 4))
    assert (fz.origin == o).all()  # fixed afterwards
    assert (frames.FuserHost(margin=1.5).add(sc.sub(fr, 0, 1)) >= -1).all()
    g = frames.FuserHost(margin=1.5)
    g.add(sc.sub(fr, 0, 1))
    assert (g.origin == first.min(0) - np.float32(1.5)).all()
    # an explicit origin is the grid's corner from the start, and fuse_host agrees with it
    lo = frames.backproject_host(fr)[0].min(0) - np.float32(0.25)
    fz, cells = _stream(fr, (2, 2), 0.02, 1, None, origin=lo)
    assert (fz.origin == lo).all()
    assert sc.same_fused(fz.snapshot(1, cells), frames.fuse_host(fr, 0.02, origin=lo))


def test_the_same_chunk_twice():
    fr = sc.sub(sc.dense4(), 0, 2)
    fz = frames.FuserHost(sc.COARSE)
    c1 = fz.add(fr)
    M, one = fz.cells, fz.snapshot()
    c2 = fz.add(fr)
    assert fz.cells == M and (c1 == c2).all()  # no new cell
    two = fz.snapshot(1, torch.cat([c1, c2]))
    assert (two.count == 2 * one.count).all() and (two.xyz.view(torch.int32) == one.xyz.view(torch.int32)).all()
    assert (two.rgb == one.rgb).all()
    assert sc.same_fused(two, frames.fuse_host(frames.concat([fr, fr]), sc.COARSE, origin=fz.origin))


def test_a_chunk_without_a_valid_pixel():
    fr = sc.gaps3()
    fz = frames.FuserHost()
    cells = [fz.add(sc.sub(fr, 0, 1))]
    M, before = fz.cells, fz.state()
    cells.append(fz.add(sc.sub(fr, 1, 2)))
    assert fz.cells == M and (cells[1] == -1).all() and cells[1].shape == cells[0].shape
    assert all((x == y).all() for x, y in zip(before, fz.state()))
    cells.append(fz.add(sc.sub(fr, 2, 3)))
    assert (cells[2] >= 0).all()  # the last frame keeps every pixel
    assert sc.same_fused(fz.snapshot(1, torch.cat(cells)), frames.fuse_host(fr, origin=fz.origin))
    # a first add with no valid pixel leaves the origin unset
    fz = frames.FuserHost()
    assert (fz.add(sc.sub(fr, 1, 2)) == -1).all() and fz.origin is None and fz.cells == 0 and fz.pixels == 0
    e = fz.snapshot(1, torch.full((1, 3, 4), -1, dtype=torch.int32))
    assert e.xyz.shape == (0, 3) and e.point_of.shape == (1, 3, 4) and (e.point_of == -1).all()
    fz.add(sc.sub(fr, 0, 1))
    assert fz.origin is not None


def test_one_cell_holds_every_pixel():
    fr = sc.dense4()
    fz, cells = _stream(fr, (1, 3), sc.ONE_CELL, 1, None)
    s = fz.snapshot(1, cells)
    assert fz.cells == 1 and s.count.tolist() == [sc.DENSE4_PIXELS] and int(cells.max()) == 0
    assert sc.same_fused(s, frames.fuse_host(fr, sc.ONE_CELL, origin=fz.origin))


def test_snapshot_changes_nothing():
    fr = sc.dense4()
    fz = frames.FuserHost(sc.COARSE)
    c1 = fz.add(sc.sub(fr, 0, 2))
    st = fz.state()
    a3, a1, b3 = fz.snapshot(3, c1), fz.snapshot(1, c1), fz.snapshot(3, c1)
    assert sc.same_fused(a3, b3) and a3.xyz.shape[0] < a1.xyz.shape[0]
    assert all((x == y).all() for x, y in zip(st, fz.state()))
    c2 = fz.add(sc.sub(fr, 2, 4))
    fz.snapshot(2)
    assert sc.same_fused(fz.snapshot(3, torch.cat([c1, c2])), frames.fuse_host(fr, sc.COARSE, min_obs=3, origin=fz.origin))
    none = fz.snapshot(10 ** 6, c1)  # above every count: an empty Fused
    assert none.xyz.shape == (0, 3) and none.count.shape == (0,) and (none.point_of == -1).all()
    assert fz.snapshot().point_of.shape == (0, 0, 0)


def test_numbers_never_change():
    fr = sc.dense4()
    parts = sc.chunks(fr, (1, 1, 1, 1))
    fz = frames.FuserHost()
    c0 = fz.add(parts[0])
    keys0, count0, _ = fz.state()
    # the key of a cell, recomputed from its pixels' points
    xyz, _, pixel_of, _, _ = frames.backproject_host(parts[0])
    with np.errstate(all="ignore"):
        c = np.floor((xyz - fz.origin) / np.float32(0.02)).astype(np.int64)
    key = c[:, 0] | c[:, 1] << 21 | c[:, 2] << 42
    mine = c0.reshape(-1)[pixel_of].numpy()
    assert (keys0[mine] == key).all()
    assert (np.diff(mine[np.sort(np.unique(mine, return_index=True)[1])]) == 1).all()  # numbered by first occurrence
    for p in parts[1:]:
        fz.add(p)
    keys, count, _ = fz.state()
    assert (keys[: keys0.shape[0]] == keys0).all() and (keys[mine] == key).all()
    assert (count[: count0.shape[0]] >= count0).all() and (count[: count0.shape[0]] > count0).any()
    assert np.unique(keys).shape[0] == keys.shape[0]


def _failures():
    fr = sc.dense4()
    lo = frames.backproject_host(fr)[0].min(0)
    return fr, lo


@pytest.mark.parametrize("trigger", ["below", "beyond", "size", "dtype", "colour", "shift"])
def test_a_failed_add_leaves_the_map_as_it_was(trigger):
    fr, lo = _failures()
    good = sc.chunks(fr, (2, 1, 1))
    origin = lo - np.float32(1.0)
    fz = frames.FuserHost(origin=origin)
    cells = [fz.add(good[0])]
    before, snap = fz.state(), fz.snapshot(1, cells[0])
    if trigger == "below":
        bad = sc.moved(good[1], (-50.0, 0.0, 0.0))
    elif trigger == "beyond":
        bad = sc.moved(good[1], (0.0, sc.REACH, 0.0))
    elif trigger == "size":
        bad = frames.make(np.ones((1, 4, 4), np.uint16), [5.0, 5.0, 2.0, 2.0], np.eye(4)[None], np.zeros((1, 4, 4, 3), np.uint8))
    elif trigger == "dtype":
        bad = sc.sub(sc.dense4("f32"), 2, 3)
    elif trigger == "colour":
        bad = sc.sub(sc.dense4("u16", False), 2, 3)
    else:
        bad = good[1]._replace(depth_shift=500.0)
    with pytest.raises(ValueError, match="origin=" if trigger in ("below", "beyond") else "differs"):
        fz.add(bad)
    assert all((x == y).all() for x, y in zip(before, fz.state())) and (fz.origin == origin).all()
    assert sc.same_fused(fz.snapshot(1, cells[0]), snap)
    cells += [fz.add(good[1]), fz.add(good[2])]
    assert sc.same_fused(fz.snapshot(1, torch.cat(cells)), frames.fuse_host(fr, origin=origin))


def test_beyond_reach_at_the_edge():
    # a point at 4096 m from the origin on one axis fails, the float below it passes; both lie inside the grid at 1 cm
    below = np.nextafter(np.float32(sc.REACH), np.float32(0))
    fz = frames.FuserHost(0.01, origin=(0, 0, 0))
    assert fz.add_points(np.array([[below, 1, 1]], np.float32)).tolist() == [0]
    with pytest.raises(ValueError, match="4096 m or more"):
        fz.add_points(np.array([[1, 1, 1], [sc.REACH, 1, 1]], np.float32))
    assert fz.cells == 1 and fz.pixels == 1
    with pytest.raises(ValueError, match="outside the grid"):
        fz.add_points(np.array([[1, -0.5, 1]], np.float32))
    assert fz.add_points(np.array([[1, 1, 1]], np.float32)).tolist() == [1]


def test_pixel_budget(monkeypatch):
    fr = sc.dense4()
    n = [int((frames.backproject_host(sc.sub(fr, k, k + 1))[3] >= 0).sum()) for k in range(2)]
    monkeypatch.setattr(frames, "STREAM_MAX_PIXELS", n[0] + n[1] - 1)
    fz = frames.FuserHost()
    c0 = fz.add(sc.sub(fr, 0, 1))
    before, snap = fz.state(), fz.snapshot(1, c0)
    with pytest.raises(ValueError, match="at most"):
        fz.add(sc.sub(fr, 1, 2))
    assert fz.pixels == n[0] and all((x == y).all() for x, y in zip(before, fz.state()))
    assert sc.same_fused(fz.snapshot(1, c0), snap)
    monkeypatch.setattr(frames, "STREAM_MAX_PIXELS", n[0] + n[1])
    fz.add(sc.sub(fr, 1, 2))
    assert fz.pixels == n[0] + n[1]
    assert frames.STREAM_MAX_PIXELS * (int(sc.REACH) << 20) < 2 ** 63  # why the sums cannot overflow


def test_add_points_is_the_grid_and_the_means():
    xyz, rgb = fc.random_points()
    fz = frames.FuserHost(0.02, origin=(0, 0, 0))
    half = xyz.shape[0] // 2
    cells = torch.cat([fz.add_points(xyz[:half], rgb[:half]), fz.add_points(xyz[half:], rgb[half:])]).numpy()
    o = np.zeros(3, np.float32)
    _, cell_of, count = postprocess.grid_subsample_host(xyz, 0.02, "first", o)
    assert (cells == cell_of).all()
    want = frames.cell_means_host(xyz, rgb, cell_of, count, o)
    got = fz.snapshot()
    assert (got.xyz.numpy().view(np.int32) == want[0].view(np.int32)).all() and (got.rgb.numpy() == want[1]).all()
    assert (got.count.numpy() == want[2]).all()
    with pytest.raises(ValueError):
        fz.add_points(xyz.astype(np.float64))
    with pytest.raises(ValueError):
        fz.add_points(np.array([[np.nan, 0, 0]], np.float32))


def test_concat():
    fr = sc.dense4()
    parts = sc.chunks(fr, (1, 2, 1))
    back = frames.concat(parts)
    assert (back.depth == fr.depth).all() and (back.color == fr.color).all() and (back.table == fr.table).all()
    assert back.depth_shift == fr.depth_shift and back.table.dtype == np.float32 and back.depth.is_contiguous()
    assert frames.concat([sc.dense4("u16", False)]).color is None
    small = frames.make(np.ones((1, 4, 4), np.uint16), [5.0, 5.0, 2.0, 2.0], np.eye(4)[None])
    for other in (sc.dense4("f32"), sc.dense4("u16", False), small, fr._replace(depth_shift=1.0)):
        with pytest.raises(ValueError, match="differs"):
            frames.concat([fr, other])
    for bad in ([], [fr, "x"], [None]):
        with pytest.raises(ValueError):
            frames.concat(bad)


def test_arguments_and_the_cpu_fuser():
    for kw in (dict(cell=0), dict(stride=0), dict(edge=-1), dict(origin=(0, 0)), dict(origin=(0, np.inf, 0)), dict(margin=-1),
               dict(margin=np.nan)):
        with pytest.raises(ValueError):
            frames.FuserHost(**kw)
    fr = sc.dense4()
    fz = frames.FuserHost()
    c = fz.add(sc.sub(fr, 0, 1))
    for bad in (c.long(), torch.full((2,), fz.cells, dtype=torch.int32), torch.tensor([0, -2], dtype=torch.int32)):
        with pytest.raises(ValueError):
            fz.snapshot(1, bad)
    with pytest.raises(ValueError):
        fz.snapshot(0)
    with pytest.raises(ValueError):
        fz.add("frames")
    # device "cpu" is the statement
    fu = frames.Fuser(sc.COARSE, device="cpu")
    cells = torch.cat([fu.add(p) for p in sc.chunks(fr, (2, 2))])
    assert sc.same_fused(fu.snapshot(3, cells), frames.fuse_host(fr, sc.COARSE, min_obs=3, origin=fu.origin))
    assert fu.cells > 0 and fu.pixels == sc.DENSE4_PIXELS and fu.slots is None
    assert frames.stream_slots(0, 4800) == (1024, 16384) and frames.stream_slots(2500, 0) == (16384, 8192)
    assert frames.stream_slots(0, 0) == (64, 64)
