"""geoformer_amd.frames without a GPU: the numpy statements of csrc/frames.hip against plain float64 restatements, the
conventions against render.py's by a round trip, and the argument checks."""
import numpy as np
import pytest
import torch

from geoformer_amd import frames, postprocess
from tests import frames_cases as fc

U = 2.0 ** -24  # half an ulp of a float32 result, relative to it


def _f64_points(fr, stride, pixel_of):
    """(xyz float64 [n, 3], bound float64 [n]): the pixels pixel_of back-projected in float64 from the same float32
    inputs, and the bound on |float32 statement - this| per coordinate.

    Derivation, to first order in U, with a = |P0 xc|, b = |P1 yc|, c = |P2 z| and S = a + b + c + |P3| (every partial
    sum of X is at most S in magnitude):
      z = d / shift: one rounding; it scales xc, yc and P2 z alike            -> U (a + b + c)
      xc = (((i + 0.5) - cx) z) / fx: i + 0.5 is exact; -, *, / round        -> 3 U a;  yc likewise -> 3 U b
      the products P0 xc, P1 yc, P2 z                                        -> U (a + b + c)
      the three sums                                                         -> 3 U S
    in all U (5 a + 5 b + 2 c + 3 S) <= 8 U S: eight roundings of half an ulp of something no larger than S.  The
    bound asserted is 10 U S: the two spare units cover the second-order terms (about 8^2 U^2 S) and the rounding of
    this float64 restatement itself many times over."""
    F, H, W = fr.depth.shape
    Hs, Ws = -(-H // stride), -(-W // stride)
    t = pixel_of.astype(np.int64)
    f, r = t // (Hs * Ws), t % (Hs * Ws)
    j, i = (r // Ws) * stride, (r % Ws) * stride
    tab = fr.table.astype(np.float64)
    z = fr.depth.numpy()[f, j, i].astype(np.float64) / np.float64(np.float32(fr.depth_shift))
    xc = (i + 0.5 - tab[f, 2]) * z / tab[f, 0]
    yc = (j + 0.5 - tab[f, 3]) * z / tab[f, 1]
    P = tab[f, 4:].reshape(-1, 3, 4)
    cam = np.stack([xc, yc, z, np.ones_like(z)], axis=1)
    xyz = np.einsum("nak,nk->na", P, cam)
    S = np.einsum("nak,nk->na", np.abs(P), np.abs(cam))
    return xyz, 10 * U * S


@pytest.mark.parametrize("kind,stride,edge", [("u16", 1, None), ("f32", 1, 0.05), ("u16", 2, 0.05), ("f32", 3, None)])
@pytest.mark.parametrize("case", ["narrow", "dense"])
def test_backproject_host_against_float64(case, kind, stride, edge):
    fr = fc.make(getattr(fc, case)(), kind)
    xyz, rgb, pixel_of, point_of, flag = frames.backproject_host(fr, stride, 0.1, 10.0, edge)
    n = xyz.shape[0]
    assert n > 50 and not flag and xyz.dtype == np.float32 and rgb.dtype == np.uint8 and pixel_of.dtype == np.int32
    assert (np.diff(pixel_of) > 0).all() and (point_of.reshape(-1)[pixel_of] == np.arange(n)).all()
    assert (point_of >= 0).sum() == n
    ref, bound = _f64_points(fr, stride, pixel_of)
    err = np.abs(xyz.astype(np.float64) - ref)
    print(f"{case} {kind} stride {stride}: n = {n}, largest error / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all()
    # the colours are those of the pixels
    F, H, W = fr.depth.shape
    assert (rgb == fr.color.numpy()[:, ::stride, ::stride].reshape(-1, 3)[pixel_of]).all()


def test_validity_range_and_edge_filter():
    d = np.full((1, 5, 6), 2.0, np.float32)
    d[0, 0, 0], d[0, 0, 1], d[0, 0, 2], d[0, 0, 3], d[0, 0, 4] = np.nan, np.inf, 0.0, -1.0, 11.0
    d[0, 3, 3] = 2.5  # a flying pixel: 0.5 > 0.05 * 2.5 and > 0.05 * 2.0
    d[0, 4, 5] = 2.05  # |2.05 - 2| = 0.05 < 0.05 * 2.05 and < 0.05 * 2: stays, and drops no neighbour
    fr = frames.make(d, [50.0, 50.0, 3.0, 2.5], np.eye(4)[None], depth_shift=1.0)
    off = frames.backproject_host(fr, 1, 0.1, 10.0, None)[3][0] >= 0
    want = np.ones((5, 6), bool)
    want[0, :5] = False
    assert (off == want).all()
    on = frames.backproject_host(fr, 1, 0.1, 10.0, 0.05)[3][0] >= 0
    want[3, 3] = want[2, 3] = want[4, 3] = want[3, 2] = want[3, 4] = False  # the flying pixel and its four neighbours
    assert (on == want).all()  # (the out-of-range pixels of row 0 drop no neighbour: row 1 stays)
    # a stride samples the full-resolution decision: the neighbours stay those at one full-resolution pixel
    s2 = frames.backproject_host(fr, 2, 0.1, 10.0, 0.05)[3][0] >= 0
    assert s2.shape == (3, 3) and (s2 == want[::2, ::2]).all()
    # near / far are closed bounds
    assert (frames.backproject_host(fr, 1, 2.0, 2.0, None)[3][0] >= 0).sum() == 30 - 5 - 2


def test_round_trip_with_the_renderer():
    """Render at radius 0 with fx = fy = scale, back-project the depth: pixel (i, j) holds the point whose projection
    (u, v) fell into [i, i + 1) x [j, j + 1) at depth z exactly; its centre is at most half a pixel away on each axis,
    which is z * 0.5 / f metres in the camera's x and y: z * sqrt(0.5) / f in all, plus the float32 bound."""
    case = fc.round_trip()
    fr = fc.make(case, "f32")
    xyz, _, pixel_of, point_of, _ = frames.backproject_host(fr, 1, 0.1, 10.0, None)
    fg = case.index.reshape(-1) >= 0
    assert ((point_of.reshape(-1) >= 0) == fg).all() and fg.sum() > 2000
    src = fc.small_scene()[0][case.index.reshape(-1)[pixel_of]].astype(np.float64)
    z = case.depth_m.reshape(-1)[pixel_of].astype(np.float64)
    _, fbound = _f64_points(fr, 1, pixel_of)
    dist = np.linalg.norm(xyz.astype(np.float64) - src, axis=1)
    bound = z * np.sqrt(0.5) / case.K[0] + np.linalg.norm(fbound, axis=1)
    print(f"round trip: largest distance / bound = {(dist / bound).max():.3f}")
    assert (dist <= bound).all()
    # a transposed pose must fail it
    bad = frames.make(np.array(case.depth_m), case.K, np.stack([np.block([[P[:3, :3].T, P[:3, 3:]], [P[3:]]]) for P in case.pose]),
                      depth_shift=1.0)
    xb = frames.backproject_host(bad, 1, 0.1, 10.0, None)[0]
    assert (np.linalg.norm(xb.astype(np.float64) - src, axis=1) > bound).mean() > 0.9
    # and frames.camera gives back the camera the frame was rendered with
    cam = frames.camera(fr, 1)
    want = case.cams[1]
    assert cam.kind == "persp" and cam.scale == want.scale and (cam.cx, cam.cy) == (want.cx, want.cy)
    assert np.allclose(cam.eye, want.eye, atol=1e-6) and np.allclose(cam.R, want.R, atol=1e-6)


def _cells(cell, stride=1):
    fr = fc.make(fc.dense(), "u16")
    xyz, rgb, _, _, _ = frames.backproject_host(fr, stride, 0.1, 10.0, None)
    origin = xyz.min(0)
    _, cell_of, count = postprocess.grid_subsample_host(xyz, cell, "first", origin)
    return xyz, rgb, cell_of, count, origin


@pytest.mark.parametrize("cell", [100.0, 0.05, 1e-5])
def test_cell_means_host_against_float64_mean(cell):
    xyz, rgb, cell_of, count, origin = _cells(cell)
    M = count.shape[0]
    got, col, cnt, new_id, flag = frames.cell_means_host(xyz, rgb, cell_of, count, origin, 1)
    assert not flag and (new_id == np.arange(M)).all() and (cnt == count).all() and got.dtype == np.float32
    assert M == {100.0: 1, 1e-5: xyz.shape[0]}.get(cell, M)
    mean = np.zeros((M, 3))
    np.add.at(mean, cell_of, xyz.astype(np.float64))
    mean /= count[:, None]
    # every point is rounded down to the 2^-20 m grid (so is the mean, by less than 2^-20); one float32 rounding at
    # the end, of a value of magnitude at most |mean| + 2^-20; the float64 operations are far below both
    bound = 2.0 ** -20 + U * (np.abs(mean) + 2.0 ** -20) + 1e-12
    err = np.abs(got.astype(np.float64) - mean)
    print(f"cell {cell}: {M} cells, largest error / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all()
    csum = np.zeros((M, 3))
    np.add.at(csum, cell_of, rgb.astype(np.float64))
    assert (np.abs(col.astype(np.float64) - csum / count[:, None]) <= 0.5 + 1e-9).all()


def test_cell_means_host_is_order_free_and_renumbers_in_order():
    xyz, rgb, cell_of, count, origin = _cells(0.05)
    a = frames.cell_means_host(xyz, rgb, cell_of, count, origin, 1)
    perm = np.random.default_rng(0).permutation(xyz.shape[0])
    b = frames.cell_means_host(xyz[perm], rgb[perm], cell_of[perm], count, origin, 1)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)  # bit for bit: integer sums
    xo, co, cnt, new_id, _ = frames.cell_means_host(xyz, rgb, cell_of, count, origin, 3)
    keep = count >= 3
    assert 0 < keep.sum() < keep.size and not keep[:keep.nonzero()[0][-1]].all()  # cells dropped in the middle
    assert (new_id[~keep] == -1).all() and (new_id[keep] == np.arange(keep.sum())).all()
    assert np.array_equal(xo, a[0][keep]) and np.array_equal(co, a[1][keep]) and np.array_equal(cnt, count[keep])
    far = xyz.copy()
    far[7, 1] = origin[1] + 20000.0
    assert frames.cell_means_host(far, rgb, cell_of, count, origin, 1)[4] == 1


@pytest.mark.parametrize("stride,edge,min_obs", [(1, None, 1), (2, 0.05, 1), (1, 0.05, 3)])
def test_fuse_host_pixels_fall_into_their_points_cell(stride, edge, min_obs):
    cell = np.float32(0.05)
    fr = fc.make(fc.dense(), "u16")
    fused = frames.fuse_host(fr, cell, stride, 0.1, 10.0, edge, min_obs)
    xyz, _, pixel_of, point_of, _ = frames.backproject_host(fr, stride, 0.1, 10.0, edge)
    origin = xyz.min(0)
    p = fused.point_of.numpy()
    n = fused.xyz.shape[0]
    assert p.shape == point_of.shape and p.dtype == np.int32 and ((p >= 0) <= (point_of >= 0)).all()
    assert p.max() == n - 1 and np.unique(p[p >= 0]).size == n
    on = p.reshape(-1)[pixel_of] >= 0
    assert (min_obs == 1) == bool(on.all())
    assert int(fused.count.sum()) == int((p >= 0).sum()) == int(on.sum()) and int(fused.count.min()) >= min_obs
    own = np.floor((xyz[on] - origin) / cell)                     # the cell of every pixel's own back-projection ...
    mean = fused.xyz.numpy()[p.reshape(-1)[pixel_of][on]]
    # ... holds the fused point: the mean of points of one cell lies in that cell (closed: a mean may round onto its face)
    lo, hi = origin + own * cell, origin + (own + 1) * cell
    assert ((mean >= lo - 1e-6) & (mean <= hi + 1e-6)).all()
    # points are numbered in order of their first pixel
    first = np.full(n, p.size, np.int64)
    np.minimum.at(first, p.reshape(-1)[p.reshape(-1) >= 0], np.nonzero(p.reshape(-1) >= 0)[0])
    assert (np.diff(first) > 0).all()
    raw, shift = fused.raw_scene()
    assert raw.shape == (n, 8) and raw.dtype == np.float64 and (raw[:, 6:] == -100).all()
    assert np.abs(raw[:, :3].mean(0)).max() < 1e-9 and np.allclose(raw[:, :3] + shift, fused.xyz.numpy().astype(np.float64))
    assert np.array_equal(raw[:, 3:6], fused.rgb.numpy() / 127.5 - 1)
    raw0, shift0 = fused.raw_scene(center=False)
    assert (shift0 == 0).all() and np.array_equal(raw0[:, :3], fused.xyz.numpy().astype(np.float64))


def test_cpu_tensors_run_the_statements_and_gather():
    fr = fc.make(fc.narrow(), "f32")
    a = frames.fuse(fr, 0.05, 2, edge=0.05, device="cpu")
    b = frames.fuse_host(fr, 0.05, 2, edge=0.05)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    xyz, rgb, pixel_of, point_of = frames.backproject(fr, 2, edge=0.05)
    h = frames.backproject_host(fr, 2, edge=0.05)
    assert all(np.array_equal(x.numpy(), y) for x, y in zip((xyz, rgb, pixel_of, point_of), h))
    n = a.xyz.shape[0]
    vals = torch.arange(n, dtype=torch.int32) * 3 + 5
    img = frames.gather(a, vals, fill=-7)
    p = a.point_of
    assert img.shape == p.shape and img.dtype == torch.int32
    assert (img[p < 0] == -7).all() and torch.equal(img[p >= 0], vals[p[p >= 0].long()])
    img3 = frames.gather(a, a.rgb.numpy(), fill=0)
    assert img3.shape == tuple(p.shape) + (3,) and torch.equal(img3[p >= 0], a.rgb[p[p >= 0].long()])
    with pytest.raises(ValueError):
        frames.gather(a, vals[:-1])
    empty = frames.fuse(fr, 0.05, near=20.0, far=30.0, device="cpu")
    assert empty.xyz.shape == (0, 3) and (empty.point_of == -1).all() and empty.raw_scene()[0].shape == (0, 8)


def test_value_errors():
    c = fc.narrow()
    d, K, pose, col = np.array(c.depth_mm), c.K, c.pose, np.array(c.color)
    ok = frames.make(d, K, pose, col)
    assert ok.table.shape == (3, frames.RECORD_FLOATS) and ok.table.dtype == np.float32 and ok.depth_shift == 1000.0
    assert frames.make(d, np.tile(K, (3, 1)), pose).color is None

    def bad(*a, **k):
        with pytest.raises(ValueError):
            frames.make(*a, **k)

    bad(d.astype(np.int32), K, pose)            # dtype
    bad(d[0], K, pose)                          # shape
    bad(d, K[:3], pose)
    bad(d, np.tile(K, (2, 1)), pose)
    bad(d, K, pose[:2])
    bad(d, K, pose[:, :3])
    bad(d, K, pose, col[..., :2])
    bad(d, K, pose, col.astype(np.float32))
    for k, v in ((0, 0.0), (1, -1.0), (2, np.nan), (3, np.inf)):
        Kb = K.copy()
        Kb[k] = v
        bad(d, Kb, pose)
    for at, v in (((1, 0, 3), np.nan), ((2, 3, 3), 2.0), ((0, 3, 0), 1e-3), ((0, 1, 1), np.inf)):
        Pb = pose.copy()
        Pb[at] = v
        bad(d, K, Pb)
    bad(d, K, pose, depth_shift=0.0)
    bad(d, K, pose, depth_shift=np.inf)
    for kw in ({"stride": 0}, {"edge": -0.1}, {"edge": np.nan}, {"cell": 0.0}, {"min_obs": 0}, {"origin": [0.0, 1.0]}):
        with pytest.raises(ValueError):
            frames.fuse_host(ok, **kw)
    with pytest.raises(ValueError):
        frames.backproject(ok, chunk=100)
    with pytest.raises(ValueError, match="fx"):
        frames.camera(frames.make(d, K * np.array([1, 2, 1, 1]), pose), 0)
    with pytest.raises(ValueError):
        frames.camera(ok, 3)
    # an origin above a point: the grid refuses it
    with pytest.raises(ValueError):
        frames.fuse_host(ok, 0.05, origin=[10.0, 10.0, 10.0])
