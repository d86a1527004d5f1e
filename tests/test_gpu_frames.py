"""csrc/frames.hip on the GPU: every case bit for bit against the numpy statement of geoformer_amd.frames, and each call
made twice for equality from call to call.  The shapes and what each straddles are named in tests/frames_cases.py."""
import numpy as np
import pytest
import torch

from geoformer_amd import frames, postprocess
from tests import frames_cases as fc

pytestmark = pytest.mark.gpu


def _dev(fr):
    return fr._replace(depth=fr.depth.cuda(), color=None if fr.color is None else fr.color.cuda())


def _backproject_equals_host(fr, stride, near, far, edge, chunk=None):
    want = frames.backproject_host(fr, stride, near, far, edge)
    assert not want[4]
    d = _dev(fr)
    a = frames.backproject(d, stride, near, far, edge, chunk, return_origin=True)
    b = frames.backproject(d, stride, near, far, edge, chunk)
    if want[0].shape[0]:
        assert np.array_equal(a[4].cpu().numpy(), want[0].min(0))  # (as values: a minimum of -0 and +0 may be either)
    for x, y, w, name in zip(a, b, want, ("xyz", "rgb", "pixel_of", "point_of")):
        x, y = x.cpu().numpy(), y.cpu().numpy()
        assert x.dtype == w.dtype and x.shape == w.shape, name
        assert np.array_equal(x.view(np.uint8), w.view(np.uint8)), name  # the bits, so that -0 and NaN count
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), name
    return want


@pytest.mark.parametrize("kind,color,edge", [("u16", True, None), ("f32", False, 0.05)])
@pytest.mark.parametrize("stride", [1, 2, 3])
def test_narrow_frames(hip, stride, kind, color, edge):
    assert frames.limits()
    n = _backproject_equals_host(fc.make(fc.narrow(), kind, color), stride, 0.1, 10.0, edge)[0].shape[0]
    assert n > 50


@pytest.mark.parametrize("depth,n", [(1234, 1), (0, 0)])
def test_one_pixel(hip, depth, n):
    fr = frames.make(np.full((1, 1, 1), depth, np.uint16), [1.5, 2.5, 0.25, 0.75], fc.dense().pose[:1],
                     np.full((1, 1, 1, 3), 200, np.uint8))
    want = _backproject_equals_host(fr, 1, 0.1, 10.0, 0.05)
    assert want[0].shape[0] == n
    assert frames.fuse(fr, 0.02).xyz.shape[0] == n


@pytest.mark.parametrize("frames_n,chunk", [(3, None), (3, fc.SMALL_CHUNK), (fc.DENSE_FRAMES_TOP, fc.SMALL_CHUNK),
                                            (fc.DENSE_FRAMES_TOP, 3 * fc.WAVE)])
@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_dense_frames_with_an_empty_and_a_full_workgroup(hip, frames_n, chunk, kind):
    d = fc.gaps(frames_n)
    depth = d if kind == "f32" else np.rint(d.astype(np.float64) * 1000).astype(np.uint16)
    fr = fc.make(fc.dense(frames_n), depth=depth)
    want = _backproject_equals_host(fr, 1, 0.1, 10.0, None, chunk)
    per = fc.DENSE[0] * fc.DENSE[1]
    p = want[3].reshape(frames_n, per)
    c = chunk or fc.CHUNK
    nb = -(-p.size // c)
    kept = np.array([(p.reshape(-1)[b * c:(b + 1) * c] >= 0).sum() for b in range(nb)])
    assert (kept == 0).any() and (kept[:-1] == c).any() and ((kept > 0) & (kept < c)).any()
    assert (nb > fc.TOP) == (frames_n == fc.DENSE_FRAMES_TOP and chunk == fc.SMALL_CHUNK)


@pytest.mark.parametrize("edge", [None, 0.05])
def test_float_depth_with_nan_inf_zero_and_negative_values(hip, edge):
    fr = fc.make(fc.dense(), depth=fc.nasty())
    want = _backproject_equals_host(fr, 1, 0.1, 10.0, edge)
    bad = ~np.isfinite(fc.nasty()) | (fc.nasty() <= 0)
    assert bad.mean() > 0.15 and (want[3][bad] == -1).all() and want[0].shape[0] > 1000


def test_no_valid_pixel(hip):
    fr = fc.make(fc.dense(), "f32")
    want = _backproject_equals_host(fr, 2, 20.0, 30.0, None)
    assert want[0].shape == (0, 3) and (want[3] == -1).all()
    f = frames.fuse(fr, 0.02, 2, near=20.0, far=30.0)
    assert f.xyz.shape == (0, 3) and f.xyz.is_cuda and f.count.numel() == 0 and bool((f.point_of == -1).all())


def test_a_coordinate_beyond_float32_is_a_value_error(hip):
    pose = fc.dense().pose[:1].copy()
    pose[0, 0, 3] = 3e38
    pose[0, :3, :3] = np.eye(3) * 2
    fr = frames.make(np.full((1, 4, 4), 3e38, np.float32), [1.0, 1.0, 0.0, 0.0], pose, depth_shift=1.0)
    assert frames.backproject_host(fr, 1, 0.1, 3.4e38)[4] == 1
    with pytest.raises(ValueError, match="not finite"):
        frames.fuse_host(fr, far=3.4e38)
    with pytest.raises(ValueError, match="not finite"):
        frames.backproject(_dev(fr), 1, 0.1, 3.4e38)


# ---- cell means -------------------------------------------------------------------------------------------------------
def _cell_means_equal_host(xyz, rgb, cell, min_obs, chunk=None, origin=None):
    origin = xyz.min(0) if origin is None else origin
    _, cell_of, count = postprocess.grid_subsample_host(xyz, cell, "first", origin)
    want = frames.cell_means_host(xyz, rgb, cell_of, count, origin, min_obs)
    assert not want[4]
    t = [torch.from_numpy(np.array(a)).cuda() for a in (xyz, rgb, cell_of, count, origin)]
    runs = [frames.cell_means(*t, min_obs, chunk, agg) for agg in (True, True, False)]
    for r in runs:
        for x, w in zip(r, want):
            x = x.cpu().numpy()
            assert x.dtype == w.dtype and x.shape == w.shape and np.array_equal(x.view(np.uint8), w.view(np.uint8))
    return count, want


@pytest.fixture(scope="module")
def dense_points():
    xyz, rgb, _, _, _ = frames.backproject_host(fc.make(fc.dense(), "u16"), 1, 0.1, 10.0, None)
    return xyz, rgb


@pytest.mark.parametrize("cell,min_obs", [(100.0, 1), (1e-5, 1), (0.05, 1), (0.05, 3), (100.0, 100000)])
def test_cell_means_regimes(hip, dense_points, cell, min_obs):
    xyz, rgb = dense_points
    count, want = _cell_means_equal_host(xyz, rgb, cell, min_obs)
    n, M, m = xyz.shape[0], count.shape[0], want[0].shape[0]
    if cell == 100.0:
        assert M == 1 and m == (min_obs == 1)  # every point on one set of sums; or no cell kept at all
    elif cell == 1e-5:
        assert M == n == m                     # every point alone
    else:
        keep = count >= min_obs
        assert 1 < M < n and m == keep.sum() and (min_obs == 1 or not keep[:keep.nonzero()[0][-1]].all())


@pytest.mark.parametrize("cell,min_obs,chunk", [(1e-4, 1, fc.SMALL_CHUNK), (0.08, 2, fc.SMALL_CHUNK), (0.08, 2, None)])
def test_cell_means_over_many_workgroups(hip, cell, min_obs, chunk):
    xyz, rgb = fc.random_points()
    count, want = _cell_means_equal_host(xyz, rgb, cell, min_obs, chunk, origin=np.zeros(3, np.float32))
    M = count.shape[0]
    if cell == 1e-4:
        assert M // fc.SMALL_CHUNK > fc.TOP  # the scan of the chunk counts carries
    else:
        assert fc.CHUNK < M and 0 < want[0].shape[0] < M


def test_cell_means_flags_a_point_out_of_reach(hip):
    xyz = np.array([[0, 0, 0], [1, 20000, 1]], np.float32)
    t = [torch.from_numpy(a).cuda() for a in (xyz, np.zeros((2, 3), np.uint8), np.array([0, 1], np.int32),
                                              np.array([1, 1], np.int32), np.zeros(3, np.float32))]
    with pytest.raises(ValueError, match="16384 m"):
        frames.cell_means(*t)


# ---- fuse ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,cell,stride,edge,min_obs,origin", [
    ("u16", 0.02, 1, None, 1, None), ("f32", 0.02, 2, 0.05, 1, None), ("u16", 0.05, 1, 0.05, 3, (-2.0, -2.0, -1.0)),
    ("f32", 100.0, 1, None, 1, None)])
def test_fuse_equals_fuse_host(hip, kind, cell, stride, edge, min_obs, origin):
    fr = fc.make(fc.dense(), kind)
    want = frames.fuse_host(fr, cell, stride, 0.1, 10.0, edge, min_obs, origin)
    a = frames.fuse(fr, cell, stride, 0.1, 10.0, edge, min_obs, origin)  # host frames: moved to the device here
    b = frames.fuse(_dev(fr), cell, stride, 0.1, 10.0, edge, min_obs, origin)
    assert want.xyz.shape[0] > 0 and a.xyz.is_cuda
    for x, y, w in zip(a, b, want):
        assert x.dtype == w.dtype and x.shape == w.shape
        assert np.array_equal(x.cpu().numpy().view(np.uint8), w.numpy().view(np.uint8))
        assert np.array_equal(x.cpu().numpy().view(np.uint8), y.cpu().numpy().view(np.uint8))


def test_argument_checks_launch_nothing(hip):
    from geoformer_amd import _lib
    from geoformer_amd._lib import GeoFormerHipError, ptr

    lib = _lib.load()
    d = torch.zeros((2, 4, 4), dtype=torch.float32, device="cuda")
    tab = torch.ones((2, 16), dtype=torch.float32, device="cuda")
    out = torch.full((64,), 7, dtype=torch.int32, device="cuda")
    good = dict(F=2, W=4, H=4, stride=1, kind=1, shift=1.0, edge=0.0, chunk=0)
    for k, v in (("F", 0), ("F", lib.gf_frames_max_frames() + 1), ("W", 0), ("H", lib.gf_frames_max_side() + 1), ("stride", 0),
                 ("kind", 2), ("shift", 0.0), ("shift", float("inf")), ("edge", -1.0), ("edge", float("nan")), ("chunk", 32),
                 ("chunk", 100), ("chunk", 1 << 17)):
        a = dict(good, **{k: v})
        st = lib.gf_frames_backproject(ptr(d), a["kind"], a["shift"], None, ptr(tab), a["F"], a["W"], a["H"], a["stride"], 0.1,
                                       10.0, a["edge"], a["chunk"], ptr(out), ptr(out), ptr(out), ptr(out), ptr(out), None, ptr(out),
                                       None)
        assert st != 0, (k, v)
        with pytest.raises(GeoFormerHipError):
            _lib.check(st, "gf_frames_backproject")
    assert lib.gf_frames_backproject(ptr(d), 1, 1.0, None, ptr(tab), 2, 4, 4, 1, 0.1, 10.0, 0.0, 0, ptr(out), None, ptr(out),
                                     ptr(out), ptr(out), None, ptr(out), None) != 0  # a NULL output
    for n, M, min_obs, chunk in ((0, 1, 1, 0), (1, 0, 1, 0), (1, 1, 0, 0), (1, 1, 1, 65)):
        assert lib.gf_frames_cell_means(ptr(out), ptr(out), ptr(out), ptr(out), n, M, ptr(out), min_obs, 1, chunk, ptr(out),
                                        ptr(out), ptr(out), ptr(out), ptr(out), ptr(out), None) != 0
    assert lib.gf_frames_compose(ptr(out), -1, ptr(out), ptr(out), None) != 0
    assert lib.gf_frames_compose(None, 0, None, None, None) == 0
    torch.cuda.synchronize()
    assert bool((out == 7).all())


# ---- through the model --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(hip):
    from geoformer_amd.model import GeoFormer, load_config
    from tests.util import synthetic_state_dict

    m = GeoFormer(load_config("test_geoformer_scannet.yaml"))
    m.load_state_dict(synthetic_state_dict(m.state_dict(), 0))
    m.cuda()
    m.eval()
    return m


def test_frames_to_labels_and_back_to_the_frames(model):
    from geoformer_amd import batch_eval

    fused = frames.fuse(fc.make(fc.dense(), "u16"), 0.02)
    raw, shift = fused.raw_scene()
    n = fused.xyz.shape[0]
    assert raw.shape == (n, 8) and n > 1000
    np.random.seed(0)
    (name, labels), = batch_eval.label_batches(model, [("frames", raw)], 1)
    ids = np.asarray(labels.ids)
    assert name == "frames" and ids.shape == (n,)
    img = frames.gather(fused, ids, fill=-5).cpu().numpy()
    p = fused.point_of.cpu().numpy()
    assert img.shape == p.shape == (3, fc.DENSE[1], fc.DENSE[0]) and (p == -1).any() and (p >= 0).any()
    assert (img[p == -1] == -5).all() and np.array_equal(img[p >= 0], ids[p[p >= 0]])
