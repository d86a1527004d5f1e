"""GPU: the splat and resolve kernels (csrc/render.hip) bit for bit against the host statement (render.splat_host /
resolve_host) in both launch regimes, the named situations, the argument checks, and render.render end to end on the
labels of batch_eval.label_batches and through the files tools/predict_scenes.py writes."""
import os

import numpy as np
import pytest
import torch

from geoformer_amd import render
from tests.render_cases import host_arrays, named_cases, random_case, render_kwargs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (7, 5), (64, 64), (65, 33), (130, 70)]


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _check(case, shade=render.Shade(), **more):
    """keys, index and image of the kernels against the host statement, each run twice; render.render too."""
    xyz, keep, table, Ws, Hs, maxr = host_arrays(case)
    S = case["supersample"]
    shade = case.get("shade", shade)
    want_keys = render.splat_host(xyz, keep, table, Ws, Hs, maxr)
    want_image, want_index = render.resolve_host(want_keys, S, case["rgb"], case["ids"], shade, **more)
    d = {k: _dev(case[k]) for k in ("xyz", "rgb", "ids", "keep")}
    runs = []
    for _ in range(2):
        keys = render.splat(d["xyz"], d["keep"], table, Ws, Hs, maxr)
        runs.append((keys,) + render.resolve(keys, S, d["rgb"], d["ids"], shade, **more))
    kw = dict(render_kwargs(case), shade=shade)
    runs.append((None,) + render.render(d["xyz"], d["rgb"], case["cams"], case["size"], ids=d["ids"], keep=d["keep"],
                                        **kw, **more))
    torch.cuda.synchronize()
    for keys, image, index in runs:
        if keys is not None:
            assert keys.dtype == torch.int64 and keys.is_cuda and keys.is_contiguous()
            assert torch.equal(keys.cpu(), torch.from_numpy(want_keys.view(np.int64)))
        assert image.dtype == torch.uint8 and index.dtype == torch.int32 and image.is_cuda and index.is_cuda
        assert torch.equal(index.cpu(), torch.from_numpy(want_index))
        assert torch.equal(image.cpu(), torch.from_numpy(want_image))
    return want_keys, want_image, want_index


@pytest.mark.parametrize("kind", ["ortho", "persp"])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257, 4000])
def test_kernels_equal_statement_over_point_counts(hip, N, kind):
    """N inside a wave, on its edge, past it, past a workgroup (256) and over 16 workgroups; radius 1 runs the
    thread-per-point kernel, radius 5 the wave kernel (a partial last wave at 1, 63, 65, 257)."""
    assert render.limits() == (20, 64, 4096, 16, 4)
    for radius in (1, 5):
        case = random_case(N, (65, 33), 3 if N <= 257 else 1, 2, kind, radius, seed=N)
        keys, _, index = _check(case)
        assert N < 63 or (index >= 0).any()


@pytest.mark.parametrize("S", [1, 2, 3])
@pytest.mark.parametrize("size", SIZES)
def test_kernels_equal_statement_over_image_sizes(hip, size, S):
    """1 x 1 (every neighbour outside), sides that are no multiple of the resolve block (64 x 4), on it, and past it."""
    for V, kind, radius in ((1, "persp", 2), (3, "ortho", (1, 6))):
        _check(random_case(257, size, V, S, kind, radius, seed=size[0] + S, point_size=0.5))


@pytest.mark.parametrize("kind", ["ortho", "persp"])
@pytest.mark.parametrize("radius", [0, 1, 3, 4, render.MAX_RADIUS, (0, 3), (0, 4), (2, render.MAX_RADIUS)])
def test_kernels_equal_statement_over_radii(hip, radius, kind):
    """The launch shape changes between max_radius 3 (render.SMALL_RADIUS: a thread per point and view) and 4 (a wave per
    64 points, lanes over each footprint): 3 and 4 are both here, with one radius and with radii that vary by depth."""
    assert render.SMALL_RADIUS == 3 and render.MAX_RADIUS == render.limits()[3]
    case = random_case(500, (130, 70), 3, 1, kind, radius, seed=11, point_size=0.25)
    _check(case)
    if isinstance(radius, tuple) and kind == "persp":
        xyz, _, table, Ws, Hs, maxr = host_arrays(case)
        ok, _, _, r, _ = render.project_host(xyz, table[0], Ws, Hs, maxr)
        assert len(np.unique(r[ok])) > 1


@pytest.mark.parametrize("name", sorted(named_cases()))
def test_named_cases(hip, name):
    case = named_cases()[name]
    keys, image, index = _check(case)
    assert (index >= 0).any()
    if name.startswith("contention"):
        z = case["xyz"][:, 2]
        assert index[0, 4, 6] == np.nonzero(z == z.min())[0][0]
    if name == "same_position":
        assert set(np.unique(index)) == {-1, 0, 1}
    if name == "keep_removes_nearest":
        assert set(np.unique(index)) == {-1, 1, 2}


def test_shading_outline_and_colours_on_the_device(hip):
    case = random_case(3000, (65, 33), 2, 2, "persp", 3, seed=2)
    for shade in (None, render.Shade(), render.Shade((256, 200, 150, 100, 80, 60, 40, 20, 0), 1, 0.0),
                  render.Shade(stride=render.MAX_STRIDE)):
        _check(case, shade=shade, background=(1, 2, 3), outline=(250, 0, 9))
    case["ids"] = None
    _check(case)


def test_empty_scene_and_view_chunking(hip):
    cams = render.turntable((np.zeros(3), np.ones(3)), 2, 20.0, (9, 6))
    xyz = torch.zeros((0, 3), device="cuda")
    rgb = torch.zeros((0, 3), dtype=torch.uint8, device="cuda")
    image, index = render.render(xyz, rgb, cams, (9, 6), background=(5, 6, 7))
    assert image.shape == (2, 6, 9, 3) and index.shape == (2, 12, 18)
    assert (index == -1).all() and (image.cpu() == torch.tensor([5, 6, 7], dtype=torch.uint8)).all()
    case = random_case(2000, (33, 20), 5, 2, "persp", 2, seed=8)
    d = {k: _dev(case[k]) for k in ("xyz", "rgb", "ids", "keep")}
    kw = dict(ids=d["ids"], keep=d["keep"], **render_kwargs(case))
    whole = render.render(d["xyz"], d["rgb"], case["cams"], case["size"], **kw)
    per_view = 8 * 66 * 40
    for max_bytes in (per_view, 2 * per_view + 1, 1):  # one view, two views (a last chunk of one), less than a view
        got = render.render(d["xyz"], d["rgb"], case["cams"], case["size"], max_bytes=max_bytes, **kw)
        assert torch.equal(got[0], whole[0]) and torch.equal(got[1], whole[1])
    want = render.render_host(case["xyz"], case["rgb"], case["cams"], case["size"], ids=case["ids"], keep=case["keep"],
                              **render_kwargs(case))
    assert torch.equal(whole[0].cpu(), torch.from_numpy(want[0])) and torch.equal(whole[1].cpu(), torch.from_numpy(want[1]))


def test_no_points_and_argument_checks_launch_nothing(hip):
    from geoformer_amd import _lib

    case = random_case(300, (16, 8), 2, 2, "persp", 2, seed=4)
    xyz, keep, table, Ws, Hs, maxr = host_arrays(case)
    st = _lib.stream_ptr()
    d_xyz, d_keep, d_tab, d_rgb, d_ids = _dev(xyz), _dev(keep), _dev(table), _dev(case["rgb"]), _dev(case["ids"])
    keys = torch.full((2, Hs, Ws), 77, dtype=torch.int64, device="cuda")
    image = torch.full((2, 8, 16, 3), 9, dtype=torch.uint8, device="cuda")
    index = torch.full((2, Hs, Ws), 77, dtype=torch.int32, device="cuda")
    lut = np.array(render.Shade().lut, np.int32)
    side = render.MAX_SIDE * render.MAX_SUPERSAMPLE

    def splat(xyz=d_xyz.data_ptr(), N=300, cams=d_tab.data_ptr(), V=2, Ws=Ws, Hs=Hs, r=2, out=keys.data_ptr()):
        return hip.gf_render_splat(xyz, d_keep.data_ptr(), N, cams, V, Ws, Hs, r, out, st)

    def resolve(k=keys.data_ptr(), V=2, W=16, H=8, S=2, rgb=d_rgb.data_ptr(), N=300, h_lut=lut.ctypes.data, stride=2,
                bg=0xFFFFFF, ol=0, im=image.data_ptr(), ix=index.data_ptr()):
        return hip.gf_render_resolve(k, V, W, H, S, rgb, d_ids.data_ptr(), N, h_lut, stride, 0.02, bg, ol, im, ix, st)

    assert splat(N=0) == 0 and splat(N=0, xyz=None) == 0  # no points: returns at once, nothing launched
    assert splat(xyz=None) == -1 and splat(cams=None) == -1 and splat(out=None) == -1
    assert b"NULL" in hip.gf_last_error()
    assert splat(V=0) == -1 and splat(V=render.MAX_VIEWS + 1) == -1
    assert splat(Ws=0) == -1 and splat(Hs=0) == -1 and splat(Ws=side + 1) == -1 and splat(Hs=side + 1) == -1
    assert splat(r=-1) == -1 and splat(r=render.MAX_RADIUS + 1) == -1
    assert splat(N=-1) == -1 and splat(N=1 << 31) == -1
    assert resolve(k=None) == -1 and resolve(rgb=None) == -1 and resolve(h_lut=None) == -1
    assert resolve(im=None) == -1 and resolve(ix=None) == -1
    assert resolve(V=0) == -1 and resolve(V=render.MAX_VIEWS + 1) == -1
    assert resolve(W=0) == -1 and resolve(H=0) == -1 and resolve(W=render.MAX_SIDE + 1) == -1
    assert resolve(S=0) == -1 and resolve(S=render.MAX_SUPERSAMPLE + 1) == -1
    assert resolve(stride=0) == -1 and resolve(stride=render.MAX_STRIDE + 1) == -1
    assert resolve(bg=-1) == -1 and resolve(ol=1 << 24) == -1 and resolve(N=-1) == -1
    bad = lut.copy()
    bad[8] = 257
    assert resolve(h_lut=bad.ctypes.data) == -1 and b"lut[8]" in hip.gf_last_error()
    torch.cuda.synchronize()
    assert (keys == 77).all() and (image == 9).all() and (index == 77).all()  # none of them launched
    keys.fill_(-1)
    assert splat() == 0 and resolve() == 0
    torch.cuda.synchronize()
    want_keys = render.splat_host(xyz, keep, table, Ws, Hs, maxr)
    want = render.resolve_host(want_keys, 2, case["rgb"], case["ids"], render.Shade())
    assert torch.equal(keys.cpu(), torch.from_numpy(want_keys.view(np.int64)))
    assert torch.equal(image.cpu(), torch.from_numpy(want[0])) and torch.equal(index.cpu(), torch.from_numpy(want[1]))
    # a record whose radii exceed the caller's bound is clamped to it, on the device as in the statement
    wide = table.copy()
    wide[:, 18:20] = (9.0, 40.0)
    got = render.splat(d_xyz, None, wide, Ws, Hs, 2)
    assert torch.equal(got.cpu(), torch.from_numpy(render.splat_host(xyz, None, wide, Ws, Hs, 2).view(np.int64)))
    # the wrappers, before any launch
    with pytest.raises(RuntimeError, match="keep"):
        render.splat(d_xyz, d_keep[:-1], table, Ws, Hs, 2)
    with pytest.raises(ValueError, match="cams"):
        render.splat(d_xyz, None, table[:, :19], Ws, Hs, 2)
    with pytest.raises(RuntimeError, match="ids"):
        render.resolve(keys, 2, d_rgb, d_ids.long())
    with pytest.raises(RuntimeError, match="keys"):
        render.resolve(keys, 3, d_rgb)
    with pytest.raises(RuntimeError, match="rgb"):
        render.render(d_xyz, d_rgb[:-1], case["cams"], case["size"])


# ---- end to end ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(hip):
    from geoformer_amd.model import GeoFormer, load_config
    from tests.util import synthetic_state_dict

    m = GeoFormer(load_config("test_geoformer_scannet.yaml"))
    m.load_state_dict(synthetic_state_dict(m.state_dict(), 0))
    m.cuda()
    m.eval()
    return m


def test_label_batches_to_pictures_and_files(model, tmp_path):
    import importlib.util

    from geoformer_amd import batch_eval, export, scene

    items = [("a", scene.make_raw_scene(3000, 41)), ("b", scene.make_raw_scene(2500, 42))]
    np.random.seed(21)
    results = list(batch_eval.label_batches(model, items, 2, min_score=0.0, reserve=False, final_score_thresh=0.0))
    assert [n for n, _ in results] == ["a", "b"]
    size = (96, 64)
    spec = importlib.util.spec_from_file_location("predict_scenes_render", os.path.join(ROOT, "tools", "predict_scenes.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    paths = tool.write_renders(str(tmp_path), results, dict(items), ("top", 1), size, "instance_pred")
    assert [os.path.relpath(p, str(tmp_path)) for p in paths] == ["render/a_instance_pred_0.png",
                                                                  "render/b_instance_pred_0.png"]
    for (name, lab), (_, raw), path in zip(results, items, paths):
        xyz = raw[:, :3].astype(np.float32)
        owner = torch.as_tensor(lab.owner).cuda()
        rgb, ids, keep = render.colors_for("instance_pred", labels=lab._replace(owner=owner))
        assert rgb.is_cuda and ids.is_cuda and keep is None
        cams = [render.top_down(render.bounds_of(xyz), size)]
        image, index = render.render(torch.from_numpy(xyz).cuda(), rgb, cams, size, ids=ids)
        want = render.render_host(xyz, rgb.cpu().numpy(), cams, size, ids=ids.cpu().numpy())
        assert torch.equal(image.cpu(), torch.from_numpy(want[0])) and torch.equal(index.cpu(), torch.from_numpy(want[1]))
        assert (want[1] >= 0).mean() > 0.2
        assert np.array_equal(export.read_png(path), want[0][0]), name
