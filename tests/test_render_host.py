"""Host: the renderer's numpy statement (render.splat_host / resolve_host) against an independent per-pixel brute force
and hand-written pictures, the camera helpers, the PNG / PLY files, the command lines and the derived binding."""
import os
import struct
import zlib

import numpy as np
import pytest

from geoformer_amd import export, render
from tests.render_cases import (axis_case, brute_force_keys, host_arrays, named_cases, random_case, render_kwargs)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BG = 0xFFFFFFFFFFFFFFFF


def _host(case):
    return render.render_host(case["xyz"], case["rgb"], case["cams"], case["size"], ids=case["ids"], keep=case["keep"],
                              **render_kwargs(case))


@pytest.mark.parametrize("kind", ["ortho", "persp"])
@pytest.mark.parametrize("radius", [0, 1, 3, (1, 5)])
def test_splat_host_equals_per_pixel_brute_force(kind, radius):
    point_size = 2.0 if isinstance(radius, tuple) else 0.0  # (a focal length of 13 sub-pixels: radii 2 .. 5 with depth)
    case = random_case(150, (17, 11), 2, 1, kind, radius, seed=3, point_size=point_size)
    args = host_arrays(case)
    got, want = render.splat_host(*args), brute_force_keys(*args)
    assert got.dtype == np.uint64 and got.shape == (2, 11, 17)
    assert np.array_equal(got, want)
    assert 20 < int((got != BG).sum()) < got.size  # something was drawn, and something was not
    if isinstance(radius, tuple) and kind == "persp":
        assert len(np.unique(render.project_host(args[0], args[2][0], 17, 11, 5)[3])) > 1  # the radii do vary


@pytest.mark.parametrize("name", sorted(named_cases()))
def test_named_cases_equal_brute_force(name):
    case = named_cases()[name]
    if name.startswith("contention"):
        case = dict(case, xyz=case["xyz"][:60], rgb=case["rgb"][:60])
    args = host_arrays(case)
    got = render.splat_host(*args)
    assert np.array_equal(got, brute_force_keys(*args))
    assert (got != BG).any()


def test_named_cases_show_what_they_are_named_for():
    cases = named_cases()
    idx = {n: _host(c)[1][0] for n, c in cases.items() if not n.startswith("contention")}
    disc = 37  # cells of dx^2 + dy^2 <= 12
    for n in ("clip_left", "clip_right", "clip_top", "clip_bottom", "clip_corner", "centre_just_outside"):
        assert 0 < (idx[n] == 0).sum() < disc, n
    assert (idx["clip_left"][:, 0] == 0).sum() == 7 and (idx["clip_corner"][8, 11] == 0)
    assert set(np.unique(idx["outside_frustum"])) == {-1, 3}
    assert set(np.unique(idx["near_plane"])) == {-1, 0, 4} and idx["near_plane"][4, 6] == 0
    neg = idx["negative_depth_ortho"]
    assert (neg[3, 3], neg[3, 4], neg[3, 5]) == (0, 3, 6)  # -2 < -1 < 1; -0.0 sorts below +0.0; -0.5 < 0.5
    assert set(np.unique(idx["same_position"])) == {-1, 0, 1}
    assert set(np.unique(idx["keep_removes_nearest"])) == {-1, 1, 2}
    crowd = cases["contention_1000_on_one_pixel"]
    keys = render.splat_host(*host_arrays(crowd))
    z = crowd["xyz"][:, 2]
    assert (keys[0, 4, 6] & np.uint64(0xFFFFFFFF)) == np.nonzero(z == z.min())[0][0]


def test_hand_written_picture():
    """4 points on a 5 x 4 image, radius 0, no supersampling: point 1 hides point 0."""
    case = axis_case([(1.5, 1.5, 2.0), (1.5, 1.5, 1.0), (3.5, 0.5, -1.0), (4.5, 3.5, 5.0)], (5, 4),
                     rgb=[(9, 9, 9), (10, 20, 30), (200, 100, 0), (1, 2, 3)])
    keys = render.splat_host(*host_arrays(case))
    image, index = render.resolve_host(keys, 1, case["rgb"], background=(255, 255, 255))
    want_index = np.array([[-1, -1, -1, 2, -1],
                           [-1, 1, -1, -1, -1],
                           [-1, -1, -1, -1, -1],
                           [-1, -1, -1, -1, 3]], np.int32)
    want_image = np.full((4, 5, 3), 255, np.uint8)
    want_image[1, 1], want_image[0, 3], want_image[3, 4] = (10, 20, 30), (200, 100, 0), (1, 2, 3)
    assert index.dtype == np.int32 and np.array_equal(index[0], want_index)
    assert image.dtype == np.uint8 and np.array_equal(image[0], want_image)
    assert keys[0, 1, 1] == (np.uint64(0x80000000 | 0x3F800000) << np.uint64(32)) | np.uint64(1)  # 1.0f, point 1
    assert keys[0, 0, 3] == (np.uint64(~0xBF800000 & 0xFFFFFFFF) << np.uint64(32)) | np.uint64(2)  # -1.0f, point 2
    assert np.array_equal(render.depth_of_keys(keys)[0, [1, 0, 3], [1, 3, 4]], np.array([1.0, -1.0, 5.0], np.float32))


def _keys(depth, index):
    """uint64 keys of a depth image (float32; NaN = background) and an index image."""
    d = np.asarray(depth, np.float32)
    bits = np.where(np.isnan(d), np.float32(0), d).view(np.uint32)
    dk = np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000)).astype(np.uint64)
    k = (dk << np.uint64(32)) | np.asarray(index, np.int64).astype(np.uint64)
    return np.where(np.isnan(d), np.uint64(BG), k)[None]


def test_resolve_shading_counts():
    """The centre of a 3 x 3 patch with o nearer neighbours takes lut[o]; dz is a strict threshold."""
    lut = (256, 240, 224, 208, 192, 176, 160, 144, 128)
    rgb = np.array([[200, 100, 50]], np.uint8)
    order = [(0, 0), (0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1), (2, 2)]
    for o in range(9):
        d = np.full((3, 3), 2.0, np.float32)
        for y, x in order[:o]:
            d[y, x] = 1.0
        image, _ = render.resolve_host(_keys(d, np.zeros((3, 3))), 1, rgb, shade=render.Shade(lut, 1, 0.5))
        assert tuple(image[0, 1, 1]) == tuple((int(c) * lut[o] + 128) >> 8 for c in rgb[0]), o
    d = np.full((3, 3), 2.0, np.float32)
    d[0, 0] = 1.5  # 1.5 + 0.5 < 2.0 is false
    d[2, 2] = np.nan  # background never counts
    image, _ = render.resolve_host(_keys(d, np.zeros((3, 3))), 1, rgb, shade=render.Shade(lut, 1, 0.5))
    assert tuple(image[0, 1, 1]) == (200, 100, 50)
    # a stride of 2 looks two sub-pixels away and not one
    d = np.full((5, 5), 2.0, np.float32)
    d[1, 1] = 1.0
    d[0, 0] = 1.0
    image, _ = render.resolve_host(_keys(d, np.zeros((5, 5))), 1, rgb, shade=render.Shade(lut, 2, 0.5))
    assert tuple(image[0, 2, 2]) == tuple((int(c) * lut[1] + 128) >> 8 for c in rgb[0])


def test_resolve_outline_at_id_boundary_and_background():
    rgb = np.array([[10, 10, 10], [20, 20, 20], [30, 30, 30]], np.uint8)
    ids = np.array([7, 7, 9], np.int32)
    index = np.array([[0, 1, 2, 2],
                      [0, 0, 2, 2],
                      [0, 0, 0, 0]])
    d = np.ones((3, 4), np.float32)
    d[2, 3] = np.nan
    image, got_index = render.resolve_host(_keys(d, index), 1, rgb, ids=ids, outline=(255, 0, 0), background=(0, 0, 255))
    R, B = (255, 0, 0), (0, 0, 255)
    c = {0: (10, 10, 10), 1: (20, 20, 20), 2: (30, 30, 30)}
    want = [[c[0], R, c[2], c[2]],     # 1 | 2: another id to the right; points 0 and 1 share id 7
            [c[0], R, R, R],           # (1, 1): id 9 to the right; (1, 2): id 7 below; (1, 3): background below
            [c[0], c[0], R, B]]        # (2, 2): background to the right; the image's border is no boundary
    assert np.array_equal(image[0], np.array(want, np.uint8))
    assert np.array_equal(got_index[0], np.where(np.isnan(d), -1, index))
    flat, _ = render.resolve_host(_keys(d, index), 1, rgb, background=(0, 0, 255))
    assert np.array_equal(flat[0, :2], rgb[index[:2]])


@pytest.mark.parametrize("S", [1, 2, 3])
def test_resolve_integer_mean(S):
    rng = np.random.default_rng(S)
    H, W = 2, 3
    index = rng.integers(0, 50, (H * S, W * S))
    d = np.ones((H * S, W * S), np.float32)
    d[rng.random(d.shape) < 0.3] = np.nan
    rgb = rng.integers(0, 256, (50, 3), dtype=np.uint8)
    image, _ = render.resolve_host(_keys(d, index), S, rgb, background=(255, 254, 1))
    for y in range(H):
        for x in range(W):
            tot = np.zeros(3, np.int64)
            for sy in range(S):
                for sx in range(S):
                    yy, xx = y * S + sy, x * S + sx
                    tot += (255, 254, 1) if np.isnan(d[yy, xx]) else rgb[index[yy, xx]]
            assert tuple(image[0, y, x]) == tuple((tot + S * S // 2) // (S * S))


def test_camera_helpers_frame_the_bounds():
    lo, hi = np.array([-3.0, -1.0, 0.0]), np.array([5.0, 4.0, 2.5])
    corners = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])], np.float32)
    R = render.look_at((3.0, -2.0, 4.0), (0.5, 0.25, 0.0))
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-6 and abs(np.linalg.det(R) - 1) < 1e-6
    assert np.abs(R[2] - np.array([-2.5, 2.25, -4.0]) / np.linalg.norm([-2.5, 2.25, -4.0])).max() < 1e-6
    assert R[1, 2] < 0  # z up in the world is up in the image (down has a negative z)
    size = (64, 48)
    cams = [render.top_down((lo, hi), size)] + render.turntable((lo, hi), 5, 30.0, size) \
        + render.turntable((lo, hi), 3, -10.0, size, kind="ortho")
    assert [c.kind for c in cams] == ["ortho"] + ["persp"] * 5 + ["ortho"] * 3
    for S in (1, 2):
        table = render.camera_table(cams, S, 0)
        assert table.dtype == np.float32 and table.shape == (9, render.CAMERA_FLOATS)
        for c, row in zip(cams, table):
            assert np.abs(np.asarray(c.R).reshape(3, 3) @ np.asarray(c.R).reshape(3, 3).T - np.eye(3)).max() < 1e-6
            ok, iu, iv, r, _ = render.project_host(corners, row, 64 * S, 48 * S, 0)
            assert ok.all() and (iu >= 0).all() and (iu < 64 * S).all() and (iv >= 0).all() and (iv < 48 * S).all()
            assert (r == 0).all()
    with pytest.raises(ValueError, match="kind"):
        render.turntable((lo, hi), 2, 0.0, size, kind="fisheye")
    with pytest.raises(ValueError, match="radius"):
        render.camera_table(cams, 1, render.MAX_RADIUS + 1)
    with pytest.raises(ValueError, match="supersample"):
        render.camera_table(cams, 5, 1)


def test_png_round_trip_and_chunk_check(tmp_path):
    rng = np.random.default_rng(0)
    image = rng.integers(0, 256, (7, 5, 3), dtype=np.uint8)
    path = export.write_png(str(tmp_path / "a.png"), image)
    assert np.array_equal(export.read_png(path), image)
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, kinds, idat = 8, [], b""
    while at < len(data):
        n, kind = struct.unpack(">I4s", data[at:at + 8])
        body = data[at + 8:at + 8 + n]
        assert struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + body) & 0xFFFFFFFF
        kinds.append(kind)
        if kind == b"IHDR":
            assert struct.unpack(">IIBBBBB", body) == (5, 7, 8, 2, 0, 0, 0)
        if kind == b"IDAT":
            idat += body
        at += 12 + n
    assert kinds[0] == b"IHDR" and kinds[-1] == b"IEND" and b"IDAT" in kinds and at == len(data)
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(7, 16)
    assert not rows[:, 0].any() and np.array_equal(rows[:, 1:].reshape(7, 5, 3), image)
    # the other row filters, as another writer may use them: Sub, Up, Average, Paeth rows of the same image
    raw = np.zeros((7, 16), np.uint8)
    pad = np.zeros((8, 6, 3), np.int64)
    pad[1:, 1:] = image
    for y in range(7):
        ft = (1, 2, 3, 4, 0, 4, 1)[y]
        a, b, c = pad[y + 1, :-1], pad[y, 1:], pad[y, :-1]
        p = a + b - c
        paeth = np.where((abs(p - a) <= abs(p - b)) & (abs(p - a) <= abs(p - c)), a, np.where(abs(p - b) <= abs(p - c), b, c))
        pred = {0: 0, 1: a, 2: b, 3: (a + b) >> 1, 4: paeth}[ft]
        raw[y, 0], raw[y, 1:] = ft, ((pad[y + 1, 1:] - pred) & 255).reshape(-1)

    def chunk(kind, body):
        return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)

    other = tmp_path / "b.png"
    other.write_bytes(data[:8] + chunk(b"IHDR", struct.pack(">IIBBBBB", 5, 7, 8, 2, 0, 0, 0))
                      + chunk(b"tEXt", b"k\0v") + chunk(b"IDAT", zlib.compress(raw.tobytes())) + chunk(b"IEND", b""))
    assert np.array_equal(export.read_png(str(other)), image)
    bad = bytearray(data)
    bad[40] ^= 1
    (tmp_path / "c.png").write_bytes(bytes(bad))
    with pytest.raises(ValueError, match="CRC"):
        export.read_png(str(tmp_path / "c.png"))
    with pytest.raises(ValueError, match="uint8"):
        export.write_png(str(tmp_path / "d.png"), image.astype(np.float32))


def test_ply_round_trip(tmp_path):
    rng = np.random.default_rng(1)
    xyz = rng.standard_normal((11, 3)).astype(np.float32)
    rgb = rng.integers(0, 256, (11, 3), dtype=np.uint8)
    path = export.write_ply(str(tmp_path / "a.ply"), xyz, rgb)
    got_xyz, got_rgb = export.read_ply(path)
    assert got_xyz.dtype == np.float32 and np.array_equal(got_xyz, xyz) and np.array_equal(got_rgb, rgb)
    data = open(path, "rb").read()
    assert data.startswith(b"ply\nformat binary_little_endian 1.0\nelement vertex 11\n")
    assert len(data) - data.index(b"end_header\n") - 11 == 11 * 15
    with pytest.raises(ValueError, match="rgb"):
        export.write_ply(str(tmp_path / "b.ply"), xyz, rgb[:5])


def test_colors_for_the_five_tasks():
    import torch

    from geoformer_amd import postprocess, scene

    raw = scene.make_raw_scene(500, 3)
    N = raw.shape[0]
    rgb, ids, keep = render.colors_for("input", raw_scene=raw)
    assert rgb.dtype == torch.uint8 and rgb.shape == (N, 3) and ids is None and keep is None
    assert np.array_equal(rgb.numpy(), np.clip(np.floor((raw[:, 3:6].astype(np.float32) + 1) * 127.5), 0, 255))
    rgb, ids, keep = render.colors_for("semantic_gt", raw_scene=raw)
    unann = raw[:, 6] == -100
    assert unann.any() and np.array_equal(keep.numpy(), (~unann).astype(np.uint8)) and ids is None
    assert np.array_equal(rgb.numpy()[~unann], render.CLASS_PALETTE[raw[~unann, 6].astype(int)])
    assert len({tuple(c) for c in render.CLASS_PALETTE}) == len(render.CLASS_PALETTE) >= 20
    pal = np.arange(60, dtype=np.uint8).reshape(20, 3)
    sem = torch.arange(N, dtype=torch.int32) % 22
    rgb, _, _ = render.colors_for("semantic_pred", semantic=sem, palette=pal)
    assert np.array_equal(rgb.numpy()[:20], pal) and tuple(rgb[21].tolist()) == render.UNLABELLED_RGB
    rgb, ids, keep = render.colors_for("instance_gt", raw_scene=raw)
    assert ids.dtype == torch.int32 and np.array_equal(ids.numpy(), raw[:, 7].astype(np.int32)) and keep is not None
    inst = np.unique(raw[raw[:, 7] >= 0, 7]).astype(int)
    cols = {i: tuple(rgb.numpy()[raw[:, 7] == i][0]) for i in inst}
    assert all((rgb.numpy()[raw[:, 7] == i] == cols[i]).all() for i in inst) and len(set(cols.values())) == len(inst)
    assert (rgb.numpy()[raw[:, 7] < 0] == render.UNLABELLED_RGB).all()
    owner = (np.arange(N) % 4 - 1).astype(np.int32)
    labels = postprocess.SceneLabels(owner, owner, None)
    rgb, ids, keep = render.colors_for("instance_pred", labels=labels)
    assert np.array_equal(ids.numpy(), owner) and keep is None and (rgb.numpy()[owner < 0] == render.UNLABELLED_RGB).all()
    with pytest.raises(ValueError, match="task"):
        render.colors_for("depth", raw_scene=raw)
    with pytest.raises(ValueError, match="labels="):
        render.colors_for("instance_pred", raw_scene=raw)


def _tool(name):
    import importlib.util

    spec = importlib.util.spec_from_file_location(f"{name}_cli_render", os.path.join(ROOT, "tools", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_command_lines():
    ap = _tool("predict_scenes").build_parser()
    a = ap.parse_args(["--synthetic", "1"])
    assert (a.render, a.render_size, a.render_task) == (None, (1024, 768), "instance_pred")
    # every option from before keeps its default
    assert (a.points, a.out, a.batch_size, a.min_score, a.nms_score, a.nms, a.checkpoint, a.config) == \
        (150_000, "predictions", 4, None, None, "matrix", None, "test_geoformer_scannet.yaml")
    assert not (a.scannet or a.full_masks or a.semantic or a.panoptic or a.geometric_segments or a.no_write)
    assert (a.segments, a.split_masks, a.tile, a.halo, a.tile_max_points, a.tile_stitch, a.reps) == \
        (None, None, None, None, None, None, 3)
    a = ap.parse_args(["--render", "turntable:4", "--render-size", "320x200", "--render-task", "input", "a.npy"])
    assert (a.render, a.render_size, a.render_task) == (("turntable", 4), (320, 200), "input")
    assert ap.parse_args(["--render", "top", "a.npy"]).render == ("top", 1)
    for bad in (["--render", "side"], ["--render", "turntable:0"], ["--render-size", "320"], ["--render-task", "depth"]):
        with pytest.raises(SystemExit):
            ap.parse_args(bad + ["a.npy"])
    ap = _tool("render_scene").build_parser()
    a = ap.parse_args(["scene0011_00_inst_nostuff.npy"])
    assert (a.task, a.views, a.size, a.predictions, a.supersample, a.radius) == ("input", ("turntable", 4), (1024, 768),
                                                                                 None, 2, 2)
    a = ap.parse_args(["s.npy", "--task", "instance_pred", "--predictions", "out", "--views", "top", "--ply"])
    assert (a.task, a.predictions, a.views, a.ply) == ("instance_pred", "out", ("top", 1), True)
    assert _tool("render_trace").build_parser().parse_args([]).points == 150_000


def test_derived_binding():
    from ctypes import c_float, c_int, c_longlong, c_void_p

    from geoformer_amd import _abi

    fns = _abi.functions()
    for name in ("gf_render_camera_floats", "gf_render_max_views", "gf_render_max_side", "gf_render_max_radius",
                 "gf_render_max_supersample"):
        assert fns[name] == (c_int, [])
    assert fns["gf_render_splat"] == (c_int, [c_void_p, c_void_p, c_longlong, c_void_p, c_int, c_int, c_int, c_int,
                                              c_void_p, c_void_p])
    assert fns["gf_render_resolve"] == (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_longlong,
                                                c_void_p, c_int, c_float, c_int, c_int, c_void_p, c_void_p, c_void_p])
    assert _abi.const("GF_ABI_VERSION") == 7


def test_wrapper_argument_errors_come_before_the_library(monkeypatch):
    import torch

    from geoformer_amd import _lib

    def no_library():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "load", no_library)
    cam = render.top_down((np.zeros(3), np.ones(3)), (8, 8))
    xyz, rgb = torch.zeros((4, 3)), torch.zeros((4, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="xyz"):
        render.render(xyz, rgb, cam, (8, 8))  # not on the GPU
    with pytest.raises(ValueError, match="pixels"):
        render.render(xyz, rgb, cam, (8, render.MAX_SIDE + 1))
    with pytest.raises(ValueError, match="supersample"):
        render.render(xyz, rgb, cam, (8, 8), supersample=5)
    with pytest.raises(ValueError, match="radius"):
        render.render(xyz, rgb, cam, (8, 8), radius=17)
    with pytest.raises(ValueError, match="radius"):
        render.render(xyz, rgb, cam, (8, 8), radius=(3, 2))
    with pytest.raises(ValueError, match="no cameras"):
        render.render(xyz, rgb, [], (8, 8))
    with pytest.raises(ValueError, match="near"):
        render.render(xyz, rgb, cam._replace(kind="persp", near=0.0), (8, 8))
    with pytest.raises(RuntimeError, match="xyz"):
        render.splat(xyz, None, render.camera_table(cam), 8, 8, 0)
    with pytest.raises(RuntimeError, match="keys"):
        render.resolve(torch.zeros((1, 8, 8), dtype=torch.int64), 1, rgb)
    with pytest.raises(ValueError, match="lut"):
        render.resolve_host(np.zeros((1, 2, 2), np.uint64), 1, rgb.numpy(), shade=render.Shade((300,) * 9, 1, 0.0))
    with pytest.raises(ValueError, match="cams"):
        render.splat_host(xyz.numpy(), None, np.zeros((1, 19), np.float32), 8, 8, 0)
    with pytest.raises(ValueError, match="max_radius"):
        render.splat_host(xyz.numpy(), None, render.camera_table(cam), 8, 8, 17)
