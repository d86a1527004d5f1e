"""Host side of the point-set operators (PG_OP / pointnet2._ext / geodesic stage).

Plain functions over device tensors; every one launches a kernel of libgeoformer_hip.so on
the current stream.  The module-shaped mirrors of the reference bindings live in
``geoformer_amd.dropin``.
"""
from __future__ import annotations

import contextlib
import os
import threading

import numpy as np
import torch

from . import _abi, _lib
from ._lib import check, ptr, stream_ptr


def _f32c(t, name):
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise RuntimeError(f"{name}: expected a contiguous float32 tensor on the GPU")
    return t


def _i32c(t, name):
    if not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous()):
        raise RuntimeError(f"{name}: expected a contiguous int32 tensor on the GPU")
    return t


# ---- PG_OP ---------------------------------------------------------------------------
def voxelize_fp(feats, rules, mode=4, out=None):
    _f32c(feats, "feats"); _i32c(rules, "rules")
    M, C = rules.shape[0], feats.shape[1]
    if out is None:
        out = torch.empty((M, C), dtype=torch.float32, device=feats.device)
    check(_lib.load().gf_voxelize_fp(ptr(feats), ptr(rules), M, rules.shape[1] - 1, C, int(mode == 4), ptr(out),
                                     stream_ptr()), "gf_voxelize_fp")
    return out


def voxelize_bp(d_out, rules, mode, d_feats):
    """d_feats [N,C] must be zero-initialised by the caller (accumulated into)."""
    _f32c(d_out, "d_out"); _i32c(rules, "rules"); _f32c(d_feats, "d_feats")
    M, C = d_out.shape
    check(_lib.load().gf_voxelize_bp(ptr(d_out), ptr(rules), M, rules.shape[1] - 1, C, int(mode == 4), ptr(d_feats),
                                     stream_ptr()), "gf_voxelize_bp")
    return d_feats


# ---- pointnet2._ext --------------------------------------------------------------------
def voxelize_idx(coords, mode=4):
    """GPU voxelisation with the semantics of PG_OP.voxelize_idx: coords int64 [N,3|4] on the device ->
    (output_coords int64 [M,ncol], input_map int32 [N], output_map int32 [M,1+maxActive]).  One host read-back
    (M, maxActive)."""
    if not (coords.is_cuda and coords.dtype == torch.int64 and coords.is_contiguous() and coords.dim() == 2):
        raise RuntimeError("coords: expected a contiguous int64 [N,3|4] tensor on the GPU")
    lib = _lib.load()
    N, ncol = coords.shape
    dev = coords.device
    scratch = torch.empty(lib.gf_voxelize_idx_scratch_bytes(N) // 8 + 1, dtype=torch.int64, device=dev)
    input_map = torch.empty(N, dtype=torch.int32, device=dev)
    head = torch.empty(3, dtype=torch.int32, device=dev)
    check(lib.gf_voxelize_idx_count(ptr(coords), N, ncol, int(mode), ptr(scratch), ptr(input_map), ptr(head),
                                    stream_ptr()), "gf_voxelize_idx_count")
    M, max_active, err = head.tolist()
    if err:
        raise _lib.GeoFormerHipError("gf_voxelize_idx: a coordinate lies outside [0, 65535] (packed 16-bit key fields)")
    max_active = max(max_active, 1)
    out_coords = torch.empty((M, ncol), dtype=torch.int64, device=dev)
    out_map = torch.empty((M, max_active + 1), dtype=torch.int32, device=dev)
    check(lib.gf_voxelize_idx_fill(ptr(coords), N, ncol, int(mode), ptr(scratch), ptr(input_map), M, max_active,
                                   ptr(out_coords), ptr(out_map), stream_ptr()), "gf_voxelize_idx_fill")
    return out_coords, input_map, out_map


def gather_points(points, idx):
    _f32c(points, "points"); _i32c(idx, "idx")
    b, c, n = points.shape
    m = idx.shape[1]
    out = torch.empty((b, c, m), dtype=torch.float32, device=points.device)
    check(_lib.load().gf_gather_points(ptr(points), ptr(idx), b, c, n, m, ptr(out), stream_ptr()), "gf_gather_points")
    return out


def gather_points_grad(grad_out, idx, n):
    _f32c(grad_out, "grad_out"); _i32c(idx, "idx")
    b, c, m = grad_out.shape
    out = torch.zeros((b, c, n), dtype=torch.float32, device=grad_out.device)
    check(_lib.load().gf_gather_points_grad(ptr(grad_out), ptr(idx), b, c, n, m, ptr(out), stream_ptr()),
          "gf_gather_points_grad")
    return out


def group_points(points, idx):
    _f32c(points, "points"); _i32c(idx, "idx")
    b, c, n = points.shape
    _, npoints, nsample = idx.shape
    out = torch.empty((b, c, npoints, nsample), dtype=torch.float32, device=points.device)
    check(_lib.load().gf_group_points(ptr(points), ptr(idx), b, c, n, npoints, nsample, ptr(out), stream_ptr()),
          "gf_group_points")
    return out


def group_points_grad(grad_out, idx, n):
    _f32c(grad_out, "grad_out"); _i32c(idx, "idx")
    b, c, npoints, nsample = grad_out.shape
    out = torch.zeros((b, c, n), dtype=torch.float32, device=grad_out.device)
    check(_lib.load().gf_group_points_grad(ptr(grad_out), ptr(idx), b, c, n, npoints, nsample, ptr(out),
                                           stream_ptr()), "gf_group_points_grad")
    return out


def ball_query(new_xyz, xyz, radius, nsample, grid=None):
    """pointnet2 ball_query.  grid: use the hash-grid kernel (same rows; default: for one point set of >= 4096 points)."""
    _f32c(new_xyz, "new_xyz"); _f32c(xyz, "xyz")
    b, m, _ = new_xyz.shape
    n = xyz.shape[1]
    idx = torch.empty((b, m, nsample), dtype=torch.int32, device=xyz.device)
    lib = _lib.load()
    if grid is None:
        grid = b == 1 and n >= 4096
    if grid and b == 1 and n >= 1:
        scratch = torch.empty(lib.gf_knn_scratch_bytes(n) // 4 + 16, dtype=torch.int32, device=xyz.device)
        check(lib.gf_ball_query_grid(ptr(xyz), n, None, ptr(new_xyz), m, float(radius), nsample, ptr(scratch), 0, None,
                                     ptr(idx), stream_ptr()), "gf_ball_query_grid")
        return idx
    check(lib.gf_ball_query(ptr(new_xyz), ptr(xyz), b, n, m, float(radius), nsample, ptr(idx), stream_ptr()),
          "gf_ball_query")
    return idx


def furthest_point_sampling(xyz, m, known=None, check=False):
    """FPS indices [b,m] (int32).  known: the first picks [b,m0] of the same sequence from an earlier call with a
    smaller m -- the draw continues from there (same result as one call with m).  check: read the kernel's error word
    back after the call (one synchronisation) and raise if it is set."""
    _f32c(xyz, "xyz")
    b, n, _ = xyz.shape
    lib = _lib.load()
    idx = torch.empty((b, m), dtype=torch.int32, device=xyz.device)
    scratch = torch.empty(lib.gf_fps_scratch_bytes(b) // 8 + 1, dtype=torch.int64, device=xyz.device)
    m0 = 0
    if known is not None:
        _i32c(known, "known")
        m0 = min(int(known.shape[1]), m)
        idx[:, :m0] = known[:, :m0]
    _lib.check(lib.gf_furthest_point_sampling_resume(ptr(xyz), b, n, m, m0, ptr(idx), ptr(scratch), stream_ptr()),
               "gf_furthest_point_sampling")
    if check and b > 0 and m0 < m:  # (otherwise nothing was launched and the scratch is as allocated)
        off = (lib.gf_fps_error_flag(ptr(scratch), b) - scratch.data_ptr()) // 4
        if int(scratch.view(torch.int32)[off].item()) != 0:
            raise _lib.GeoFormerHipError("gf_furthest_point_sampling: an exchange gave up waiting for a workgroup of its "
                                         "point set (picks wrong)")
    return idx


def select_foreground(scores, cls, equal, locs, batch_idxs, feats, feat_rows=None, deferred=False):
    """Fused foreground selection (csrc/foreground.hip): points whose arg-max class is >= cls (== cls with `equal`).
    Returns (fg_idxs int64 [n], locs_ [n,3], batch_idxs_ int32 [n], feats_ [n,F], scores_ [n,C]) -- views of
    capacity-N buffers -- after ONE read-back (the count)."""
    _f32c(scores, "scores"); _f32c(locs, "locs"); _i32c(batch_idxs, "batch_idxs"); _f32c(feats, "feats")
    if feat_rows is not None:
        _i32c(feat_rows, "feat_rows")  # feats are rows of another table (voxels), read as feats[feat_rows[p]]
    N, C = scores.shape
    F = feats.shape[1]
    dev = scores.device
    lib = _lib.load()
    scratch = torch.empty(lib.gf_fg_scratch_bytes(N) // 4 + 1, dtype=torch.int32, device=dev)
    fg = torch.empty(N, dtype=torch.int64, device=dev)
    locs_o = torch.empty((N, 3), dtype=torch.float32, device=dev)
    bidx_o = torch.empty(N, dtype=torch.int32, device=dev)
    feats_o = torch.empty((N, F), dtype=torch.float32, device=dev)
    scores_o = torch.empty((N, C), dtype=torch.float32, device=dev)
    cnt = torch.empty(1, dtype=torch.int32, device=dev)
    host = PendingForeground.take_word() if deferred else None  # (pinned, set to -1: the scan kernel stores the count there)
    check(lib.gf_fg_select(ptr(scores), N, C, int(cls), int(bool(equal)), ptr(locs), ptr(batch_idxs), ptr(feats),
                           ptr(feat_rows), F,
                           ptr(scratch), ptr(fg), ptr(locs_o), ptr(bidx_o), ptr(feats_o), ptr(scores_o), ptr(cnt),
                           ptr(host), stream_ptr()), "gf_fg_select")
    if not deferred:
        n = int(cnt.item())
        return fg[:n], locs_o[:n], bidx_o[:n], feats_o[:n], scores_o[:n]
    return PendingForeground(cnt, (fg, locs_o, bidx_o, feats_o, scores_o), host)


class PendingForeground:
    """select_foreground(..., deferred=True): the launches are queued; ``wait()`` returns the count, ``views()`` the five
    slices.  The count reaches the host through a pinned word the scan kernel stores it to (gf_fg_select's h_count): no copy
    command, no event, and BEFORE the gathers of the outputs have run -- the host polls the word natively
    (gf_host_wait_word, interpreter lock released) and starts on what follows the count while the device finishes the
    selection.  (The staggered serving loop queues a scene's selection with its backbone and comes back for the count after
    it has queued the next scene's first launches.)"""

    _pinned = []
    _lock = threading.Lock()

    @staticmethod
    def take_word():
        with PendingForeground._lock:
            host = PendingForeground._pinned.pop() if PendingForeground._pinned else None
        if host is None:
            host = torch.zeros(1, dtype=torch.int32).pin_memory()
        host[0] = -1
        return host

    def __init__(self, cnt, bufs, host=None):
        self.polled = host is not None
        if host is None:  # (no polled word: the count as an asynchronous copy behind the selection, waited for by event)
            host = PendingForeground.take_word()
            host.copy_(cnt, non_blocking=True)
        self.host, self.bufs, self.cnt = host, bufs, cnt
        self.done = torch.cuda.Event()  # behind the whole selection (what other streams wait for before they read it)
        self.done.record()

    def wait(self):
        """Block until the count is on the host; returns it.  (``views()`` afterwards: the five slices -- a caller with
        something urgent to launch from the count alone does that in between.)"""
        import time

        t = time.perf_counter()
        if self.polled:
            n = int(_lib.load().gf_host_wait_word(self.host.data_ptr(), -1, 5_000_000))
            if n < 0:  # (five seconds without the store: the event and a plain read-back)
                self.done.synchronize()
                n = int(self.cnt.item())
        else:
            self.done.synchronize()
            n = int(self.host[0])
        _lib.host_wait_s[0] += time.perf_counter() - t
        self.n = n
        with PendingForeground._lock:
            PendingForeground._pinned.append(self.host)
        self.host = None
        return self.n

    def views(self):
        return tuple(b[:self.n] for b in self.bufs)

    def get(self):
        self.wait()
        return self.views()


_LEGACY_STATE = {}  # id(bit generator) -> (generator, address of its {uint32 key[624]; int pos}) or (generator, None)


def _legacy_state():
    """numpy's global legacy generator in place: (address of its MT19937 state -- ``uint32 key[624]; int pos``,
    numpy/random/src/mt19937/mt19937.h -- , the generator's lock), or None when the global RandomState runs on another
    bit generator or the layout does not check out against ``get_state()`` (then: the get_state / set_state route).
    ``np.random.get_state()`` + ``set_state()`` are 20-40 us each -- on the forward's critical path, once per scene."""
    import ctypes

    import numpy as np

    bg = np.random.mtrand._rand._bit_generator
    hit = _LEGACY_STATE.get(id(bg))
    if hit is None or hit[0] is not bg:
        addr = None
        if type(bg).__name__ == "MT19937":
            try:
                a = int(bg.ctypes.state_address)
                st = np.random.get_state()
                key = np.ctypeslib.as_array((ctypes.c_uint32 * 624).from_address(a))
                if st[0] == "MT19937" and int(ctypes.c_int.from_address(a + 2496).value) == int(st[2]) and \
                        bool((key == np.asarray(st[1], dtype=np.uint32)).all()):
                    addr = a
            except Exception:  # noqa: BLE001  (an interface this numpy does not have: the portable route)
                addr = None
        _LEGACY_STATE.clear()
        hit = _LEGACY_STATE[id(bg)] = (bg, addr)
    return None if hit[1] is None else (hit[1], bg.lock)


def legacy_prefetch(nwords):
    """Draw the next `nwords` outputs of numpy's global legacy generator ahead (into a per-thread native buffer, the
    generator itself untouched): a legacy_choice that starts from the same state takes its words from there."""
    import ctypes

    import numpy as np

    direct = _legacy_state()
    if direct is not None:
        addr, lock = direct
        with lock:
            check(_lib.load().gf_host_legacy_prefetch(addr, int(ctypes.c_int.from_address(addr + 2496).value), int(nwords)),
                  "gf_host_legacy_prefetch")
        return
    st = np.random.get_state()
    if st[0] != "MT19937":
        return
    key = np.ascontiguousarray(st[1], dtype=np.uint32)
    check(_lib.load().gf_host_legacy_prefetch(key.ctypes.data, int(st[2]), int(nwords)), "gf_host_legacy_prefetch")


_DRAW_PINS = {}  # (device index, stream) -> pinned int32 buffer of the fused draw (grow-only)


def draw_sample_buffers(kmax, n_cap, device, fps_m=0):
    """Device outputs and the pinned staging buffer of ``draw_sample`` for at most `kmax` drawn indices out of at most
    `n_cap` points, allocated ahead (the caller does this while it waits for the count the draw depends on).
    fps_m > 0: also the outputs of a first furthest-point-sampling launch of fps_m picks over the drawn points."""
    key = (device.index, stream_ptr())
    pin = _DRAW_PINS.get(key)
    if pin is None or pin.numel() < max(n_cap, kmax):
        pin = _DRAW_PINS[key] = torch.empty(max(n_cap + n_cap // 4, kmax, 65536), dtype=torch.int32).pin_memory()
    bufs = {"pin": pin, "idx32": torch.empty(kmax, dtype=torch.int32, device=device),
            "idx64": torch.empty(kmax, dtype=torch.int64, device=device),
            "xyz": torch.empty((1, kmax, 3), dtype=torch.float32, device=device), "kmax": kmax, "fps_m": 0}
    if fps_m > 0:
        bufs["fps_m"] = int(fps_m)
        bufs["fps_idx"] = torch.empty((1, int(fps_m)), dtype=torch.int32, device=device)
        bufs["fps_scratch"] = torch.empty(_lib.load().gf_fps_scratch_bytes(1) // 8 + 1, dtype=torch.int64, device=device)
    return bufs


def draw_sample(n, k, xyz_src, bufs):
    """The reference's per-scene draw ``np.random.choice(n, k, replace=False)`` (geoformer.py:575-577) and what follows it
    -- upload of the indices, gather of the drawn points -- as ONE native call (gf_host_draw_sample, csrc/host_draw.hip):
    returns (sampling_indices int64 [k], xyz [1,k,3]) on the device, queued on the current stream; numpy's global
    generator advances exactly as by the draw.  None when the generator cannot be driven in place (the caller then takes
    legacy_choice's route).  xyz_src: [>= n, 3] fp32 contiguous.  With buffers made for a first sampling launch
    (``fps_m``) and k >= fps_m that launch is queued in the same call: a third result, its picks int32 [1, fps_m]."""
    n, k = int(n), int(k)
    direct = _legacy_state() if 1 <= k <= n <= 0x7fffffff and k <= bufs["kmax"] else None
    if direct is None:
        return None
    _f32c(xyz_src, "xyz_src")
    addr, lock = direct
    pin = bufs["pin"]
    fps_m = bufs["fps_m"] if 0 < bufs["fps_m"] <= k else 0
    with lock:
        check(_lib.load().gf_host_draw_sample(addr, addr + 2496, n, k, pin.data_ptr(), pin.numel(), ptr(bufs["idx32"]),
                                              ptr(bufs["idx64"]), ptr(xyz_src), ptr(bufs["xyz"]), fps_m,
                                              ptr(bufs["fps_idx"]) if fps_m else None,
                                              ptr(bufs["fps_scratch"]) if fps_m else None, stream_ptr()),
              "gf_host_draw_sample")
    if fps_m:
        return bufs["idx64"][:k], bufs["xyz"][:, :k], bufs["fps_idx"]
    return bufs["idx64"][:k], bufs["xyz"][:, :k]


def legacy_choice(n, k, out=None):
    """``np.random.choice(n, k, replace=False)`` on numpy's global legacy generator -- same values, same generator
    state afterwards -- through the native restatement (csrc/host_draw.hip; about half the host time).
    out: optional int64 numpy array of at least k entries to draw into (e.g. the view of a pinned tensor, so that the
    upload that follows is an asynchronous copy); the first k entries are returned."""
    import ctypes

    import numpy as np

    n, k = int(n), int(k)
    direct = _legacy_state() if 1 <= k <= n <= 0x7fffffff else None
    if direct is not None:  # the generator's state advanced in place, under its lock
        addr, lock = direct
        if out is None or out.dtype != np.int64 or out.size < k or not out.flags.c_contiguous:
            out = np.empty(k, dtype=np.int64)
        with lock:
            check(_lib.load().gf_host_legacy_choice(addr, addr + 2496, n, k, out.ctypes.data), "gf_host_legacy_choice")
        return out[:k]
    st = np.random.get_state()
    if st[0] != "MT19937" or not (1 <= k <= n <= 0x7fffffff):
        return np.random.choice(n, k, replace=False)  # numpy's own argument errors / exotic sizes
    key = np.ascontiguousarray(st[1], dtype=np.uint32).copy()
    pos = ctypes.c_int32(int(st[2]))
    if out is None or out.dtype != np.int64 or out.size < k or not out.flags.c_contiguous:
        out = np.empty(k, dtype=np.int64)
    check(_lib.load().gf_host_legacy_choice(key.ctypes.data, ctypes.addressof(pos), n, k, out.ctypes.data),
          "gf_host_legacy_choice")
    np.random.set_state((st[0], key, int(pos.value), st[3], st[4]))
    return out[:k]


# ---- geodesic stage --------------------------------------------------------------------
def knn_radius(xyz, k, radius, sqrt_out=True, check_overflow=False, return_flag=False):
    """Radius-limited kNN graph of one scene.  Returns D [n,k] fp32, I [n,k] int32, deg [n] int32
    (+ with return_flag the kernel's device-side truncation flag, int32 [1], for a caller that folds it into a
    read-back it makes anyway; check_overflow reads it here and raises)."""
    _f32c(xyz, "xyz")
    n = xyz.shape[0]
    lib = _lib.load()
    dev = xyz.device
    D = torch.empty((n, k), dtype=torch.float32, device=dev)
    I = torch.empty((n, k), dtype=torch.int32, device=dev)
    deg = torch.empty(n, dtype=torch.int32, device=dev)
    scratch = torch.empty(lib.gf_knn_scratch_bytes(n) // 4 + 16, dtype=torch.int32, device=dev)
    check(lib.gf_knn_radius(ptr(xyz), n, k, float(radius), int(sqrt_out), ptr(D), ptr(I), ptr(deg), ptr(scratch),
                            stream_ptr()), "gf_knn_radius")
    if check_overflow:
        off = (lib.gf_knn_error_flag(ptr(scratch), n) - scratch.data_ptr()) // 4
        if int(scratch[off].item()) != 0:
            raise _lib.GeoFormerHipError("gf_knn_radius: a point has more in-radius neighbours than the kernel's "
                                         "candidate list holds (rows truncated)")
    if return_flag:
        off = (lib.gf_knn_error_flag(ptr(scratch), n) - scratch.data_ptr()) // 4
        return D, I, deg, scratch[off:off + 1]
    return D, I, deg


_SCRATCH = {}


def scratch(name, numel, dtype, device):
    """Grow-only scratch tensor per (device, current stream, name): PURE scratch of one native call (workspaces the
    kernels fill and nobody reads afterwards), reused by the next call on the same stream, which stream order places
    behind this one.  The big per-scene workspaces (U-Net workspace, BFS keys and queues: ~0.8 GB for a 150k-point
    scene) then never go through the framework's caching allocator, whose blocks get split by scenes of other sizes
    until a larger scene needs a fresh hipMalloc in the middle of a forward (20-30 ms; bench.py secondary.fresh_scenes)."""
    dev = torch.device(device)
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), torch.cuda.current_stream(dev).cuda_stream,
           name, dtype)
    t = _SCRATCH.get(key)
    if t is None or t.numel() < numel:
        _SCRATCH[key] = None  # (drop the old block before asking for the new one)
        t = _SCRATCH[key] = torch.empty(int(numel * 1.25) + 64, dtype=dtype, device=dev)
    return t[:numel]


def release_scratch(device=None):
    """Drop the grow-only scratch blocks (of one device, or of all): ~0.8 GB per stream that ran a 150k-point scene
    (U-Net workspace, BFS keys and queues, mask-head split).  Nothing else frees them -- `torch.cuda.empty_cache()` does
    not see tensors that are still referenced.  Called by `invalidate_fused_caches()` of the models and by a serving
    loop's teardown; the caller makes sure no kernel that uses them is still queued (synchronise first)."""
    if device is not None:
        dev = torch.device(device)
        idx = dev.index if dev.index is not None else torch.cuda.current_device()
    for key in list(_SCRATCH):
        if device is None or key[0] == idx:
            del _SCRATCH[key]


def scratch_bytes():
    """Bytes the scratch blocks hold right now (all devices and streams)."""
    return sum(t.numel() * t.element_size() for t in _SCRATCH.values() if t is not None)


def geodesic_bfs(D, I, deg, src, radius, max_step, wg_threads=1024):
    """geo [nq,n] fp32 for the sources `src` (int32 [nq]) over the kNN rows D/I (column 0 skipped).
    wg_threads: 1024 = one query per compute unit; 256 / 512 = several per unit (to run beside another kernel)."""
    _f32c(D, "D"); _i32c(I, "I"); _i32c(src, "src")
    n, K = D.shape
    nq = src.shape[0]
    dev = D.device
    geo = torch.empty((nq, n), dtype=torch.float32, device=dev)
    lib = _lib.load()
    keys = scratch("bfs_keys", nq * n, torch.int64, dev)
    qwords = int(lib.gf_geodesic_bfs_queue_words(n))
    queues = scratch("bfs_queues", nq * qwords, torch.int32, dev)
    check(lib.gf_geodesic_bfs_cfg(ptr(D), ptr(I), ptr(deg), n, K, ptr(src), nq, float(radius), int(max_step),
                                          ptr(geo), ptr(keys), ptr(queues), qwords, int(wg_threads), stream_ptr()),
          "gf_geodesic_bfs")
    return geo


# ---- fused heads -------------------------------------------------------------------------
def _mask_head_split_ws(N, device, split):
    """Scratch for the features' three bf16 pieces (gf_mask_head_episodes: fp32-accurate products on the bf16 matrix
    pipe); split=False keeps the fp32 MFMA."""
    if not split:
        return None
    return scratch("mask_head_split", _lib.load().gf_mask_head_split_bytes(N) // 8 + 1, torch.int64, device)


def mask_head(feat, coords, geo, qxyz, sqrt_max_geo, w1, b1, w2, b2, split=True):
    """Fused dynamic-conv mask head: logits [nq,N].  feat [N,16], coords [N,3], geo [nq,N] or None,
    qxyz [nq,3], sqrt_max_geo [nq] or None, w1 [nq,16,19], b1 [nq,16], w2 [nq,16], b2 [nq]."""
    for t, name in ((feat, "feat"), (coords, "coords"), (qxyz, "qxyz"), (w1, "w1"), (b1, "b1"), (w2, "w2"), (b2, "b2")):
        _f32c(t, name)
    N, C = feat.shape
    nq = qxyz.shape[0]
    out = torch.empty((nq, N), dtype=torch.float32, device=feat.device)
    check(_lib.load().gf_mask_head_episodes(ptr(feat), ptr(coords), ptr(geo), ptr(qxyz), ptr(sqrt_max_geo), ptr(w1), ptr(b1),
                                            ptr(w2), ptr(b2), 0, N, nq, 1, C, ptr(_mask_head_split_ws(N, feat.device, split)),
                                            ptr(out), stream_ptr()), "gf_mask_head")
    return out


def mask_head_packed(feat, coords, geo, qxyz, sqrt_max_geo, params, split=True):
    """mask_head with the per-query parameters read in place from the controller's output params [nq, 16*19+16+16+1]
    (column blocks w1 | w2 | b1 | b2, parse_dynamic_params of geoformer.py:264-284)."""
    return mask_head_episodes(feat, coords, geo, qxyz, sqrt_max_geo, params.unsqueeze(0), split=split)[0]


def mask_head_episodes(feat, coords, geo, qxyz, sqrt_max_geo, params, split=True):
    """E episodes over one scene in ONE launch (gf_mask_head_episodes): params [E, nq, 337] -> logits [E, nq, N];
    feat / coords / geo [nq,N] / qxyz [nq,3] / sqrt_max_geo [nq] are the scene's and shared by the episodes."""
    for t, name in ((feat, "feat"), (coords, "coords"), (qxyz, "qxyz"), (params, "params")):
        _f32c(t, name)
    N, C = feat.shape
    E, nq, ld = params.shape
    if ld != C * (C + 3) + C + C + 1 or qxyz.shape[0] != nq:
        raise RuntimeError(f"mask_head_episodes: params {tuple(params.shape)} for {qxyz.shape[0]} queries, C={C}")
    base = params.data_ptr()
    o_w2, o_b1, o_b2 = C * (C + 3), C * (C + 3) + C, C * (C + 3) + 2 * C
    out = torch.empty((E, nq, N), dtype=torch.float32, device=feat.device)
    check(_lib.load().gf_mask_head_episodes(ptr(feat), ptr(coords), ptr(geo), ptr(qxyz), ptr(sqrt_max_geo), base,
                                            base + 4 * o_b1, base + 4 * o_w2, base + 4 * o_b2, ld, N, nq, E, C,
                                            ptr(_mask_head_split_ws(N, feat.device, split)), ptr(out), stream_ptr()),
          "gf_mask_head_episodes")
    return out


class _MaskHeadFn(torch.autograd.Function):
    """Fused mask head with a fused, recompute-based backward (csrc/mask_head.hip): gradients for the mask features
    and the generated per-query parameters; coordinates and geodesic distances are data."""

    @staticmethod
    def forward(ctx, feat, params, coords, geo, qxyz, sqrt_max_geo):
        ctx.save_for_backward(feat, params, coords, geo, qxyz, sqrt_max_geo)
        return mask_head_packed(feat, coords, geo, qxyz, sqrt_max_geo, params)

    @staticmethod
    def backward(ctx, gout):
        feat, params, coords, geo, qxyz, mx = ctx.saved_tensors
        N, C = feat.shape
        nq, ld = params.shape
        lib = _lib.load()
        dparams = torch.empty_like(params)
        dfeat = torch.zeros_like(feat)
        scratch = torch.empty(lib.gf_mask_head_bwd_scratch_floats(N, nq), dtype=torch.float32, device=feat.device)
        base = params.data_ptr()
        o_w2, o_b1 = C * (C + 3), C * (C + 3) + C
        check(lib.gf_mask_head_bwd(ptr(feat), ptr(coords), ptr(geo), ptr(qxyz), ptr(mx), base, base + 4 * o_b1,
                                   base + 4 * o_w2, ptr(gout.contiguous()), ld, N, nq, C, ptr(dparams), ptr(dfeat),
                                   ptr(scratch), stream_ptr()), "gf_mask_head_bwd")
        return dfeat, dparams, None, None, None, None


class _MaskHeadEpisodesFn(torch.autograd.Function):
    """E parameter sets over one scene (the decoder layers of a training step): one forward launch and one backward
    triple for all of them; the features' gradient is summed over the episodes inside the kernel."""

    @staticmethod
    def forward(ctx, feat, params, coords, geo, qxyz, sqrt_max_geo):
        ctx.save_for_backward(feat, params, coords, geo, qxyz, sqrt_max_geo)
        return mask_head_episodes(feat, coords, geo, qxyz, sqrt_max_geo, params)

    @staticmethod
    def backward(ctx, gout):
        feat, params, coords, geo, qxyz, mx = ctx.saved_tensors
        N, C = feat.shape
        E, nq, ld = params.shape
        lib = _lib.load()
        dparams = torch.empty_like(params)
        dfeat = torch.zeros_like(feat)
        scratch = torch.empty(lib.gf_mask_head_bwd_scratch_floats(N, E * nq), dtype=torch.float32, device=feat.device)
        base = params.data_ptr()
        o_w2, o_b1 = C * (C + 3), C * (C + 3) + C
        check(lib.gf_mask_head_bwd_episodes(ptr(feat), ptr(coords), ptr(geo), ptr(qxyz), ptr(mx), base, base + 4 * o_b1,
                                            base + 4 * o_w2, ptr(gout.contiguous()), ld, N, nq, E, C, ptr(dparams),
                                            ptr(dfeat), ptr(scratch), stream_ptr()), "gf_mask_head_bwd_episodes")
        return dfeat, dparams, None, None, None, None


def mask_head_train_episodes(feat, params, coords, geo, qxyz, sqrt_max_geo):
    """logits [E,nq,N] with autograd through feat [N,16] and params [E,nq,337]."""
    for t, name in ((feat, "feat"), (coords, "coords"), (qxyz, "qxyz"), (params, "params")):
        _f32c(t, name)
    return _MaskHeadEpisodesFn.apply(feat, params, coords, geo, qxyz, sqrt_max_geo)


def mask_head_train(feat, params, coords, geo, qxyz, sqrt_max_geo):
    """logits [nq,N] with autograd through feat [N,16] and params [nq,337] (fused forward AND backward)."""
    for t, name in ((feat, "feat"), (coords, "coords"), (qxyz, "qxyz"), (params, "params")):
        _f32c(t, name)
    return _MaskHeadFn.apply(feat, params, coords, geo, qxyz, sqrt_max_geo)


class PointwiseChain:
    """Folded parameters of a Conv1d(k=1)/Linear + eval BatchNorm1d + ReLU stack for gf_pointwise_mlp."""

    def __init__(self, modules):
        import ctypes

        layers = []  # [W, scale, shift, relu]
        for m in modules:
            name = type(m).__name__
            if isinstance(m, (torch.nn.Linear, torch.nn.Conv1d, torch.nn.Conv2d)):
                W = m.weight.detach()
                W = W.reshape(W.shape[0], W.shape[1]).float().contiguous()
                bias = m.bias.detach().float() if m.bias is not None else torch.zeros(W.shape[0], device=W.device)
                layers.append([W, torch.ones_like(bias), bias.clone(), 0])
            elif isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                if m.training:
                    raise RuntimeError("PointwiseChain folds eval-mode BatchNorm only")
                s = (m.weight / torch.sqrt(m.running_var + m.eps)).detach().float()
                layers[-1][2] = (layers[-1][2] - m.running_mean.detach()) * s + m.bias.detach()
                layers[-1][1] = layers[-1][1] * s
            elif isinstance(m, torch.nn.ReLU):
                layers[-1][3] = 1
            elif isinstance(m, (torch.nn.Identity, torch.nn.Dropout)):
                continue
            else:
                raise RuntimeError(f"PointwiseChain: unsupported module {name}")
        self.tensors = [[l[0], l[1].contiguous(), l[2].contiguous()] for l in layers]
        n = len(layers)
        self.n = n
        self.channels = [layers[0][0].shape[1]] + [l[0].shape[0] for l in layers]
        mk = lambda k: (ctypes.c_void_p * n)(*[t[k].data_ptr() for t in self.tensors])  # noqa: E731
        self.W, self.scale, self.shift = mk(0), mk(1), mk(2)
        self.ch = (ctypes.c_int * (n + 1))(*self.channels)
        self.relu = (ctypes.c_int * n)(*[l[3] for l in layers])

    @staticmethod
    def supported(modules):
        ch = []
        for m in modules:
            if isinstance(m, (torch.nn.Linear, torch.nn.Conv1d)):
                if isinstance(m, torch.nn.Conv1d) and (m.kernel_size != (1,) or m.groups != 1 or m.stride != (1,)):
                    return False
                ch.append((m.weight.shape[1], m.weight.shape[0]))
        if not 1 <= len(ch) <= 4:
            return False
        ok = all(ci % 16 == 0 and 16 <= ci <= 64 for ci, _ in ch) and all(co % 16 == 0 and co <= 64 for _, co in ch[:-1])
        return ok and 1 <= ch[-1][1] <= 64


def pointwise_mlp(x, chain, rows=None):
    """Fused per-point MLP chain over the rows of x [N, C0] -> [N, C_last] (include/geoformer_hip.h); with
    rows (int32 [N]) over x[rows] without materialising the gather."""
    _f32c(x, "x")
    N = x.shape[0]
    if rows is not None:
        _i32c(rows, "rows")
        N = rows.shape[0]
    if x.shape[1] != chain.channels[0]:
        raise RuntimeError(f"pointwise_mlp: x has {x.shape[1]} channels, the chain expects {chain.channels[0]}")
    out = torch.empty((N, chain.channels[-1]), dtype=torch.float32, device=x.device)
    check(_lib.load().gf_pointwise_mlp_rows(ptr(x), ptr(rows), N, chain.n, chain.W, chain.scale, chain.shift, chain.ch,
                                            chain.relu, ptr(out), stream_ptr()), "gf_pointwise_mlp")
    return out


def group_mlp_max(grouped, chain):
    """Fused SharedMLP + max over the samples: grouped [B,C0,npoint,nsample] -> [B,C_last,npoint]."""
    _f32c(grouped, "grouped")
    B, c0, npnt, ns = grouped.shape
    if c0 != chain.channels[0]:
        raise RuntimeError(f"group_mlp_max: grouped has {c0} channels, the chain expects {chain.channels[0]}")
    out = torch.empty((B, chain.channels[-1], npnt), dtype=torch.float32, device=grouped.device)
    check(_lib.load().gf_group_mlp_max(ptr(grouped), B, npnt, ns, chain.n, chain.W, chain.scale, chain.shift, chain.ch,
                                       chain.relu, ptr(out), stream_ptr()), "gf_group_mlp_max")
    return out


def point_grid_build(xyz, radius):
    """Hash grid of one point set [1,n,3] with cells of `radius` for the grid ball query (returns the scratch tensor
    to hand to sa_group_mlp_max(grid=...)); runs on the current stream."""
    _f32c(xyz, "xyz")
    n = xyz.shape[1]
    lib = _lib.load()
    scratch = torch.empty(lib.gf_knn_scratch_bytes(n) // 4 + 16, dtype=torch.int32, device=xyz.device)
    check(lib.gf_point_grid_build(ptr(xyz), n, float(radius), ptr(scratch), stream_ptr()), "gf_point_grid_build")
    return scratch


def sa_group_mlp_max(xyz, feats, inds, radius, nsample, use_xyz, normalize_xyz, chain, grid=None):
    """Set-abstraction stage for given sample indices, fused: returns (new_xyz [B,np,3], idx [B,np,ns] int32,
    pooled [B,C_last,np]).  xyz [B,n,3], feats [B,C,n] (or None), inds int32 [B,np]."""
    _f32c(xyz, "xyz"); _i32c(inds, "inds")
    B, n, _ = xyz.shape
    C = 0
    if feats is not None:
        _f32c(feats, "feats")
        C = feats.shape[1]
    npnt = inds.shape[1]
    dev = xyz.device
    new_xyz = torch.empty((B, npnt, 3), dtype=torch.float32, device=dev)
    idx = torch.empty((B, npnt, nsample), dtype=torch.int32, device=dev)
    out = torch.empty((B, chain.channels[-1], npnt), dtype=torch.float32, device=dev)
    lib = _lib.load()
    scratch, ready = grid, grid is not None
    if scratch is None and B == 1 and n >= 4096:  # hash grid for the ball query, built here
        scratch = torch.empty(lib.gf_knn_scratch_bytes(n) // 4 + 16, dtype=torch.int32, device=dev)
    check(lib.gf_sa_group_mlp_max(ptr(xyz), ptr(feats) if feats is not None else None, ptr(inds), B, n, C, npnt,
                                  float(radius), int(nsample), int(bool(use_xyz)), int(bool(normalize_xyz)),
                                  chain.n, chain.W, chain.scale, chain.shift, chain.ch, chain.relu,
                                  ptr(new_xyz), ptr(idx), ptr(out), ptr(scratch), int(ready), stream_ptr()),
          "gf_sa_group_mlp_max")
    return new_xyz, idx, out


def decoder_stage_tables(layer, final_norm):
    """(post, pre) device-pointer tables of one decoder layer for gf_decoder_token_stage (header order)."""
    import ctypes

    sa = layer.self_attn
    post = [layer.out_mlp[0].weight, layer.out_mlp[0].bias, layer.norm3.weight, layer.norm3.bias, layer.linear1.weight,
            layer.linear1.bias, layer.linear2.weight, layer.linear2.bias, final_norm.weight, final_norm.bias]
    pre = [layer.norm1.weight, layer.norm1.bias, sa.in_proj_weight, sa.in_proj_bias, sa.out_proj.weight,
           sa.out_proj.bias, layer.norm2.weight, layer.norm2.bias, layer.attn_mlp[0].weight, layer.attn_mlp[0].bias]
    for t in post + pre:
        _f32c(t.data, "decoder parameter")
    mk = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])  # noqa: E731
    return mk(post), mk(pre)


def decoder_stage_tensors(layer, final_norm):
    """(pre, post) parameter lists of one decoder layer in gf_decoder_token_stage's table order."""
    sa = layer.self_attn
    pre = [layer.norm1.weight, layer.norm1.bias, sa.in_proj_weight, sa.in_proj_bias, sa.out_proj.weight,
           sa.out_proj.bias, layer.norm2.weight, layer.norm2.bias, layer.attn_mlp[0].weight, layer.attn_mlp[0].bias]
    post = [layer.out_mlp[0].weight, layer.out_mlp[0].bias, layer.norm3.weight, layer.norm3.bias, layer.linear1.weight,
            layer.linear1.bias, layer.linear2.weight, layer.linear2.bias, final_norm.weight, final_norm.bias]
    return pre, post


def _ptr_table(ts):
    import ctypes

    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _split_grads(grads, params):
    outs, o = [], 0
    for t in params:
        outs.append(grads[o:o + t.numel()].view(t.shape))
        o += t.numel()
    assert o == grads.numel()
    return outs


class _DecoderPreTrainFn(torch.autograd.Function):
    """norm1 -> self-attention -> residual -> norm2 -> query half of the cross-attention's first linear, with the layer's
    dropouts: forward and backward in csrc/decoder_layer_train.hip.  x, qpos [B,T,64] -> (t2n, q1)."""

    @staticmethod
    def forward(ctx, x, qpos, layer, p, seed, *params):
        lib = _lib.load()
        B, T, _ = x.shape
        x, qpos = _f32c(x.contiguous(), "x"), _f32c(qpos.contiguous(), "qpos")
        params = [_f32c(t.detach().contiguous(), "decoder parameter") for t in params]
        t2n, q1 = torch.empty_like(x), torch.empty_like(x)
        save = torch.empty(lib.gf_decoder_pre_train_save_bytes(T, B) // 4, dtype=torch.float32, device=x.device)
        check(lib.gf_decoder_pre_train_fwd(ptr(x), ptr(qpos), T, B, _ptr_table(params), float(p), int(seed), int(layer),
                                           ptr(save), ptr(t2n), ptr(q1), stream_ptr()), "gf_decoder_pre_train_fwd")
        ctx.save_for_backward(x, qpos, t2n, save, *params)
        ctx.cfg = (int(layer), float(p), int(seed))
        ctx.set_materialize_grads(False)
        return t2n, q1

    @staticmethod
    def backward(ctx, d_t2n, d_q1):
        lib = _lib.load()
        x, qpos, t2n, save, *params = ctx.saved_tensors
        layer, p, seed = ctx.cfg
        B, T, _ = x.shape
        if d_t2n is None and d_q1 is None:
            return (None,) * (5 + len(params))
        d_t2n = None if d_t2n is None else _f32c(d_t2n.contiguous(), "d_t2n")
        d_q1 = None if d_q1 is None else _f32c(d_q1.contiguous(), "d_q1")
        work = torch.empty(lib.gf_decoder_pre_train_work_bytes(T, B) // 4, dtype=torch.float32, device=x.device)
        grads = torch.empty(lib.gf_decoder_pre_grad_floats(), dtype=torch.float32, device=x.device)
        dx, dqpos = torch.empty_like(x), torch.empty_like(x)
        check(lib.gf_decoder_pre_train_bwd(ptr(x), ptr(qpos), ptr(t2n), ptr(d_t2n), ptr(d_q1), T, B, _ptr_table(params), p,
                                           seed, layer, ptr(save), ptr(work), ptr(dx), ptr(dqpos), ptr(grads),
                                           stream_ptr()), "gf_decoder_pre_train_bwd")
        return (dx, dqpos, None, None, None) + tuple(_split_grads(grads, params))


class _DecoderPostTrainFn(torch.autograd.Function):
    """out_mlp -> residual with the normed query -> norm3 -> FFN -> residual -> decoder.norm, with the layer's dropouts.
    ca, t2n [B,T,64] -> (x3, inter)."""

    @staticmethod
    def forward(ctx, ca, t2n, layer, p, seed, *params):
        lib = _lib.load()
        B, T, _ = ca.shape
        ca, t2n = _f32c(ca.contiguous(), "ca"), _f32c(t2n.contiguous(), "t2n")
        params = [_f32c(t.detach().contiguous(), "decoder parameter") for t in params]
        ff = params[4].shape[0]
        x3, inter = torch.empty_like(ca), torch.empty_like(ca)
        save = torch.empty(lib.gf_decoder_post_train_save_bytes(T, B, ff) // 4, dtype=torch.float32, device=ca.device)
        check(lib.gf_decoder_post_train_fwd(ptr(ca), ptr(t2n), T, B, ff, _ptr_table(params), float(p), int(seed), int(layer),
                                            ptr(save), ptr(x3), ptr(inter), stream_ptr()), "gf_decoder_post_train_fwd")
        ctx.save_for_backward(ca, x3, save, *params)
        ctx.cfg = (int(layer), float(p), int(seed), ff)
        ctx.set_materialize_grads(False)
        return x3, inter

    @staticmethod
    def backward(ctx, d_x3, d_inter):
        lib = _lib.load()
        ca, x3, save, *params = ctx.saved_tensors
        layer, p, seed, ff = ctx.cfg
        B, T, _ = ca.shape
        if d_x3 is None and d_inter is None:
            return (None,) * (5 + len(params))
        d_x3 = None if d_x3 is None else _f32c(d_x3.contiguous(), "d_x3")
        d_inter = None if d_inter is None else _f32c(d_inter.contiguous(), "d_inter")
        work = torch.empty(lib.gf_decoder_post_train_work_bytes(T, B, ff) // 4, dtype=torch.float32, device=ca.device)
        grads = torch.empty(lib.gf_decoder_post_grad_floats(ff), dtype=torch.float32, device=ca.device)
        d_ca, d_t2n = torch.empty_like(ca), torch.empty_like(ca)
        check(lib.gf_decoder_post_train_bwd(ptr(ca), ptr(x3), ptr(d_x3), ptr(d_inter), T, B, ff, _ptr_table(params), p, seed,
                                            layer, ptr(save), ptr(work), ptr(d_ca), ptr(d_t2n), ptr(grads), stream_ptr()),
              "gf_decoder_post_train_bwd")
        return (d_ca, d_t2n, None, None, None) + tuple(_split_grads(grads, params))


def decoder_pre_train(x, qpos, layer_index, p, seed, pre_params):
    return _DecoderPreTrainFn.apply(x, qpos, layer_index, p, seed, *pre_params)


def decoder_post_train(ca, t2n, layer_index, p, seed, post_params):
    return _DecoderPostTrainFn.apply(ca, t2n, layer_index, p, seed, *post_params)


def decoder_token_stage(attn_out, tgt_in, query_pos, nq, B, nhead, ff, post, pre, state, inter_out, q1_out):
    """One fused token-side stage between two cross-attentions (include/geoformer_hip.h)."""
    check(_lib.load().gf_decoder_token_stage(ptr(attn_out), ptr(tgt_in), ptr(query_pos), nq, B, 64, nhead, ff, post,
                                             pre, ptr(state), ptr(inter_out), ptr(q1_out), stream_ptr()),
          "gf_decoder_token_stage")


def decoder_token_state(nq, B, device):
    return torch.empty(_lib.load().gf_decoder_token_state_bytes(nq, B) // 4, dtype=torch.float32, device=device)


def proposal_stats(mask_logits, cls_logits, sem_prob, logit_thresh, score_thresh, npoint_thresh, min_class=4,
                   class_major=False):
    """Fused statistics of generate_proposal: (cls_pred i32[nq], npoints i32[nq], scores f32[nq], final i32[nq]).
    sem_prob [N,ncls] is handed to the kernel class-major (one coalesced row per predicted class); pass it as
    [ncls,N] with class_major=True when the caller already has that copy."""
    _f32c(mask_logits, "mask_logits"), _f32c(cls_logits, "cls_logits")
    nq, N = mask_logits.shape
    ncls = cls_logits.shape[1]
    if sem_prob.shape != ((ncls, N) if class_major else (N, ncls)):
        raise RuntimeError(f"sem_prob must be [{N},{ncls}] ([{ncls},{N}] class-major), got {tuple(sem_prob.shape)}")
    sem_prob = _f32c(sem_prob if class_major else sem_prob.t().contiguous(), "sem_prob")
    ints = torch.empty((3, nq), dtype=torch.int32, device=mask_logits.device)
    scores = torch.empty(nq, dtype=torch.float32, device=mask_logits.device)
    check(_lib.load().gf_proposal_stats(ptr(mask_logits), ptr(cls_logits), ptr(sem_prob), nq, N, ncls,
                                        float(logit_thresh), float(score_thresh), int(npoint_thresh), int(min_class),
                                        ptr(ints[0]), ptr(ints[1]), ptr(scores), ptr(ints[2]), stream_ptr()),
          "gf_proposal_stats")
    return ints[0], ints[1], scores, ints[2]


def proposal_stats_fs(mask_logits, sim, logit_thresh, score_thresh, npoint_thresh, sim_thresh):
    """Few-shot proposal statistics (geoformer_fs.py:205-238): (npoints i32[nq], scores f32[nq], final i32[nq]) of
    the queries' mask-logit rows [nq,N] and their similarities to the support prototype [nq]."""
    _f32c(mask_logits, "mask_logits"), _f32c(sim, "sim")
    nq, N = mask_logits.shape
    if sim.shape != (nq,):
        raise RuntimeError(f"sim must be [{nq}], got {tuple(sim.shape)}")
    ints = torch.empty((2, nq), dtype=torch.int32, device=mask_logits.device)
    scores = torch.empty(nq, dtype=torch.float32, device=mask_logits.device)
    check(_lib.load().gf_proposal_stats_fs(ptr(mask_logits), ptr(sim), nq, N, float(logit_thresh), float(score_thresh),
                                           int(npoint_thresh), float(sim_thresh), ptr(ints[0]), ptr(scores),
                                           ptr(ints[1]), stream_ptr()), "gf_proposal_stats_fs")
    return ints[0], scores, ints[1]


def proposal_select(final, cls_pred, scores):
    """Accepted queries compacted on the device: (sel i32[nq], cls i64[nq], scores f32[nq], count i32[1]); the first
    `count` entries are valid."""
    _i32c(final, "final"); _i32c(cls_pred, "cls_pred"); _f32c(scores, "scores")
    nq = final.shape[0]
    dev = final.device
    sel = torch.empty(nq, dtype=torch.int32, device=dev)
    cls = torch.empty(nq, dtype=torch.int64, device=dev)
    sc = torch.empty(nq, dtype=torch.float32, device=dev)
    cnt = torch.empty(1, dtype=torch.int32, device=dev)
    check(_lib.load().gf_proposal_select(ptr(final), ptr(cls_pred), ptr(scores), nq, ptr(sel), ptr(cls), ptr(sc), ptr(cnt),
                                         stream_ptr()), "gf_proposal_select")
    return sel, cls, sc, cnt


def proposal_scatter(mask_logits, sel, fg_idxs, logit_thresh, num_points):
    """0/1 membership rows [len(sel), num_points] (int32) of the selected queries over the scene's points."""
    _f32c(mask_logits, "mask_logits"), _i32c(sel, "sel")
    if not (fg_idxs.is_cuda and fg_idxs.dtype == torch.int64 and fg_idxs.is_contiguous()):
        raise RuntimeError("fg_idxs: expected a contiguous int64 tensor on the GPU")
    out = torch.zeros((sel.shape[0], num_points), dtype=torch.int32, device=mask_logits.device)
    check(_lib.load().gf_proposal_scatter(ptr(mask_logits), ptr(sel), sel.shape[0], mask_logits.shape[1],
                                          ptr(fg_idxs), float(logit_thresh), int(num_points), ptr(out), stream_ptr()),
          "gf_proposal_scatter")
    return out


def relpos_prepare(geo, inds):
    """(geo_ctx [nq,nc], max_geo [nq]) of one scene: geo[:, inds] and its row maxima with all-unreachable rows set to
    the largest maximum (ingredients of the relative position embedding, csrc/proposal.hip)."""
    _f32c(geo, "geo"); _i32c(inds, "inds")
    nq, n = geo.shape
    nc = inds.shape[0]
    geo_ctx = torch.empty((nq, nc), dtype=torch.float32, device=geo.device)
    max_geo = torch.empty(nq, dtype=torch.float32, device=geo.device)
    check(_lib.load().gf_relpos_prepare(ptr(geo), ptr(inds), nq, n, nc, ptr(geo_ctx), ptr(max_geo), stream_ptr()),
          "gf_relpos_prepare")
    return geo_ctx, max_geo


def mask_intersections(masks):
    """inter[i,j] = |mask_i AND mask_j| for 0/1 int32 masks [n,N] (bit-packed popcount kernel)."""
    _i32c(masks, "masks")
    n, N = masks.shape
    lib = _lib.load()
    scratch = torch.empty(lib.gf_mask_intersections_scratch_bytes(n, N) // 8 + 1, dtype=torch.int64,
                          device=masks.device)
    inter = torch.empty((n, n), dtype=torch.int32, device=masks.device)
    check(lib.gf_mask_intersections(ptr(masks), n, N, ptr(scratch), ptr(inter), stream_ptr()), "gf_mask_intersections")
    return inter


def overlap_layout(n, max_gt, extra_words=0):
    """Word offsets (int32 words) of instance_overlaps_packed's buffer: G at 0, gt_id (int64) at `id`, gt_count at `count`,
    inter [n, G+1] at `inter`, `extra_words` caller words at `extra` (an even offset: 8-byte values fit), `total` words."""
    o_id = 2
    o_cnt = o_id + 2 * max_gt
    o_inter = o_cnt + max_gt
    o_extra = (o_inter + n * (max_gt + 1) + 1) // 2 * 2
    return {"id": o_id, "count": o_cnt, "inter": o_inter, "extra": o_extra, "total": o_extra + extra_words}


def instance_overlaps_packed(masks, gt_ids, class_ids, rows=None, max_gt=256, extra_words=0):
    """One gf_instance_overlaps call into a single int32 device buffer laid out by overlap_layout(n, max_gt, extra_words),
    so that one device-to-host copy brings every table back.  No synchronisation: buf[0] (G) may exceed max_gt, in which
    case only buf[0] is meaningful.  Returns (buf, layout)."""
    _i32c(masks, "masks")
    if masks.dim() != 2:
        raise RuntimeError("masks: expected [n_rows, N]")
    if not (gt_ids.is_cuda and gt_ids.dtype == torch.int64 and gt_ids.is_contiguous() and gt_ids.dim() == 1):
        raise RuntimeError("gt_ids: expected a contiguous int64 vector on the GPU")
    _i32c(class_ids, "class_ids")
    n_rows, N = masks.shape
    if gt_ids.shape[0] != N:
        raise RuntimeError(f"gt_ids has {gt_ids.shape[0]} points, the masks {N}")
    if rows is not None:
        _i32c(rows, "rows")
    n = n_rows if rows is None else rows.shape[0]
    C = class_ids.shape[0]
    lay = overlap_layout(n, max_gt, extra_words)
    buf = torch.empty(lay["total"], dtype=torch.int32, device=masks.device)
    lib = _lib.load()
    scratch = torch.empty(lib.gf_instance_overlaps_scratch_bytes(N, C) // 4 + 1, dtype=torch.int32, device=masks.device)
    base = buf.data_ptr()
    check(lib.gf_instance_overlaps(ptr(masks), n_rows, N, ptr(rows), n, ptr(gt_ids), ptr(class_ids), C, max_gt,
                                   ptr(scratch), base, base + 4 * lay["id"], base + 4 * lay["count"],
                                   base + 4 * lay["inter"], stream_ptr()), "gf_instance_overlaps")
    return buf, lay


def instance_overlaps(masks, gt_ids, class_ids, rows=None, max_gt=256):
    """Overlap tables of the instance evaluation for one scene (gf_instance_overlaps): device tensors
    (gt_id int64 [G], gt_count int32 [G], inter int32 [n, G+1]) -- instances in ascending id order, inter[i, g] the
    points of picked mask i in instance g, inter[i, G] its void points.  masks int32 [n_rows, N] (any nonzero is a
    member), gt_ids int64 [N] (val_gt encoding), class_ids int32 [C] (the evaluated nyu40 ids), rows int32 [n] (the
    picked rows, default all).  Reads G back (one synchronisation) and repeats the call with room for G instances when
    max_gt was too small."""
    while True:
        buf, lay = instance_overlaps_packed(masks, gt_ids, class_ids, rows, max_gt)
        G = int(buf[0])
        if G <= max_gt:
            break
        max_gt = G
    n = masks.shape[0] if rows is None else rows.shape[0]
    gt_id = buf[lay["id"]:lay["id"] + 2 * G].view(torch.int64)
    gt_count = buf[lay["count"]:lay["count"] + G]
    inter = buf[lay["inter"]:lay["inter"] + n * (G + 1)].view(n, G + 1)
    return gt_id, gt_count, inter


def semantic_confusion_limits():
    """(largest class count, points per workgroup run) of gf_semantic_confusion."""
    lib = _lib.load()
    return lib.gf_semantic_confusion_max_classes(), lib.gf_semantic_confusion_run_points()


def semantic_confusion(scores, labels, offsets, conf, *, lut=None, ignore_label=-100, map_ignore=-1, map_other=-1,
                       want_preds=True, offsets_host=None):
    """Per-point predictions and per-scene confusion matrices of a batch (gf_semantic_confusion), one launch on the
    current stream, nothing read back.  scores fp32 [N, C]; labels int64 [N] or None (prediction only: conf is left as
    it is); offsets int32 [S+1] on the device; conf int64 [S, C+1, C], ADDED to (row = mapped label, C = ignored; column
    = prediction).  lut int32 [L] on the device: label -> class for 0..L-1, map_other outside, map_ignore for
    ignore_label; None: the identity over 0..C-1.  offsets_host: a host int32 copy of offsets, checked by the native
    call before it launches (without it a malformed table loses counts, nothing else).  Returns preds int32 [N] (the
    first maximal class, select_foreground's rule), None with want_preds=False."""
    _f32c(scores, "scores")
    if scores.dim() != 2:
        raise RuntimeError("scores: expected [N, C]")
    N, C = scores.shape
    S = 0
    if labels is not None:
        if not (labels.is_cuda and labels.dtype == torch.int64 and labels.is_contiguous() and labels.shape == (N,)):
            raise RuntimeError(f"labels: expected a contiguous int64 [{N}] tensor on the GPU")
        _i32c(offsets, "offsets")
        S = offsets.shape[0] - 1
        if not (conf.is_cuda and conf.dtype == torch.int64 and conf.is_contiguous() and conf.shape == (S, C + 1, C)):
            raise RuntimeError(f"conf: expected a contiguous int64 [{S}, {C + 1}, {C}] tensor on the GPU")
        if offsets_host is not None and not (offsets_host.device.type == "cpu" and offsets_host.dtype == torch.int32
                                             and offsets_host.is_contiguous() and offsets_host.shape == (S + 1,)):
            raise RuntimeError(f"offsets_host: expected a contiguous int32 [{S + 1}] host tensor")
    if lut is not None:
        _i32c(lut, "lut")
    preds = torch.empty(N, dtype=torch.int32, device=scores.device) if want_preds else None
    check(_lib.load().gf_semantic_confusion(
        ptr(scores), ptr(labels), ptr(offsets) if labels is not None else None,
        ptr(offsets_host) if labels is not None else None, S, N, C, ptr(lut), 0 if lut is None else lut.shape[0],
        int(ignore_label), int(map_ignore), int(map_other), ptr(preds), ptr(conf) if labels is not None else None,
        stream_ptr()), "gf_semantic_confusion")
    return preds


def panoptic_limits():
    """(largest row count P + n_stuff + 1, points per workgroup run) of gf_panoptic_overlaps."""
    lib = _lib.load()
    return lib.gf_panoptic_max_rows(), lib.gf_panoptic_run_points()


def panoptic_layout(S, R, max_gt):
    """Word offsets (int32 words) of panoptic_overlaps_packed's buffer: G [S] at 0, gt_id (int64 [S, max_gt]) at `id`,
    inter [S, R, max_gt + 1] at `inter`, `total` words."""
    o_id = (S + 1) // 2 * 2
    o_inter = o_id + 2 * S * max_gt
    return {"id": o_id, "inter": o_inter, "total": o_inter + S * R * (max_gt + 1)}


def _panoptic_args(owner, ids, sem, gt_ids, offsets, class_ids, is_stuff, stuff_of_sem, offsets_host):
    _i32c(owner, "owner"); _i32c(sem, "sem"); _i32c(offsets, "offsets")
    _i32c(class_ids, "class_ids"); _i32c(is_stuff, "is_stuff"); _i32c(stuff_of_sem, "stuff_of_sem")
    N, S = owner.shape[0], offsets.shape[0] - 1
    if ids is not None:
        _i32c(ids, "ids")
    for name, t in (("owner", owner), ("ids", ids), ("sem", sem), ("gt_ids", gt_ids)):
        if t is not None and t.shape != (N,):
            raise RuntimeError(f"{name}: expected [{N}], one value per point")
    if gt_ids is not None and not (gt_ids.is_cuda and gt_ids.dtype == torch.int64 and gt_ids.is_contiguous()):
        raise RuntimeError("gt_ids: expected a contiguous int64 vector on the GPU")
    if class_ids.shape != is_stuff.shape or class_ids.dim() != 1:
        raise RuntimeError("class_ids / is_stuff: expected two [C] vectors")
    if offsets_host is not None and not (offsets_host.device.type == "cpu" and offsets_host.dtype == torch.int32
                                         and offsets_host.is_contiguous() and offsets_host.shape == (S + 1,)):
        raise RuntimeError(f"offsets_host: expected a contiguous int32 [{S + 1}] host tensor")
    return N, S


def panoptic_overlaps_packed(owner, ids, sem, gt_ids, offsets, class_ids, is_stuff, stuff_of_sem, n_stuff, P,
                             max_gt=256, offsets_host=None, want_pan=True):
    """One gf_panoptic_overlaps call into a single int32 device buffer laid out by panoptic_layout(S, R, max_gt), so
    that one device-to-host copy brings every table back.  No synchronisation: a scene's G may exceed max_gt, in which
    case only its G is meaningful.  Returns (pan int32 [N] or None, buf, layout)."""
    N, S = _panoptic_args(owner, ids, sem, gt_ids, offsets, class_ids, is_stuff, stuff_of_sem, offsets_host)
    if gt_ids is None:
        raise RuntimeError("gt_ids: needed for the tables (panoptic_points gives the labels alone)")
    C = class_ids.shape[0]
    R = int(P) + int(n_stuff) + 1
    lay = panoptic_layout(S, R, int(max_gt))
    dev = owner.device
    buf = torch.empty(lay["total"], dtype=torch.int32, device=dev)
    pan = torch.empty(N, dtype=torch.int32, device=dev) if want_pan else None
    lib = _lib.load()
    ws = scratch("panoptic", lib.gf_panoptic_overlaps_scratch_bytes(S, N, C) // 4 + 1, torch.int32, dev)
    base = buf.data_ptr()
    check(lib.gf_panoptic_overlaps(ptr(owner), ptr(ids) if want_pan else None, ptr(sem), ptr(gt_ids), ptr(offsets),
                                   ptr(offsets_host), S, N, ptr(class_ids), ptr(is_stuff), C, ptr(stuff_of_sem),
                                   stuff_of_sem.shape[0], int(n_stuff), int(P), int(max_gt), ptr(ws), ptr(pan), base,
                                   base + 4 * lay["id"], base + 4 * lay["inter"], stream_ptr()), "gf_panoptic_overlaps")
    return pan, buf, lay


def panoptic_unpack(h, lay, S, R, max_gt):
    """(G int32 [S], gt_id int64 [S, max_gt], inter int32 [S, R, max_gt + 1]) of a host copy of the packed buffer."""
    G = h[:S]
    gt_id = h[lay["id"]:lay["id"] + 2 * S * max_gt].view(np.int64).reshape(S, max_gt)
    inter = h[lay["inter"]:lay["inter"] + S * R * (max_gt + 1)].reshape(S, R, max_gt + 1)
    return G, gt_id, inter


def panoptic_overlaps(owner, ids, sem, gt_ids, offsets, class_ids, is_stuff, stuff_of_sem, n_stuff, P, max_gt=256,
                      offsets_host=None, want_pan=True):
    """Panoptic ids and contingency tables of a batch of S scenes packed one after the other (gf_panoptic_overlaps):
    (pan int32 [N] on the device, G int32 [S], gt_id int64 [S, max_gt], inter int32 [S, R, max_gt + 1], max_gt) with the
    tables on the host (numpy; one device-to-host copy per call).  owner / ids / sem int32 [N], gt_ids int64 [N],
    offsets int32 [S+1], class_ids / is_stuff int32 [C], stuff_of_sem int32 [L]: device tensors.  Rows: P thing rows,
    n_stuff stuff rows, the unlabelled row; columns: a scene's segments in ascending key order, void at max_gt.  When a
    scene has more than max_gt segments the call is repeated with room for them: the returned max_gt is the one used."""
    S, R = offsets.shape[0] - 1, int(P) + int(n_stuff) + 1
    while True:
        pan, buf, lay = panoptic_overlaps_packed(owner, ids, sem, gt_ids, offsets, class_ids, is_stuff, stuff_of_sem,
                                                 n_stuff, P, max_gt, offsets_host, want_pan)
        G, gt_id, inter = panoptic_unpack(buf.cpu().numpy(), lay, S, R, max_gt)
        if S == 0 or int(G.max()) <= max_gt:
            return pan, G, gt_id, inter, max_gt
        max_gt = int(G.max())  # nothing was written past the capacities: run again with room


def panoptic_points(owner, ids, sem, offsets, class_ids, is_stuff, stuff_of_sem, n_stuff, P):
    """Panoptic id of every point (gf_panoptic_overlaps without ground truth: one launch, no table): ids where the
    point has an owner in [0, P), class_ids[j] * 1000 where the semantic class names stuff class j, 0 elsewhere."""
    N, S = _panoptic_args(owner, ids, sem, None, offsets, class_ids, is_stuff, stuff_of_sem, None)
    pan = torch.empty(N, dtype=torch.int32, device=owner.device)
    if N:
        check(_lib.load().gf_panoptic_overlaps(ptr(owner), ptr(ids), ptr(sem), None, ptr(offsets), None, S, N,
                                               ptr(class_ids), ptr(is_stuff), class_ids.shape[0], ptr(stuff_of_sem),
                                               stuff_of_sem.shape[0], int(n_stuff), int(P), 0, None, ptr(pan), None,
                                               None, None, stream_ptr()), "gf_panoptic_overlaps")
    return pan


def backbone_transformer_params(before, transformer, after):
    """Device-pointer table of gf_backbone_transformer in the order include/geoformer_hip.h documents."""
    import ctypes

    ts = [before.weight, before.bias, transformer.position_linear.weight, transformer.position_linear.bias]
    for layer in transformer.layers:
        a, ff = layer.attn_1, layer.ff
        ts += [layer.norm_1.alpha, layer.norm_1.bias, a.q_linear.weight, a.q_linear.bias, a.k_linear.weight,
               a.k_linear.bias, a.v_linear.weight, a.v_linear.bias, a.out.weight, a.out.bias, layer.norm_2.alpha,
               layer.norm_2.bias, ff.linear_1.weight, ff.linear_1.bias, ff.linear_2.weight, ff.linear_2.bias]
    ts += [transformer.norm.alpha, transformer.norm.bias, after.weight, after.bias]
    for t in ts:
        _f32c(t.data, "transformer parameter")
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts]), len(transformer.layers)


BACKBONE_TRANSFORMER_MAX_C = 384  # csrc/backbone_attn.hip: 3 * BT_D, the widest level either form of the stack takes


def backbone_transformer_supported(c, transformer):
    """Whether gf_backbone_transformer (inference) takes a level of width c with this transformer: the native entry's
    argument checks (bt_forward) plus the fixed shape of its kernels -- d_model 128, 4 heads, d_ff 64, 1..4 layers."""
    return (c > 0 and c % 16 == 0 and c <= BACKBONE_TRANSFORMER_MAX_C and transformer.d_model == 128
            and 1 <= len(transformer.layers) <= 4
            and all(l.attn_1.h == 4 and l.ff.linear_1.out_features == 64 for l in transformer.layers))


def backbone_transformer(feats, coords, scene_offsets, n_scenes, params, n_layers):
    """Fused before-linear -> per-scene voxel transformer -> after-linear: feats [M,c], coords int32 [M,4],
    scene_offsets int32 [n_scenes+1] on the device.  Returns [M,c]."""
    _f32c(feats, "feats")
    if coords.dtype != torch.int32 or not coords.is_contiguous():
        raise RuntimeError("coords must be contiguous int32 [M,4]")
    lib = _lib.load()
    M, c = feats.shape
    out = torch.empty_like(feats)
    scratch = torch.empty(lib.gf_backbone_transformer_scratch_bytes(M) // 4, dtype=torch.float32, device=feats.device)
    check(lib.gf_backbone_transformer(ptr(feats), ptr(coords), ptr(scene_offsets), n_scenes, M, c, n_layers, params,
                                      ptr(scratch), ptr(out), stream_ptr()), "gf_backbone_transformer")
    return out


def backbone_transformer_tensors(before, transformer, after):
    """The parameters of the voxel transformer stack in the order of gf_backbone_transformer's table."""
    ts = [before.weight, before.bias, transformer.position_linear.weight, transformer.position_linear.bias]
    for layer in transformer.layers:
        a, ff = layer.attn_1, layer.ff
        ts += [layer.norm_1.alpha, layer.norm_1.bias, a.q_linear.weight, a.q_linear.bias, a.k_linear.weight,
               a.k_linear.bias, a.v_linear.weight, a.v_linear.bias, a.out.weight, a.out.bias, layer.norm_2.alpha,
               layer.norm_2.bias, ff.linear_1.weight, ff.linear_1.bias, ff.linear_2.weight, ff.linear_2.bias]
    return ts + [transformer.norm.alpha, transformer.norm.bias, after.weight, after.bias]


def dropout_keep_reference(seed, p, site, rows, cols):
    """The keep factor (0 or 1/(1-p)) gf_backbone_transformer_train_* uses for element (row, col) of a dropout site, as
    the header states it -- for tests that rebuild the masks.  rows, cols: integer tensors (broadcast together)."""
    M32 = 0xFFFFFFFF

    def fmix(x):
        x = x ^ (x >> 16)
        x = (x * 0x85EBCA6B) & M32
        x = x ^ (x >> 13)
        x = (x * 0xC2B2AE35) & M32
        return x ^ (x >> 16)

    rows, cols = rows.to(torch.int64), cols.to(torch.int64)
    h = fmix((int(seed) & M32) ^ ((rows * 64 + int(site)) & M32))
    h = fmix((h + ((cols * 0x9E3779B1) & M32)) & M32)
    if p <= 0:
        return torch.ones_like(h, dtype=torch.float32)
    keep = (h >> 8) >= int(float(p) * 16777216.0)
    return keep.to(torch.float32) * float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


class _VoxelTransformerTrainFn(torch.autograd.Function):
    """before-linear -> per-scene voxel transformer (with its dropouts) -> after-linear of a deep U-Net level, forward and
    backward in csrc/backbone_attn.hip (gf_backbone_transformer_train_fwd / _bwd)."""

    @staticmethod
    def forward(ctx, feats, coords, n_scenes, n_layers, p, seed, *params):
        import ctypes

        lib = _lib.load()
        M, c = feats.shape
        feats = _f32c(feats.contiguous(), "feats")
        params = [_f32c(t.detach().contiguous(), "transformer parameter") for t in params]
        table = (ctypes.c_void_p * len(params))(*[t.data_ptr() for t in params])
        out = torch.empty_like(feats)
        save = torch.empty(lib.gf_backbone_transformer_train_save_bytes(M, n_layers) // 4, dtype=torch.float32,
                           device=feats.device)
        check(lib.gf_backbone_transformer_train_fwd(ptr(feats), ptr(coords), n_scenes, M, c, n_layers, table, float(p),
                                                    int(seed), ptr(save), ptr(out), stream_ptr()),
              "gf_backbone_transformer_train_fwd")
        ctx.save_for_backward(feats, save, *params)
        ctx.cfg = (n_scenes, n_layers, float(p), int(seed))
        return out

    @staticmethod
    def backward(ctx, dout):
        import ctypes

        lib = _lib.load()
        feats, save, *params = ctx.saved_tensors
        n_scenes, n_layers, p, seed = ctx.cfg
        M, c = feats.shape
        dout = _f32c(dout.contiguous(), "dout")
        table = (ctypes.c_void_p * len(params))(*[t.data_ptr() for t in params])
        work = torch.empty(lib.gf_backbone_transformer_train_work_bytes(M, n_layers, n_scenes) // 4, dtype=torch.float32,
                           device=feats.device)
        grads = torch.empty(lib.gf_backbone_transformer_grad_floats(c, n_layers), dtype=torch.float32, device=feats.device)
        dfeats = torch.empty_like(feats)
        check(lib.gf_backbone_transformer_train_bwd(ptr(feats), ptr(dout), n_scenes, M, c, n_layers, table, p, seed,
                                                    ptr(save), ptr(work), ptr(dfeats), ptr(grads), stream_ptr()),
              "gf_backbone_transformer_train_bwd")
        outs, o = [], 0
        for t in params:
            outs.append(grads[o:o + t.numel()].view(t.shape))
            o += t.numel()
        assert o == grads.numel()
        return (dfeats, None, None, None, None, None) + tuple(outs)


def backbone_transformer_train_supported(feats, coords, transformer):
    return (feats.is_cuda and feats.dtype == torch.float32 and feats.shape[0] > 0 and feats.shape[1] % 16 == 0
            and feats.shape[1] <= BACKBONE_TRANSFORMER_MAX_C and coords.dtype == torch.int32 and coords.is_contiguous()
            and transformer.d_model == 128 and 1 <= len(transformer.layers) <= 4
            and len({float(m.p) for m in transformer.modules() if isinstance(m, torch.nn.Dropout)}) == 1
            and all(l.attn_1.h == 4 and l.ff.linear_1.out_features == 64 for l in transformer.layers)
            and os.environ.get("GF_FUSED_VOXEL_TRANSFORMER", "1") != "0")


def backbone_transformer_train(feats, coords, n_scenes, before, transformer, after, seed=None):
    """Training forward of a deep level's voxel transformer stack with a native backward.  The dropouts are active when
    the transformer module is in training mode (p of its modules); `seed` defaults to a draw from the framework's CPU
    generator, so torch.manual_seed fixes the masks."""
    layer0 = transformer.layers[0]
    p = float(layer0.dropout_1.p) if transformer.training else 0.0
    if seed is None:
        seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())
    ts = backbone_transformer_tensors(before, transformer, after)
    return _VoxelTransformerTrainFn.apply(feats, coords, int(n_scenes), len(transformer.layers), p, seed, *ts)


def decoder_pack_weights(W1, W2, Wv):
    lib = _lib.load()
    wp = torch.empty(lib.gf_decoder_wpack_floats(), dtype=torch.float32, device=W1.device)
    check(lib.gf_decoder_pack_weights(ptr(_f32c(W1, "W1")), ptr(_f32c(W2, "W2")), ptr(_f32c(Wv, "Wv")), ptr(wp),
                                      stream_ptr()), "gf_decoder_pack_weights")
    return wp


_launch_cfg = threading.local()


@contextlib.contextmanager
def co_resident_launches():
    """Inside this context the inference cross-attention is launched in its 8-wave workgroup shape
    (gf_decoder_cross_attn_cfg), which fits on a compute unit beside a BFS workgroup: SplitForward.finish() queues one
    scene's decoder under the next scene's sampling / BFS stretch.  Per host thread."""
    old = getattr(_launch_cfg, "cross_attn_waves", 16)
    _launch_cfg.cross_attn_waves = 8
    try:
        yield
    finally:
        _launch_cfg.cross_attn_waves = old


def co_resident():
    """Whether this host thread is inside ``co_resident_launches`` (a serving loop's SplitForward.finish())."""
    return getattr(_launch_cfg, "cross_attn_waves", 16) != 16


def decoder_cross_attn(geo_ctx, max_geo, qloc, cloc, lo, hi, gaussB, Q1, K1, Kv, wpack, b2):
    """Fused vector cross-attention; shapes as in include/geoformer_hip.h.  Returns [B,nq,64]."""
    for t, name in ((geo_ctx, "geo_ctx"), (max_geo, "max_geo"), (qloc, "qloc"), (cloc, "cloc"), (lo, "lo"), (hi, "hi"),
                    (gaussB, "gaussB"), (Q1, "Q1"), (K1, "K1"), (Kv, "Kv"), (wpack, "wpack"), (b2, "b2")):
        _f32c(t, name)
    B, nq, nc = geo_ctx.shape
    d = Q1.shape[-1]
    out = torch.empty((B, nq, d), dtype=torch.float32, device=Q1.device)
    check(_lib.load().gf_decoder_cross_attn_cfg(ptr(geo_ctx), ptr(max_geo), ptr(qloc), ptr(cloc), ptr(lo), ptr(hi),
                                                ptr(gaussB), ptr(Q1), ptr(K1), ptr(Kv), ptr(wpack), ptr(b2), B, nq, nc, d,
                                                ptr(out), None, None, getattr(_launch_cfg, "cross_attn_waves", 16),
                                                stream_ptr()), "gf_decoder_cross_attn")
    return out


class _CrossAttnFn(torch.autograd.Function):
    """Fused vector cross-attention with a fused, recompute-based backward (csrc/decoder_attn.hip).  Differentiable
    inputs: Q1 [B,nq,64], K1, Kv [B,nc,64] (the hoisted projections) and the pair weights W1, W2, Wv [64,64]; the
    geodesic embedding inputs are data."""

    @staticmethod
    def forward(ctx, geo_ctx, max_geo, qloc, cloc, lo, hi, gaussB, Q1, K1, Kv, W1, W2, Wv):
        lib = _lib.load()
        B, nq, nc = geo_ctx.shape
        d = Q1.shape[-1]
        wpack = decoder_pack_weights(W1.detach().contiguous(), W2.detach().contiguous(), Wv.detach().contiguous())
        out = torch.empty((B, nq, d), dtype=torch.float32, device=Q1.device)
        sm, sl = torch.empty_like(out), torch.empty_like(out)
        Q1, K1, Kv = Q1.contiguous(), K1.contiguous(), Kv.contiguous()
        check(lib.gf_decoder_cross_attn(ptr(geo_ctx), ptr(max_geo), ptr(qloc), ptr(cloc), ptr(lo), ptr(hi), ptr(gaussB),
                                        ptr(Q1), ptr(K1), ptr(Kv), ptr(wpack), None, B, nq, nc, d, ptr(out), ptr(sm),
                                        ptr(sl), stream_ptr()), "gf_decoder_cross_attn")
        ctx.save_for_backward(geo_ctx, max_geo, qloc, cloc, lo, hi, gaussB, Q1, K1, Kv, wpack, W2.detach().contiguous(),
                              out, sm, sl)
        return out

    @staticmethod
    def backward(ctx, gout):
        lib = _lib.load()
        geo_ctx, max_geo, qloc, cloc, lo, hi, gaussB, Q1, K1, Kv, wpack, W2, out, sm, sl = ctx.saved_tensors
        B, nq, nc = geo_ctx.shape
        d = Q1.shape[-1]
        dQ1 = torch.empty_like(Q1)
        dK1, dKv = torch.zeros_like(K1), torch.zeros_like(Kv)
        dW = torch.empty((3, d, d), dtype=torch.float32, device=Q1.device)
        scratch = torch.empty(lib.gf_decoder_cross_attn_bwd_scratch_floats(B, nq, nc), dtype=torch.float32,
                              device=Q1.device)
        check(lib.gf_decoder_cross_attn_bwd(ptr(geo_ctx), ptr(max_geo), ptr(qloc), ptr(cloc), ptr(lo), ptr(hi),
                                            ptr(gaussB), ptr(Q1), ptr(K1), ptr(Kv), ptr(wpack), ptr(W2), ptr(out),
                                            ptr(sm), ptr(sl), ptr(gout.contiguous()), B, nq, nc, d, ptr(dQ1), ptr(dK1),
                                            ptr(dKv), ptr(dW), ptr(scratch), stream_ptr()),
              "gf_decoder_cross_attn_bwd")
        return None, None, None, None, None, None, None, dQ1, dK1, dKv, dW[0], dW[1], dW[2]


def decoder_cross_attn_train(geo_ctx, max_geo, qloc, cloc, lo, hi, gaussB, Q1, K1, Kv, W1, W2, Wv):
    """[B,nq,64] with autograd through Q1, K1, Kv, W1, W2, Wv (fused forward AND backward)."""
    for t, name in ((geo_ctx, "geo_ctx"), (max_geo, "max_geo"), (qloc, "qloc"), (cloc, "cloc"), (lo, "lo"), (hi, "hi"),
                    (gaussB, "gaussB")):
        _f32c(t, name)
    return _CrossAttnFn.apply(geo_ctx, max_geo, qloc, cloc, lo, hi, gaussB, Q1, K1, Kv, W1, W2, Wv)


class _SoftmaxDim1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, scale):
        x = x.contiguous()
        n0, n1 = x.shape[0], x.shape[1]
        inner = x.numel() // max(n0 * n1, 1)
        y = torch.empty_like(x)
        check(_lib.load().gf_softmax_dim1_fwd(ptr(x), n0, n1, inner, float(scale), ptr(y), stream_ptr()),
              "gf_softmax_dim1_fwd")
        ctx.save_for_backward(y)
        ctx.scale = float(scale)
        return y

    @staticmethod
    def backward(ctx, gy):
        (y,) = ctx.saved_tensors
        gy = gy.contiguous()
        n0, n1 = y.shape[0], y.shape[1]
        inner = y.numel() // max(n0 * n1, 1)
        gx = torch.empty_like(y)
        check(_lib.load().gf_softmax_dim1_bwd(ptr(y), ptr(gy), n0, n1, inner, ctx.scale, ptr(gx), stream_ptr()),
              "gf_softmax_dim1_bwd")
        return gx, None


def softmax_dim1(x, scale=1.0):
    """softmax(scale * x, dim=1) for a float32 GPU tensor with >= 2 dims, differentiable (streaming HIP kernels)."""
    _f32c(x.detach() if x.is_contiguous() else x.detach().contiguous(), "x")
    return _SoftmaxDim1.apply(x, scale)


# ---- training-mode BatchNorm1d + ReLU over voxel rows (csrc/bn_train.hip) -----------------------------------------
class _BNReLUTrainFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, eps, momentum, relu):
        lib = _lib.load()
        M, C = x.shape
        y = torch.empty_like(x)
        stats = torch.empty((2, C), dtype=torch.float32, device=x.device)
        scratch = torch.empty(lib.gf_bn_train_scratch_floats(M, C), dtype=torch.float32, device=x.device)
        check(lib.gf_bn_relu_train_fwd(ptr(x), M, C, ptr(weight), ptr(bias), float(eps), float(momentum), int(relu),
                                       ptr(running_mean), ptr(running_var), ptr(y), stats[0].data_ptr(),
                                       stats[1].data_ptr(), ptr(scratch), stream_ptr()),
              "gf_bn_relu_train_fwd")
        ctx.save_for_backward(x, y, weight, stats)
        ctx.relu = int(relu)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, y, weight, stats = ctx.saved_tensors
        lib = _lib.load()
        M, C = x.shape
        gy = gy.contiguous()
        need_x = ctx.needs_input_grad[0]
        dx = torch.empty_like(x) if need_x else None
        dwb = torch.empty((2, C), dtype=torch.float32, device=x.device)
        scratch = torch.empty(lib.gf_bn_train_scratch_floats(M, C), dtype=torch.float32, device=x.device)
        check(lib.gf_bn_relu_train_bwd(ptr(x), ptr(y), ptr(gy), M, C, ptr(weight), stats[0].data_ptr(),
                                       stats[1].data_ptr(), ctx.relu, ptr(dx), dwb[0].data_ptr(), dwb[1].data_ptr(),
                                       ptr(scratch), stream_ptr()), "gf_bn_relu_train_bwd")
        return dx, dwb[0], dwb[1], None, None, None, None, None


def bn_relu_train_supported(bn, x):
    """Training-mode BatchNorm1d over fp32 voxel rows [M, C] on the GPU that the fused pair can take."""
    return (bn.training and not getattr(bn, "sync_across_ranks", False) and x.is_cuda and x.dim() == 2 and x.dtype == torch.float32 and x.shape[0] >= 2
            and x.shape[1] % 4 == 0 and x.shape[1] <= 256 and bn.affine and bn.track_running_stats
            and bn.momentum is not None)


def bn_relu_train(bn, x, relu=True):
    """relu(bn(x)) for a training-mode nn.BatchNorm1d `bn` over rows x [M, C]: batch statistics, running statistics
    updated like nn.BatchNorm1d does, three launches forward and three backward (autograd through x, weight, bias)."""
    _f32c(x, "x")
    y = _BNReLUTrainFn.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, bn.momentum, relu)
    if hasattr(bn, "_flush_counter"):
        bn._nbt_pending = getattr(bn, "_nbt_pending", 0) + 1  # the lean subclass counts on the host (model/layers.py)
    elif bn.num_batches_tracked is not None:
        bn.num_batches_tracked += 1
    return y


class _BNTrainCLFn(torch.autograd.Function):
    """Training-mode batch norm over the channel-major layouts [B, C, L] / [B, C, H, W] (csrc/bn_train.hip)."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, eps, momentum, relu):
        lib = _lib.load()
        B, C = x.shape[0], x.shape[1]
        L = x.numel() // (B * C)
        y = torch.empty_like(x)
        stats = torch.empty((2, C), dtype=torch.float32, device=x.device)
        scratch = torch.empty(lib.gf_bn_train_cl_scratch_floats(B, C, L), dtype=torch.float32, device=x.device)
        check(lib.gf_bn_relu_train_cl_fwd(ptr(x), B, C, L, ptr(weight), ptr(bias), float(eps), float(momentum), int(relu),
                                          ptr(running_mean), ptr(running_var), ptr(y), stats[0].data_ptr(),
                                          stats[1].data_ptr(), ptr(scratch), stream_ptr()),
              "gf_bn_relu_train_cl_fwd")
        ctx.save_for_backward(x, y if relu else None, weight, stats)
        ctx.relu, ctx.dims = int(relu), (B, C, L)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, y, weight, stats = ctx.saved_tensors
        lib = _lib.load()
        B, C, L = ctx.dims
        gy = gy.contiguous()
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dwb = torch.empty((2, C), dtype=torch.float32, device=x.device)
        scratch = torch.empty(lib.gf_bn_train_cl_scratch_floats(B, C, L), dtype=torch.float32, device=x.device)
        check(lib.gf_bn_relu_train_cl_bwd(ptr(x), ptr(y), ptr(gy), B, C, L, ptr(weight), stats[0].data_ptr(),
                                          stats[1].data_ptr(), ctx.relu, ptr(dx), dwb[0].data_ptr(), dwb[1].data_ptr(),
                                          ptr(scratch), stream_ptr()),
              "gf_bn_relu_train_cl_bwd")
        return dx, dwb[0], dwb[1], None, None, None, None, None


def bn_train_cl_supported(bn, x):
    return (x.is_cuda and x.dtype == torch.float32 and x.dim() >= 3 and x.is_contiguous() and bn.affine
            and bn.track_running_stats and bn.momentum is not None and x.shape[1] <= 256
            and x.shape[0] * x.shape[1] < 65536 and x.numel() // x.shape[1] >= 2)


def bn_train_cl(bn, x, relu=False):
    """bn(x) (optionally followed by ReLU) for a training-mode BatchNorm over x [B, C, L...]: batch statistics, running
    statistics updated; three launches forward, three backward."""
    return _BNTrainCLFn.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, bn.momentum, relu)


# ---- row gathers with cheap exact gradients ---------------------------------------------------------------------------
class _TakeRowsUniqueFn(torch.autograd.Function):
    """x[idx] for an index WITHOUT repeats (the foreground list, the host-RNG draws without replacement): the gradient
    is a plain scatter of rows into zeros.  The framework's index backward does not know the rows are unique and goes
    through its accumulating index_put (sort / atomics: 0.3 ms for the [550k, 16] feature rows of a training batch)."""

    @staticmethod
    def forward(ctx, x, idx):
        ctx.save_for_backward(idx)
        ctx.shape = x.shape
        return x[idx]

    @staticmethod
    def backward(ctx, g):
        (idx,) = ctx.saved_tensors
        gx = g.new_zeros(ctx.shape)
        gx.index_copy_(0, idx, g)
        return gx, None


def take_rows_unique(x, idx):
    """x[idx] along dim 0; idx int64 without repeats (the caller's guarantee)."""
    if x.requires_grad and torch.is_grad_enabled() and x.is_cuda:
        return _TakeRowsUniqueFn.apply(x, idx)
    return x[idx]


class _PointsFromVoxelsFn(torch.autograd.Function):
    """feats[p2v_map] (voxel rows -> point rows, geoformer.py:541); the gradient is the per-voxel SUM of the points'
    rows -- the native voxel reduction over the rule table v2p_map (gf_voxelize_fp, sum mode: ascending point order,
    deterministic) instead of an accumulating index_put with atomics."""

    @staticmethod
    def forward(ctx, feats, p2v, v2p):
        ctx.save_for_backward(v2p)
        return feats[p2v.long()]

    @staticmethod
    def backward(ctx, g):
        (v2p,) = ctx.saved_tensors
        return voxelize_fp(g.contiguous(), v2p, mode=3), None, None


def points_from_voxels(feats, p2v, v2p=None):
    if (v2p is not None and feats.requires_grad and torch.is_grad_enabled() and feats.is_cuda and feats.dtype == torch.float32
            and v2p.dtype == torch.int32 and v2p.is_contiguous() and v2p.shape[0] == feats.shape[0]):
        return _PointsFromVoxelsFn.apply(feats, p2v, v2p)
    return feats[p2v.long()]


# ---- batched post-processing over a scene table (csrc/batch_post.hip) -----------------------------------------------
def _table_dev(table, device):
    """int64 scene table (numpy [S, F]) on the device: one small asynchronous upload from pinned memory."""
    t = torch.from_numpy(np.ascontiguousarray(table, dtype=np.int64))
    return t.pin_memory().to(device, non_blocking=True)


def proposal_stats_batched(table, nq, cls_logits, sem_t, logit_thresh, score_thresh, npoint_thresh, min_class=4):
    """proposal_stats of every (scene, query) in one launch: (cls_pred i32[S,nq], npoints i32[S,nq], scores f32[S,nq],
    final i32[S,nq]).  table: device int64 [S, GF_PROP_SCENE_FIELDS] (postprocess.proposal_scene_table);
    cls_logits fp32 [S, nq, ncls]; sem_t fp32 class-major [ncls, n_fg] over the batch's foreground points."""
    _f32c(cls_logits, "cls_logits"), _f32c(sem_t, "sem_t")
    S = table.shape[0]
    ncls = cls_logits.shape[-1]
    if cls_logits.shape != (S, nq, ncls) or sem_t.shape[0] != ncls:
        raise RuntimeError(f"proposal_stats_batched: cls_logits {tuple(cls_logits.shape)} / sem_t {tuple(sem_t.shape)} "
                           f"do not fit S={S} nq={nq}")
    dev = cls_logits.device
    ints = torch.empty((3, S, nq), dtype=torch.int32, device=dev)
    scores = torch.empty((S, nq), dtype=torch.float32, device=dev)
    check(_lib.load().gf_proposal_stats_batched(ptr(table), S, nq, ptr(cls_logits), ptr(sem_t), sem_t.shape[1], ncls,
                                                float(logit_thresh), float(score_thresh), int(npoint_thresh),
                                                int(min_class), ptr(ints[0]), ptr(ints[1]), ptr(scores), ptr(ints[2]),
                                                stream_ptr()), "gf_proposal_stats_batched")
    return ints[0], ints[1], scores, ints[2]


def proposal_select_batched(final, cls_pred, scores):
    """proposal_select per scene: (sel i32[S,nq], cls i64[S,nq], scores f32[S,nq], counts i32[S]); row b's first
    counts[b] entries are valid."""
    _i32c(final, "final"); _i32c(cls_pred, "cls_pred"); _f32c(scores, "scores")
    S, nq = final.shape
    dev = final.device
    sel = torch.empty((S, nq), dtype=torch.int32, device=dev)
    cls = torch.empty((S, nq), dtype=torch.int64, device=dev)
    sc = torch.empty((S, nq), dtype=torch.float32, device=dev)
    counts = torch.empty(S, dtype=torch.int32, device=dev)
    check(_lib.load().gf_proposal_select_batched(ptr(final), ptr(cls_pred), ptr(scores), S, nq, ptr(sel), ptr(cls),
                                                 ptr(sc), ptr(counts), stream_ptr()), "gf_proposal_select_batched")
    return sel, cls, sc, counts


def proposal_scatter_batched(table, sel, counts, total_rows, total_elems, max_N, fg_idxs, logit_thresh):
    """Accepted rows of every scene as 0/1 int32 over the scene's own points, packed into one buffer of total_elems
    (postprocess.packed_layout gives the blocks).  counts: the device counts of proposal_select_batched (their host
    copy gave total_rows / total_elems)."""
    _i32c(sel, "sel"); _i32c(counts, "counts")
    if not (fg_idxs.is_cuda and fg_idxs.dtype == torch.int64 and fg_idxs.is_contiguous()):
        raise RuntimeError("fg_idxs: expected a contiguous int64 tensor on the GPU")
    out = torch.zeros(int(total_elems), dtype=torch.int32, device=sel.device)
    check(_lib.load().gf_proposal_scatter_batched(ptr(table), table.shape[0], sel.shape[1], ptr(sel), ptr(counts),
                                                  int(total_rows), int(max_N), ptr(fg_idxs), float(logit_thresh),
                                                  ptr(out), stream_ptr()), "gf_proposal_scatter_batched")
    return out


def mask_intersections_batched(table, sizes):
    """[n_b, n_b] intersection blocks of every scene, packed (table / sizes: postprocess.nms_scene_table)."""
    dev = table.device
    bits = torch.empty(max(int(sizes["bits"]), 1), dtype=torch.int64, device=dev)
    inter = torch.empty(max(int(sizes["inter"]), 1), dtype=torch.int32, device=dev)
    check(_lib.load().gf_mask_intersections_batched(ptr(table), table.shape[0], int(sizes["max_waves"]),
                                                    int(sizes["max_pairs"]), ptr(bits), ptr(inter), stream_ptr()),
          "gf_mask_intersections_batched")
    return inter


def matrix_nms_batched(table, inter, sizes, kernel, sigma, final_score_thresh):
    """(picks i32 [sum n_b] packed at each scene's pick_off, pick_counts i32 [S]) of the fused matrix NMS."""
    dev = table.device
    picks = torch.empty(max(int(sizes["picks"]), 1), dtype=torch.int32, device=dev)
    counts = torch.empty(table.shape[0], dtype=torch.int32, device=dev)
    check(_lib.load().gf_matrix_nms_batched(ptr(table), table.shape[0], ptr(inter), int(kernel), float(sigma),
                                            float(final_score_thresh), ptr(picks), ptr(counts), stream_ptr()),
          "gf_matrix_nms_batched")
    return picks, counts


def greedy_nms_batched(table, inter, sizes, threshold):
    """(picks i32 [sum n_b] packed at each scene's pick_off, pick_counts i32 [S]) of the greedy NMS walk."""
    dev = table.device
    picks = torch.empty(max(int(sizes["picks"]), 1), dtype=torch.int32, device=dev)
    counts = torch.empty(table.shape[0], dtype=torch.int32, device=dev)
    check(_lib.load().gf_greedy_nms_batched(ptr(table), table.shape[0], ptr(inter), float(threshold), ptr(picks),
                                            ptr(counts), stream_ptr()), "gf_greedy_nms_batched")
    return picks, counts


def greedy_nms_ious(ious, scores, threshold):
    """(picks i32 [n], count i32 [1]) of the greedy NMS walk over a row-major fp32 [n, n] IoU matrix."""
    _f32c(ious, "ious"), _f32c(scores, "scores")
    n = scores.shape[0]
    if ious.shape != (n, n):
        raise RuntimeError(f"greedy_nms_ious: ious {tuple(ious.shape)} does not fit scores [{n}]")
    picks = torch.empty(max(n, 1), dtype=torch.int32, device=scores.device)
    count = torch.empty(1, dtype=torch.int32, device=scores.device)
    check(_lib.load().gf_greedy_nms_ious(ptr(ious), ptr(scores), n, float(threshold), ptr(picks), ptr(count),
                                         stream_ptr()), "gf_greedy_nms_ious")
    return picks, count


def label_map_batched(table, sizes, min_score):
    """gf_label_map_batched on a device label scene table (postprocess.label_scene_table): (int32 [2, points] = owner,
    ids; tab_i int32 [rows, GF_LBL_TABLE_INTS]; tab_f fp32 [rows, GF_LBL_TABLE_FLOATS])."""
    from .postprocess import LBL_OWN_SPLIT, LBL_TABLE_FLOATS, LBL_TABLE_INTS

    dev = table.device
    bits = torch.empty(max(int(sizes["bits"]), 1), dtype=torch.int64, device=dev)
    parts = max(int(sizes["parts"]), 1)
    part_f = torch.empty((parts, 9), dtype=torch.float32, device=dev)
    part_i = torch.empty(parts * (1 + LBL_OWN_SPLIT), dtype=torch.int32, device=dev)  # part_cnt, own_part
    points, rows = int(sizes["points"]), int(sizes["rows"])
    pts = torch.empty((2, max(points, 1)), dtype=torch.int32, device=dev)
    tab_i = torch.empty((max(rows, 1), LBL_TABLE_INTS), dtype=torch.int32, device=dev)
    tab_f = torch.empty((max(rows, 1), LBL_TABLE_FLOATS), dtype=torch.float32, device=dev)
    check(_lib.load().gf_label_map_batched(ptr(table), table.shape[0], int(sizes["max_points"]), int(sizes["max_picks"]),
                                           float(min_score), ptr(bits), ptr(part_f), ptr(part_i), ptr(part_i[parts:]),
                                           ptr(pts[0]), ptr(pts[1]), ptr(tab_i), ptr(tab_f), stream_ptr()),
          "gf_label_map_batched")
    return pts[:, :points], tab_i[:rows], tab_f[:rows]


# ---- mask logits pooled over over-segments (csrc/segment_pool.hip) ----------------------------------------------------
def segment_pool_limits():
    """(int64 words per row of the segment scene table, sorted positions per workgroup) of gf_segment_pool_batched."""
    lib = _lib.load()
    return lib.gf_segment_pool_scene_fields(), lib.gf_segment_pool_chunk_points()


def segment_pool_keys(seg_fg, fg_offsets):
    """(keys_sorted int64 [n_fg], order int32 [n_fg]) for gf_segment_pool_batched: one key per foreground row of the
    batch -- (scene, id) where the id is >= 0, (scene, 2^32 + the row's index in its scene) where it is negative, so such
    a row is a run of its own -- in one stable sort.  Framework plumbing on the current stream, nothing read back."""
    _i32c(seg_fg, "seg_fg")
    off = [int(o) for o in fg_offsets]
    n_fg, S = off[-1], len(off) - 1
    if seg_fg.shape != (n_fg,):
        raise RuntimeError(f"seg_fg: expected [{n_fg}], one id per foreground point, got {tuple(seg_fg.shape)}")
    dev = seg_fg.device
    pos = torch.arange(n_fg, dtype=torch.int64, device=dev)
    if S > 1:
        off_d = torch.tensor(off, dtype=torch.int64).pin_memory().to(dev, non_blocking=True)
        scene = torch.bucketize(pos, off_d[1:], right=True)
        pos = pos - off_d[scene]
    else:
        scene = None
    seg = seg_fg.long()
    key = torch.where(seg >= 0, seg, pos + (1 << 32))
    if scene is not None:
        key = key + (scene << 33)
    keys_sorted, order = torch.sort(key, stable=True)
    return keys_sorted, order.int()


def segment_pool_batched(logits_list, seg_fg, fg_offsets):
    """Mask logits pooled over the scenes' over-segments (postprocess.segment_pool_host per scene): a list of new fp32
    tensors [nq, N_b], every foreground point's logit replaced by the mean over the foreground points of its scene that
    carry its segment id; a point with a negative id keeps its logit.  logits_list: fp32 [nq, N_b] per kept scene of
    the forward; seg_fg int32 [n_fg] on the device, the ids of the batch's foreground points (scene-local: the same id
    in two scenes names two segments); fg_offsets: host offsets [S + 1] of the scenes' foreground rows.  A fixed number
    of launches on the current stream, no synchronisation; bit-identical from call to call and for a scene alone."""
    from . import postprocess

    S = len(logits_list)
    off = [int(o) for o in fg_offsets]
    if len(off) != S + 1:
        raise RuntimeError(f"segment_pool_batched: {S} scenes need {S + 1} foreground offsets")
    if S == 0:
        return []
    nq = logits_list[0].shape[0]
    for b, t in enumerate(logits_list):
        _f32c(t, "mask_logits")
        if t.shape != (nq, off[b + 1] - off[b]):
            raise RuntimeError(f"segment_pool_batched: scene {b}: logits {tuple(t.shape)}, expected "
                               f"[{nq}, {off[b + 1] - off[b]}]")
    outs = [torch.empty_like(t) for t in logits_list]
    n_fg = off[-1]
    if n_fg == 0:
        _i32c(seg_fg, "seg_fg")
        return outs
    keys_sorted, order = segment_pool_keys(seg_fg, off)
    table = postprocess.segment_scene_table([t.data_ptr() for t in logits_list], [t.data_ptr() for t in outs], off)
    dev = seg_fg.device
    table_d = _table_dev(table, dev)
    lib = _lib.load()
    ws = torch.empty(lib.gf_segment_pool_scratch_bytes(S, n_fg, nq) // 4 + 1, dtype=torch.int32, device=dev)
    check(lib.gf_segment_pool_batched(ptr(table_d), table.ctypes.data, S, nq, ptr(keys_sorted), ptr(order), n_fg,
                                      int(postprocess.scene_rows(table, postprocess.SEG_ROW)["N"].max()), ptr(ws),
                                      stream_ptr()), "gf_segment_pool_batched")
    return outs


# ---- geometric over-segmentation (csrc/oversegment.hip) -----------------------------------------------------------------
def _knn_rows(xyz, I, deg, name):
    _f32c(xyz, "xyz"); _i32c(I, "I"); _i32c(deg, "deg")
    n = xyz.shape[0]
    if xyz.dim() != 2 or xyz.shape[1] != 3 or I.dim() != 2 or I.shape[0] != n or I.shape[1] < 1 or deg.shape != (n,):
        raise RuntimeError(f"{name}: expected xyz [n, 3], I [n, k >= 1] and deg [n], got {tuple(xyz.shape)}, "
                           f"{tuple(I.shape)}, {tuple(deg.shape)}")
    return n, I.shape[1]


def point_normals(xyz, I, deg):
    """fp32 [n, 4] = (nx, ny, nz, sigma) per point of one scene from its kNN rows (knn_radius' I and deg): stage A of
    postprocess.oversegment_host (point_normals_host), one launch on the current stream."""
    n, k = _knn_rows(xyz, I, deg, "point_normals")
    out = torch.empty((n, 4), dtype=torch.float32, device=xyz.device)
    check(_lib.load().gf_point_normals(ptr(xyz), ptr(I), ptr(deg), n, k, ptr(out), stream_ptr()), "gf_point_normals")
    return out


def smooth_components(xyz, normals4, I, deg, normal_deg=15.0, offset=0.012, flatness=0.01, min_points=8):
    """int32 [n] over-segment ids (the smallest point index of the segment, or -1) from ANY kNN rows and ANY normals4
    (fp32 [n, 4]): stages B-D of postprocess.oversegment_host (smooth_components_host).  Five launches on the current
    stream, nothing read back; bit-identical from call to call."""
    n, k = _knn_rows(xyz, I, deg, "smooth_components")
    _f32c(normals4, "normals4")
    if normals4.shape != (n, 4):
        raise RuntimeError(f"smooth_components: expected normals4 [{n}, 4], got {tuple(normals4.shape)}")
    if min_points < 1:
        raise RuntimeError(f"smooth_components: min_points = {min_points} (at least 1)")
    lib = _lib.load()
    ids = torch.empty(n, dtype=torch.int32, device=xyz.device)
    ws = torch.empty(lib.gf_smooth_components_scratch_bytes(n) // 4 + 1, dtype=torch.int32, device=xyz.device)
    check(lib.gf_smooth_components(ptr(xyz), ptr(normals4), ptr(I), ptr(deg), n, k,
                                   float(np.float32(np.cos(np.radians(normal_deg)))), float(offset), float(flatness),
                                   int(min_points), ptr(ids), ptr(ws), stream_ptr()), "gf_smooth_components")
    return ids


def oversegment(xyz, k=16, radius=0.07, normal_deg=15.0, offset=0.012, flatness=0.01, min_points=8, return_flag=False):
    """Geometric over-segmentation of one scene (postprocess.oversegment_host): int32 [n] ids, the id space
    segment_pool_batched and the batch key "segments" accept.  xyz fp32 [n, 3] on the GPU: knn_radius(k, radius),
    point_normals and smooth_components on the current stream, nothing read back; return_flag: also knn_radius'
    truncation flag (int32 [1], device).  A CPU tensor runs the host statement (the flag is then None)."""
    if not xyz.is_cuda:
        from . import postprocess

        ids = torch.from_numpy(postprocess.oversegment_host(xyz, k=k, radius=radius, normal_deg=normal_deg,
                                                            offset=offset, flatness=flatness, min_points=min_points))
        return (ids, None) if return_flag else ids
    _f32c(xyz, "xyz")
    if min_points < 1:
        raise RuntimeError(f"oversegment: min_points = {min_points} (at least 1)")
    if xyz.shape[0] == 0:
        ids = torch.empty(0, dtype=torch.int32, device=xyz.device)
        return (ids, torch.zeros(1, dtype=torch.int32, device=xyz.device)) if return_flag else ids
    _, I, deg, flag = knn_radius(xyz, k, radius, sqrt_out=False, return_flag=True)
    ids = smooth_components(xyz, point_normals(xyz, I, deg), I, deg, normal_deg, offset, flatness, min_points)
    return (ids, flag) if return_flag else ids


# ---- picked masks split into connected clusters (csrc/mask_split.hip) ----------------------------------------------------
MSP_TABLE_INTS = _abi.const("GF_MSP_TABLE_INTS")
NMS_MAX_N = _abi.const("GF_NMS_MAX_N")


def _mask_rows(masks, pick, name):
    _i32c(masks, "masks")
    if not (pick.is_cuda and pick.dtype == torch.int64 and pick.is_contiguous()):
        raise RuntimeError(f"{name}: pick: expected a contiguous int64 tensor on the GPU")
    if masks.dim() != 2 or pick.dim() != 1:
        raise RuntimeError(f"{name}: expected masks [n_rows, N] and pick [p], got {tuple(masks.shape)}, "
                           f"{tuple(pick.shape)}")
    if pick.shape[0] > NMS_MAX_N:
        raise RuntimeError(f"{name}: {pick.shape[0]} picks (at most {NMS_MAX_N})")
    return masks.shape[0], masks.shape[1], pick.shape[0]


def mask_components(masks, pick, I, deg, min_samples=1, min_points=1):
    """DBSCAN of the picked rows of masks (int32 [n_rows, N], nonzero = member; pick int64 [p]) over one scene's kNN rows
    (knn_radius' I int32 [N, k] and deg int32 [N]), every mask restricting the graph to its own points:
    postprocess.mask_components_host on the GPU.  Returns (comp int32 [p, N]: the cluster id -- its smallest core point
    -- of every member point or -1, tab int32 [p, 5]: members, clusters kept, points in them, the largest cluster's id or
    -1, its size).  Seven launches on the current stream, nothing read back; bit-identical from call to call."""
    n_rows, N, p = _mask_rows(masks, pick, "mask_components")
    _i32c(I, "I"); _i32c(deg, "deg")
    if I.dim() != 2 or I.shape[0] != N or I.shape[1] < 1 or deg.shape != (N,):
        raise RuntimeError(f"mask_components: expected I [{N}, k >= 1] and deg [{N}], got {tuple(I.shape)}, "
                           f"{tuple(deg.shape)}")
    if min_samples < 1 or min_points < 1:
        raise RuntimeError(f"mask_components: min_samples = {min_samples}, min_points = {min_points} (at least 1)")
    lib = _lib.load()
    dev = masks.device
    comp = torch.empty((p, N), dtype=torch.int32, device=dev)
    if N == 0 or p == 0:  # nothing is launched: the rows of picks without points
        return comp, torch.tensor([0, 0, 0, -1, 0], dtype=torch.int32, device=dev).repeat(p, 1)
    tab = torch.empty((p, MSP_TABLE_INTS), dtype=torch.int32, device=dev)
    ws = torch.empty(lib.gf_mask_components_scratch_bytes(N, p) // 8 + 1, dtype=torch.int64, device=dev)
    check(lib.gf_mask_components(ptr(masks), n_rows, N, ptr(pick), p, ptr(I), ptr(deg), I.shape[1], int(min_samples),
                                 int(min_points), ptr(comp), ptr(tab), ptr(ws), stream_ptr()), "gf_mask_components")
    return comp, tab


def mask_keep_largest(masks, pick, comp, tab):
    """masks_out int32 [n_rows, N]: every picked row of masks cut down to its largest kept cluster (mask_components' comp
    and tab; all zero without one), every other row copied.  One launch on the current stream, nothing read back."""
    n_rows, N, p = _mask_rows(masks, pick, "mask_keep_largest")
    _i32c(comp, "comp"); _i32c(tab, "tab")
    if comp.shape != (p, N) or tab.shape != (p, MSP_TABLE_INTS):
        raise RuntimeError(f"mask_keep_largest: expected comp [{p}, {N}] and tab [{p}, {MSP_TABLE_INTS}], got "
                           f"{tuple(comp.shape)}, {tuple(tab.shape)}")
    if p == 0 or n_rows == 0 or N == 0:
        return masks.clone()
    out = torch.empty_like(masks)
    check(_lib.load().gf_mask_keep_largest(ptr(masks), n_rows, N, ptr(pick), p, ptr(comp), ptr(tab), ptr(out),
                                           stream_ptr()), "gf_mask_keep_largest")
    return out


def dbscan(xyz, radius, min_samples=1, k=32, min_points=1, return_flag=False):
    """DBSCAN of one point cloud: int32 [n] cluster ids (the smallest core point of the cluster) or -1 for noise and for
    clusters of fewer than min_points points.  xyz fp32 [n, 3] on the GPU: knn_radius(k, radius) and mask_components
    with one all-ones mask on the current stream, nothing read back.  The rows hold at most k - 1 neighbours: with every
    in-radius neighbour in its row (deg < k - 1 everywhere) the result is sklearn.cluster.DBSCAN(radius, min_samples)
    with the clusters named by their smallest core index; return_flag: also knn_radius' truncation flag (int32 [1],
    device).  A CPU tensor runs the host statement (the flag is then None)."""
    if min_samples < 1 or min_points < 1:
        raise RuntimeError(f"dbscan: min_samples = {min_samples}, min_points = {min_points} (at least 1)")
    if not xyz.is_cuda:
        from . import postprocess

        I, deg = postprocess.knn_radius_host(xyz, k, radius)
        n = I.shape[0]
        comp, _ = postprocess.mask_components_host(np.ones((1, n), np.int32), np.zeros(1, np.int64), I, deg,
                                                   min_samples, min_points)
        ids = torch.from_numpy(comp[0].copy())
        return (ids, None) if return_flag else ids
    _f32c(xyz, "xyz")
    n = xyz.shape[0]
    if n == 0:
        ids = torch.empty(0, dtype=torch.int32, device=xyz.device)
        return (ids, torch.zeros(1, dtype=torch.int32, device=xyz.device)) if return_flag else ids
    _, I, deg, flag = knn_radius(xyz, k, radius, sqrt_out=False, return_flag=True)
    comp, _ = mask_components(torch.ones((1, n), dtype=torch.int32, device=xyz.device),
                              torch.zeros(1, dtype=torch.int64, device=xyz.device), I, deg, min_samples, min_points)
    return (comp[0], flag) if return_flag else comp[0]


# ---- instances joined across the tiles of a large scan (csrc/tile_merge.hip) ---------------------------------------------
TILE_SCENE_FIELDS = _abi.const("GF_TILE_SCENE_FIELDS")
TILE_MAX_ROWS = 4096   # gf_tile_merge_max_rows(): asserted against the library in tile_limits()
TILE_MAX_PICKS = 256   # gf_tile_merge_max_picks()


def tile_limits():
    """(most rows in all, most picks in one tile) of the tile merge, from the library."""
    lib = _lib.load()
    lim = lib.gf_tile_merge_max_rows(), lib.gf_tile_merge_max_picks()
    if lim != (TILE_MAX_ROWS, TILE_MAX_PICKS):
        raise RuntimeError(f"tile merge: the library's limits {lim} are not {(TILE_MAX_ROWS, TILE_MAX_PICKS)}")
    return lim


def tile_check_caps(table_host):
    """The caps of the tile merge on a host tile scene table (postprocess.tile_scene_table), before any launch."""
    t = np.asarray(table_host)
    if t.ndim != 2 or t.shape[1] != TILE_SCENE_FIELDS or t.dtype != np.int64:
        raise RuntimeError(f"tile scene table: expected int64 [T, {TILE_SCENE_FIELDS}], got {t.dtype} {t.shape}")
    from . import postprocess

    p_s = postprocess.scene_rows(t, postprocess.TILE_ROW)["p_s"]
    most = int(p_s.max()) if len(t) else 0
    if most > TILE_MAX_PICKS:
        raise RuntimeError(f"tile merge: {most} picks in tile {int(p_s.argmax())} (at most {TILE_MAX_PICKS} per tile)")
    if int(p_s.sum()) > TILE_MAX_ROWS:
        raise RuntimeError(f"tile merge: {int(p_s.sum())} picked rows over {len(t)} tiles (at most {TILE_MAX_ROWS})")
    return int(p_s.sum())


def _tile_tables(table, table_host, tile_of, local_of, name):
    P = tile_check_caps(table_host)
    table_host = np.ascontiguousarray(table_host)
    if not (table.is_cuda and table.dtype == torch.int64 and table.is_contiguous()
            and tuple(table.shape) == table_host.shape):
        raise RuntimeError(f"{name}: table: expected a contiguous int64 tensor {table_host.shape} on the GPU")
    if tile_of is not None:
        _i32c(tile_of, "tile_of"); _i32c(local_of, "local_of")
        if tile_of.dim() != 2 or tile_of.shape[1] != 4 or local_of.shape != tile_of.shape:
            raise RuntimeError(f"{name}: expected tile_of and local_of [N, 4], got {tuple(tile_of.shape)}, "
                               f"{tuple(local_of.shape)}")
    return table_host, P


def tile_pack_picks(table, table_host, sizes):
    """bits int32 [words]: per tile-local point the bitset of its memberships in the tile's picked masks, ceil(p_s / 32)
    consecutive words (gf_tile_pack_picks; table / table_host / sizes: postprocess.tile_scene_table on the device and
    on the host).  One launch on the current stream."""
    table_host, P = _tile_tables(table, table_host, None, None, "tile_pack_picks")
    bits = torch.empty(max(int(sizes["words"]), 1), dtype=torch.int32, device=table.device)
    check(_lib.load().gf_tile_pack_picks(ptr(table), table_host.ctypes.data, table_host.shape[0], P, ptr(bits),
                                         stream_ptr()), "gf_tile_pack_picks")
    return bits


def tile_overlaps(table, table_host, tile_of, local_of, bits, P):
    """(inter int32 [P, P], shared int32 [P, T]) of postprocess.merge_tiles_host from the bitsets of tile_pack_picks and
    the plan's point tables (int32 [N, 4] on the device): gf_tile_overlaps, one launch after two memsets on the current
    stream, integer atomics only."""
    table_host, rows = _tile_tables(table, table_host, tile_of, local_of, "tile_overlaps")
    _i32c(bits, "bits")
    if rows != P:
        raise RuntimeError(f"tile_overlaps: the table holds {rows} rows, P = {P}")
    T = table_host.shape[0]
    inter = torch.empty((P, P), dtype=torch.int32, device=table.device)
    shared = torch.empty((P, T), dtype=torch.int32, device=table.device)
    check(_lib.load().gf_tile_overlaps(ptr(table), table_host.ctypes.data, T, ptr(tile_of), ptr(local_of),
                                       tile_of.shape[0], ptr(bits), P, ptr(inter), ptr(shared), stream_ptr()),
          "gf_tile_overlaps")
    return inter, shared


def tile_merge(inter, shared, cls, scores, row_tile, iom=0.5, min_shared=20):
    """(comp int32 [P], members int32 [P], G int32 [1], cls int64 [P], scores fp32 [P]; the first G of the last two are
    the instances') from the overlap tables: the connected components of postprocess.merge_tiles_host's edges, one
    launch of one workgroup (gf_tile_merge).  cls int64 [P], scores fp32 [P], row_tile int32 [P]."""
    _i32c(inter, "inter"); _i32c(shared, "shared"); _f32c(scores, "scores"); _i32c(row_tile, "row_tile")
    P = scores.shape[0]
    if P > TILE_MAX_ROWS:
        raise RuntimeError(f"tile_merge: {P} rows (at most {TILE_MAX_ROWS})")
    if not (cls.is_cuda and cls.dtype == torch.int64 and cls.is_contiguous()):
        raise RuntimeError("tile_merge: cls: expected a contiguous int64 tensor on the GPU")
    if inter.shape != (P, P) or shared.dim() != 2 or shared.shape[0] != P or cls.shape != (P,) or row_tile.shape != (P,):
        raise RuntimeError(f"tile_merge: expected inter [{P}, {P}], shared [{P}, T], cls [{P}] and row_tile [{P}], got "
                           f"{tuple(inter.shape)}, {tuple(shared.shape)}, {tuple(cls.shape)}, {tuple(row_tile.shape)}")
    dev = scores.device
    ints = torch.empty((2, max(P, 1)), dtype=torch.int32, device=dev)
    d_G = torch.empty(1, dtype=torch.int32, device=dev)
    inst_cls = torch.empty(max(P, 1), dtype=torch.int64, device=dev)
    inst_scores = torch.empty(max(P, 1), dtype=torch.float32, device=dev)
    check(_lib.load().gf_tile_merge(ptr(inter), ptr(shared), ptr(cls), ptr(scores), ptr(row_tile), P, shared.shape[1],
                                    float(iom), int(min_shared), ptr(ints[0]), ptr(ints[1]), ptr(d_G), ptr(inst_cls),
                                    ptr(inst_scores), stream_ptr()), "gf_tile_merge")
    return ints[0, :P], ints[1, :P], d_G, inst_cls[:P], inst_scores[:P]


def tile_assemble(table, table_host, tile_of, local_of, bits, members, G):
    """(masks int32 [G, N], count int32 [G]): the union of the member rows of every instance over the scan's points,
    scattered through the bitsets (gf_tile_assemble: two memsets and one launch on the current stream; the call zeroes
    its outputs).  members int32 [P]: tile_merge's."""
    table_host, P = _tile_tables(table, table_host, tile_of, local_of, "tile_assemble")
    _i32c(bits, "bits"); _i32c(members, "members")
    N = tile_of.shape[0]
    if members.shape != (P,) or not 0 <= G <= P:
        raise RuntimeError(f"tile_assemble: expected members [{P}] and 0 <= G <= {P}, got {tuple(members.shape)}, G = {G}")
    masks = torch.empty((G, N), dtype=torch.int32, device=table.device)
    count = torch.empty(G, dtype=torch.int32, device=table.device)
    check(_lib.load().gf_tile_assemble(ptr(table), table_host.ctypes.data, table_host.shape[0], ptr(tile_of),
                                       ptr(local_of), N, ptr(bits), ptr(members), P, int(G), ptr(masks), ptr(count),
                                       stream_ptr()), "gf_tile_assemble")
    return masks, count


# ---- semantic scores stitched across the tiles of a large scan (csrc/tile_stitch.hip) ------------------------------------
TILE_SCORE_FIELDS = _abi.const("GF_TILE_SCORE_FIELDS")
TILE_STITCH_MODES = {"core": _abi.const("GF_TILE_STITCH_CORE"), "mean": _abi.const("GF_TILE_STITCH_MEAN")}
TILE_STITCH_MAX_CLASSES = 64  # gf_tile_stitch_max_classes(): asserted against the library in tile_stitch_limits()


def tile_stitch_limits():
    """The largest class count of the tile stitch, from the library (that of gf_semantic_confusion)."""
    cap = _lib.load().gf_tile_stitch_max_classes()
    if cap != TILE_STITCH_MAX_CLASSES:
        raise RuntimeError(f"tile stitch: the library's cap {cap} is not {TILE_STITCH_MAX_CLASSES}")
    return cap


def tile_stitch_scores(table, table_host, tile_of, local_of, core_of, C, mode):
    """out fp32 [N, C]: the scan's per-point scores from its tiles' (gf_tile_stitch_scores, the statement is
    postprocess.stitch_tiles_host): one launch on the current stream, no memset, no atomics, nothing read back.  table /
    table_host: int64 [T, GF_TILE_SCORE_FIELDS] (postprocess.tile_score_table) on the device and on the host;
    tile_of, local_of int32 [N, 4] and core_of int32 [N] on the device: the plan's point tables; mode "core" or "mean".
    Shapes that disagree or C above the cap raise before anything is launched."""
    if mode not in TILE_STITCH_MODES:
        raise ValueError(f"tile_stitch_scores: mode must be one of {tuple(TILE_STITCH_MODES)}, got {mode!r}")
    t = np.asarray(table_host)
    if t.ndim != 2 or t.shape[1] != TILE_SCORE_FIELDS or t.dtype != np.int64 or t.shape[0] < 1:
        raise RuntimeError(f"tile_stitch_scores: table_host: expected int64 [T >= 1, {TILE_SCORE_FIELDS}], got {t.dtype} "
                           f"{t.shape}")
    table_host = np.ascontiguousarray(t)
    if not (table.is_cuda and table.dtype == torch.int64 and table.is_contiguous()
            and tuple(table.shape) == table_host.shape):
        raise RuntimeError(f"tile_stitch_scores: table: expected a contiguous int64 tensor {table_host.shape} on the GPU")
    _i32c(tile_of, "tile_of"); _i32c(local_of, "local_of"); _i32c(core_of, "core_of")
    if tile_of.dim() != 2 or tile_of.shape[1] != 4 or local_of.shape != tile_of.shape \
            or core_of.shape != (tile_of.shape[0],):
        raise RuntimeError(f"tile_stitch_scores: expected tile_of and local_of [N, 4] and core_of [N], got "
                           f"{tuple(tile_of.shape)}, {tuple(local_of.shape)}, {tuple(core_of.shape)}")
    C = int(C)
    if not 1 <= C <= TILE_STITCH_MAX_CLASSES:
        raise RuntimeError(f"tile_stitch_scores: C = {C} classes (1 to {TILE_STITCH_MAX_CLASSES})")
    N = tile_of.shape[0]
    out = torch.empty((N, C), dtype=torch.float32, device=table.device)
    check(_lib.load().gf_tile_stitch_scores(ptr(table), table_host.ctypes.data, table_host.shape[0], ptr(tile_of),
                                            ptr(local_of), ptr(core_of), N, C, TILE_STITCH_MODES[mode], ptr(out),
                                            stream_ptr()), "gf_tile_stitch_scores")
    return out


# ---- scans of any density: grid subsample and nearest point (csrc/resample.hip) ------------------------------------------
GRID_MODES = {"first": 0, "center": 1}  # gf_grid_subsample's mode
RESAMPLE_MAX_POINTS = 1 << 29           # gf_resample_max_points(): asserted against the library in resample_limits()
GRID_AXIS_CELLS = 1 << 21               # gf_grid_subsample_max_cells()
NEAREST_MAX_CELLS = float(1 << 30)      # gf_nearest_point_max_cells()


def resample_limits():
    """(most points of a set, cells per axis of the subsample, cells per axis the nearest-point walk is proven for), from
    the library."""
    lib = _lib.load()
    lim = lib.gf_resample_max_points(), lib.gf_grid_subsample_max_cells(), lib.gf_nearest_point_max_cells()
    assert lim == (RESAMPLE_MAX_POINTS, GRID_AXIS_CELLS, NEAREST_MAX_CELLS), lim
    return lim


def _xyz3(t, name, device=None):
    if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 3 or not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous float32 tensor [n, 3], got "
                         f"{(t.dtype, tuple(t.shape)) if torch.is_tensor(t) else type(t).__name__}")
    if device is not None and t.device != device:
        raise ValueError(f"{name}: expected a tensor on {device}, got {t.device}")
    if t.shape[0] > RESAMPLE_MAX_POINTS:
        raise ValueError(f"{name}: {t.shape[0]} points (at most {RESAMPLE_MAX_POINTS})")
    return t


def grid_subsample(xyz, cell, mode="center", origin=None):
    """(rep int32 [M], cell_of int32 [N], count int32 [M]) of postprocess.grid_subsample_host on xyz's device: one
    representative -- a real point -- per occupied cell of a grid of `cell` metres, the cells numbered in order of first
    occurrence.  xyz fp32 [N, 3]; origin: fp32 [3] tensor on the same device (None: the minimum corner, found on the
    device).  On the GPU: gf_grid_subsample on the current stream, bit-identical to the statement and from call to call;
    the two words {M, invalid} are read back once (the only synchronisation) and an invalid point -- not finite, below
    the origin, or 2^21 cells or more from it -- is a ValueError, as in the statement.  A CPU tensor runs the
    statement."""
    from . import postprocess

    _xyz3(xyz, "grid_subsample: xyz")
    c = postprocess._grid_args(cell, mode, "grid_subsample")
    if origin is not None and not (torch.is_tensor(origin) and origin.dtype == torch.float32 and origin.shape == (3,)
                                   and origin.is_contiguous() and origin.device == xyz.device):
        raise ValueError(f"grid_subsample: origin: expected a contiguous float32 tensor [3] on {xyz.device}")
    if not xyz.is_cuda:
        return tuple(torch.from_numpy(a) for a in postprocess.grid_subsample_host(xyz, c, mode, origin))
    N, dev = xyz.shape[0], xyz.device
    if N == 0:
        return tuple(torch.empty(0, dtype=torch.int32, device=dev) for _ in range(3))
    lib = _lib.load()
    out = torch.empty((3, N), dtype=torch.int32, device=dev)
    words = torch.empty(2, dtype=torch.int32, device=dev)
    ws = torch.empty(lib.gf_grid_subsample_scratch_bytes(N) // 8 + 1, dtype=torch.int64, device=dev)
    check(lib.gf_grid_subsample(ptr(xyz), N, float(c), GRID_MODES[mode], ptr(origin) if origin is not None else None,
                                ptr(ws), ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(words), stream_ptr()),
          "gf_grid_subsample")
    M, invalid = words.tolist()
    if invalid:
        raise ValueError(f"grid_subsample: a point lies outside the grid (not finite, below the origin or "
                         f"{GRID_AXIS_CELLS} cells or more from it)")
    return out[0, :M], out[1], out[2, :M]


def nearest_point(query, xyz, max_dist, check=True, return_flag=False):
    """(idx int32 [Q], d2 fp32 [Q]) of postprocess.nearest_point_host on the tensors' device: for every query the point
    of xyz minimising (d2, index) among those within max_dist, (-1, inf) without one.  On the GPU: gf_nearest_point on
    the current stream (a hash grid over xyz, 27 cells walked per query), bit-identical to the statement and from call
    to call.  The walk is proven complete while xyz's bounding box spans fewer than 2^30 cells of max_dist * 1.001 on
    every axis; the kernel raises a device flag beyond that, which `check` reads here (one read-back) and turns into a
    ValueError.  return_flag: also the flag (int32 [1], device; None on the CPU) for a caller who folds it into a
    read-back of their own -- with check=False nothing is read back.  A CPU tensor runs the statement."""
    from . import postprocess

    _xyz3(query, "nearest_point: query")
    _xyz3(xyz, "nearest_point: xyz", query.device)
    md = np.float32(max_dist)
    if not (md > 0 and np.isfinite(md)):
        raise ValueError(f"nearest_point: max_dist must be positive and finite in float32, got {max_dist!r}")
    if not query.is_cuda:
        idx, d2 = (torch.from_numpy(a) for a in postprocess.nearest_point_host(query, xyz, md))
        return (idx, d2, None) if return_flag else (idx, d2)
    Q, n, dev = query.shape[0], xyz.shape[0], query.device
    idx = torch.empty(Q, dtype=torch.int32, device=dev)
    d2 = torch.empty(Q, dtype=torch.float32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    if Q:
        lib = _lib.load()
        ws = torch.empty(lib.gf_nearest_point_scratch_bytes(n) // 8 + 1, dtype=torch.int64, device=dev)
        _lib.check(lib.gf_nearest_point(ptr(query), Q, ptr(xyz) if n else None, n, float(md), ptr(ws), ptr(idx), ptr(d2),
                                        ptr(flag), stream_ptr()), "gf_nearest_point")
        if check and int(flag.item()):
            raise ValueError(f"nearest_point: the points span {int(NEAREST_MAX_CELLS)} cells of max_dist or more on an "
                             f"axis, beyond the range the search is proven complete for")
    return (idx, d2, flag) if return_flag else (idx, d2)


# ---- 3D boxes of instances and the IoU of boxes (csrc/boxes.hip) ---------------------------------------------------------
def box_limits():
    """(points per workgroup chunk, most angles, most groups of a scene) of gf_instance_boxes_batched, from the library."""
    from .postprocess import BOX_MAX_ANGLES, BOX_MAX_GROUPS

    lib = _lib.load()
    lim = lib.gf_box_chunk(), lib.gf_box_max_angles(), lib.gf_box_max_groups()
    assert lim[1:] == (BOX_MAX_ANGLES, BOX_MAX_GROUPS), lim
    return lim


def instance_boxes_batched(table, sizes, angles):
    """gf_instance_boxes_batched on a device box scene table (postprocess.box_scene_table): (count int32 [rows], aligned
    float64 [rows, GF_BOX_FLOATS], oriented float64 [rows, GF_BOX_FLOATS]).  angles: fp32 [A, 2] (cos, sin) on the
    device.  Two memsets and two launches on the current stream, nothing read back."""
    from .postprocess import BOX_FLOATS

    _f32c(angles, "angles")
    dev = table.device
    rows, A = int(sizes["rows"]), angles.shape[0]
    lib = _lib.load()
    count = torch.empty(max(rows, 1), dtype=torch.int32, device=dev)
    out = torch.empty((2, max(rows, 1), BOX_FLOATS), dtype=torch.float64, device=dev)
    ws = torch.empty(lib.gf_instance_boxes_scratch_bytes(rows, A) // 8 + 1, dtype=torch.int64, device=dev)
    check(lib.gf_instance_boxes_batched(ptr(table), table.shape[0], int(sizes["max_points"]), int(sizes["max_groups"]),
                                        rows, ptr(angles), A, ptr(ws), ptr(count), ptr(out[0]), ptr(out[1]),
                                        stream_ptr()), "gf_instance_boxes_batched")
    return count[:rows], out[0, :rows], out[1, :rows]


def box_iou_batched(table, sizes, a, b):
    """gf_box_iou_batched on a device IoU table (postprocess.box_iou_table): float64 [sizes["out"]], every scene's
    [P, G] block at its offset.  a, b: packed boxes float64 [., GF_BOX_FLOATS] on the device.  One launch."""
    from .postprocess import BOX_FLOATS

    for t, name, rows in ((a, "a", sizes["a"]), (b, "b", sizes["b"])):
        if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and tuple(t.shape) == (rows, BOX_FLOATS)):
            raise RuntimeError(f"box_iou_batched: {name}: expected a contiguous float64 tensor [{rows}, {BOX_FLOATS}] on "
                               f"the GPU")
    n = int(sizes["out"])
    out = torch.empty(max(n, 1), dtype=torch.float64, device=table.device)
    check(_lib.load().gf_box_iou_batched(ptr(table), table.shape[0], int(sizes["max_pairs"]), ptr(a), ptr(b), ptr(out),
                                         stream_ptr()), "gf_box_iou_batched")
    return out[:n]
