"""GeoFormer on MI355X: the build's counterpart of ``model/geoformer/geoformer.py``.

Same class name, ``forward(batch_input, epoch, training=True)`` signature, output-dict keys,
``state_dict`` names/shapes and yaml keys as the reference (geoformer.py:23-662), so its drivers
(train.py:63, test.py:56) and checkpoints can be pointed at this class unchanged.  The native
work runs in libgeoformer_hip.so: voxel mean, rulebooks + gather-MFMA sparse convolutions, FPS,
ball query, grouping, the kNN graph and the frontier BFS.  The reference's index-space quirk
(FPS indices taken on the permuted points but applied to the un-permuted ones)
and its host-RNG draws are reproduced deliberately.
"""
from __future__ import annotations

import functools
import os

import numpy as np
import torch
import torch.nn as nn
from torch.nn import functional as F

from .. import _lib, pointops, spconv, unet_exec, unet_train
from . import config as _config
from .backbone import ResidualBlock, UBlock, conv1d_bn_relu, random_downsample
from .layers import (BatchNorm1d, BigLinear, GenericMLP, LazyRelPos, PointwiseConv1d, PositionEmbeddingCoordsSine, RelPosSpec,
                     TransformerDecoder,
                     TransformerDecoderLayer, scene_counts)
from .set_abstraction import PointnetSAModuleVotesSeparate


class _Voxelization(torch.autograd.Function):
    """pointgroup_ops.voxelization (lib/pointgroup_ops/functions/pointgroup_ops.py:42-72)."""

    @staticmethod
    def forward(ctx, feats, map_rule, mode=4):
        ctx.rule, ctx.mode, ctx.N = map_rule, mode, feats.shape[0]
        return pointops.voxelize_fp(feats.contiguous(), map_rule, mode)

    @staticmethod
    def backward(ctx, d_out):
        d_feats = torch.zeros((ctx.N, d_out.shape[1]), dtype=torch.float32, device=d_out.device)
        pointops.voxelize_bp(d_out.contiguous(), ctx.rule, ctx.mode, d_feats)
        return d_feats, None, None


voxelization = _Voxelization.apply


import threading
import weakref


def _bfs_wg(nq, scenes=1):
    """1024 threads per query (the kernel's fastest layout: 1.06 against 1.25 ms at 512) when the workgroups of the
    scenes' launches -- they run beside each other on streams of their own -- fit the compute units the sampling
    kernels leave free in one round: the train yaml's 128 queries on one scene, the few-shot model's; 512 (two queries
    share a unit) for the test yaml's 256 queries and for a training batch (4 x 128 queries: 56.3 -> 52.9 ms per step;
    256 threads: 57.1)."""
    return 1024 if nq * scenes <= 224 else 512
# Side streams of the sampling / BFS stretch, keyed by (device, caller stream, role): a process resource, not a model's --
# a second model instance taking fresh streams from the framework's pool measured 6.0 against 4.5 ms per scene on the
# nq = 128 forward (bench.py's secondary leg; which hardware queue a stream lands on depends on what was created before it)
_SIDE_STREAMS = {}
_OFFS_CACHE = threading.local()  # per thread: concurrent scenes run on separate host threads / streams


def get_batch_offsets(batch_idxs, bs, host_only=False):
    """offsets[i+1] = offsets[i] + count(batch_idxs == i)  (util/utils.py:132-142), one device op.
    host_only (one scene): the offsets tensor stays on the host -- every reader of the eval forward wants host integers,
    and creating a two-element device tensor is a synchronous 40 us copy in a launch-bound stretch."""
    if bs == 1:
        # one scene: the offsets are known on the host, no device round trip when they are read back
        n = int(batch_idxs.shape[0])
        t = torch.tensor([0, n], dtype=torch.int32, device="cpu" if host_only else batch_idxs.device)
        _OFFS_CACHE.key, _OFFS_CACHE.val = t, [0, n]
        return t
    counts = scene_counts(batch_idxs, bs)
    return torch.cat([counts.new_zeros(1), counts.cumsum(0)]).int()



def _offsets_list(t):
    """Host copy of a small offsets tensor, fetched once per tensor object (each fetch from the device is a
    synchronisation: a serving loop that re-uses its batch dicts must not pay it per forward, and one forward reads two
    different offsets tensors -- the batch's and the foreground's -- alternately)."""
    if getattr(_OFFS_CACHE, "key", None) is t:
        return _OFFS_CACHE.val
    lru = getattr(_OFFS_CACHE, "lru", None)
    if lru is None:
        lru = _OFFS_CACHE.lru = {}
    hit = lru.get(id(t))
    if hit is not None and hit[0]() is t and hit[1] == t._version:
        return hit[2]
    val = t.tolist()
    if len(lru) > 64:
        lru.clear()
    lru[id(t)] = (weakref.ref(t), t._version, val)
    return val


def _tensors_of(obj):
    """All tensors inside nested tuples / lists (for record_stream)."""
    if torch.is_tensor(obj):
        yield obj
    elif isinstance(obj, (tuple, list)):
        for o in obj:
            yield from _tensors_of(o)


@torch.no_grad()
def knn_graphs(locs_float_, batch_offsets_, batch_size, neighbor=64, radius=0.05):
    """Per scene the radius-limited kNN graph of the foreground points (find_knn + the radius filter of
    geodesic_utils.py:11-24,110-125).  Depends on the points only, so the forward issues it before the
    host-side RNG draw and FPS."""
    offs = _offsets_list(batch_offsets_)
    return [pointops.knn_radius(locs_float_[offs[b]:offs[b + 1]].contiguous(), neighbor, radius, sqrt_out=True,
                                return_flag=True)
            for b in range(batch_size)]


def knn_truncated(graphs):
    """One device word (int32 [1]) that is non-zero when a scene's kNN rows were cut at the kernel's candidate list
    (rows are then no longer the k nearest: wrong geodesic distances).  A copy: the per-scene flags are views of the
    kNN scratch buffers, which must not be kept alive by them.  None without graphs / flags (host operators)."""
    fl = [g[3] for g in (graphs or ()) if len(g) > 3]
    return torch.stack([f.reshape(()) for f in fl]).amax().reshape(1) if fl else None


@torch.no_grad()
def cal_geodesic(pre_enc_inds, locs_float_, batch_offsets_, max_step=128, neighbor=64, radius=0.05, n_queries=128,
                 graphs=None):
    """cal_geodesic_vectorize (geodesic_utils.py:91-164): per scene a kNN graph (k=neighbor, edges
    within `radius`) and a hop-synchronous BFS from the first n_queries FPS indices -- interpreted,
    like the reference does, as indices into the scene's un-permuted foreground points."""
    if graphs is None:
        graphs = knn_graphs(locs_float_, batch_offsets_, pre_enc_inds.shape[0], neighbor, radius)
    out = []
    for b in range(pre_enc_inds.shape[0]):
        D, I, deg = graphs[b][:3]
        src = pre_enc_inds[b][:n_queries].int().contiguous()
        out.append(pointops.geodesic_bfs(D, I, deg, src, radius, max_step))
    return out


def _stream_key_of(device, stream):
    """_stream_key() of an explicit (device, torch stream)."""
    idx = torch.device(device).index
    return (torch.cuda.current_device() if idx is None else idx, stream.cuda_stream)


def _stream_key(device=None):
    """(device, stream) the caller is running on: the forward's in-flight side-stream state is kept per caller
    stream, so scenes queued from different host threads / streams on ONE model never pick up each other's events."""
    raw = getattr(torch._C, "_cuda_getCurrentRawStream", None)
    if raw is not None:  # (constructing a torch.cuda.Stream object costs ~8 us, this is called ~10 times per forward)
        idx = torch.cuda.current_device() if device is None else torch.device(device).index
        if idx is None:
            idx = torch.cuda.current_device()
        return (idx, raw(idx))
    st = torch.cuda.current_stream(device)
    return (st.device.index, st.cuda_stream)


def _segments_arg(segments, n_points=None):
    """The batch dict's "segments" (or None): int32 [N], one over-segment id per point of the batch."""
    if segments is None:
        return None
    if not torch.is_tensor(segments) or segments.dtype != torch.int32:
        raise TypeError(f'"segments": expected an int32 tensor [N], one id per point of the batch, got '
                        f"{segments.dtype if torch.is_tensor(segments) else type(segments).__name__}")
    if segments.dim() != 1 or (n_points is not None and segments.shape[0] != n_points):
        raise ValueError(f'"segments": expected [{n_points if n_points is not None else "N"}], one id per point of the '
                         f"batch, got {tuple(segments.shape)}")
    return segments


class PendingProposals:
    """The tail of generate_proposal (geoformer.py:236-262) behind the forward's last device->host read-back.  The
    accepted queries are compacted on the device (indices, classes, scores); only their NUMBER travels to a pinned
    host word.  ``get()`` waits for it and queues the membership scatter on the stream the forward ran on."""

    _pinned = []
    _lock = threading.Lock()

    def __init__(self, final, cls_pred, scores, logits, fg_idxs, logit_thresh, num_points, knn_flags=()):
        self.stream = torch.cuda.current_stream(logits.device)
        sel, cls, sc, cnt = pointops.proposal_select(final.contiguous(), cls_pred.contiguous(), scores.contiguous())
        self.args = (sel, cls, sc, logits, fg_idxs, logit_thresh, num_points)
        with PendingProposals._lock:
            buf = PendingProposals._pinned.pop() if PendingProposals._pinned else None
        if buf is None:
            buf = torch.zeros(2, dtype=torch.int32).pin_memory()
        buf[1] = 0
        buf[0:1].copy_(cnt, non_blocking=True)
        # the kNN graph's truncation flag (more in-radius candidates than the kernel's list holds: rows would no
        # longer be the nearest neighbours) rides in the same read-back instead of costing one of its own
        for f in knn_flags:
            buf[1:2].copy_(f, non_blocking=True)
        self.host = buf
        self.done = torch.cuda.Event()
        self.done.record(self.stream)
        self.value = None
        self.home = None  # the caller's stream when this object lives on a side stream (generate_proposal)

    def get(self):
        if self.value is None:
            sel, cls, sc, logits, fg_idxs, logit_thresh, num_points = self.args
            _lib.timed_wait(self.done)
            n, overflow = int(self.host[0]), int(self.host[1])
            with PendingProposals._lock:
                PendingProposals._pinned.append(self.host)
            self.host = None
            if overflow:
                from .._lib import GeoFormerHipError

                raise GeoFormerHipError("kNN graph: a point has more in-radius neighbours than the kernel's candidate list "
                                        "holds (1024); its row is not the 64 nearest and the geodesic distances "
                                        "would be wrong -- deduplicate the scene's points")
            if n == 0:
                self.value = ([], [], [])
            else:
                with torch.cuda.stream(self.stream):
                    proposals = pointops.proposal_scatter(logits, sel[:n], fg_idxs, logit_thresh, num_points)
                self.value = (cls[:n], sc[:n], proposals)
                if self.home is not None:
                    # the scatter ran on the side stream: whoever reads the result on the stream that is current now
                    # waits for it there
                    cur = torch.cuda.current_stream(logits.device)
                    if cur.cuda_stream != self.stream.cuda_stream:
                        ev = torch.cuda.Event()
                        ev.record(self.stream)
                        cur.wait_event(ev)
                        for t in self.value:
                            t.record_stream(cur)
            self.args = None
        return self.value


class PendingBatchProposals:
    """Proposals of every scene of a batched eval forward (forward(..., all_scenes=True, defer_proposals=True)) behind
    ONE read-back: the per-scene accepted counts (and the kNN truncation flag) travel to a pinned buffer together;
    ``get()`` waits for them, queues the packed membership scatter of all scenes (csrc/batch_post.hip) and returns a
    list of B tuples (cls_final, scores_final, masks_final) -- ([], [], []) for a scene without proposals or without
    foreground.  ``value`` given: nothing is in flight (every scene was empty)."""

    def __init__(self, n_scenes, scene_ids=(), table=None, sel=None, cls=None, scores=None, counts=None, fg_idxs=None,
                 logit_thresh=0.5, num_points=(), max_N=0, knn_flags=(), value=None):
        self.value = value
        if value is not None:
            return
        self.n_scenes, self.scene_ids, self.num_points, self.max_N = n_scenes, list(scene_ids), list(num_points), max_N
        self.args = (table, sel, cls, scores, counts, fg_idxs, logit_thresh)
        S = len(self.scene_ids)
        self.stream = torch.cuda.current_stream(sel.device)
        self.host = torch.zeros(S + 1, dtype=torch.int32).pin_memory()
        self.host[:S].copy_(counts, non_blocking=True)
        for f in knn_flags:
            self.host[S:S + 1].copy_(f, non_blocking=True)
        self.done = torch.cuda.Event()
        self.done.record(self.stream)

    def get(self):
        if self.value is None:
            from .. import postprocess

            table, sel, cls, scores, counts, fg_idxs, logit_thresh = self.args
            _lib.timed_wait(self.done)
            S = len(self.scene_ids)
            h = self.host.tolist()
            counts_h, overflow = h[:S], h[S]
            if overflow:
                from .._lib import GeoFormerHipError

                raise GeoFormerHipError("kNN graph: a point has more in-radius neighbours than the kernel's candidate list "
                                        "holds (1024); its row is not the 64 nearest and the geodesic distances "
                                        "would be wrong -- deduplicate the scene's points")
            rows, elems = postprocess.packed_layout(counts_h, self.num_points)
            out = [([], [], []) for _ in range(self.n_scenes)]
            if rows[-1] > 0:
                with torch.cuda.stream(self.stream):
                    packed = pointops.proposal_scatter_batched(table, sel, counts, int(rows[-1]), int(elems[-1]),
                                                               self.max_N, fg_idxs, logit_thresh)
                masks = postprocess.split_packed(packed, counts_h, self.num_points)
                for k, b in enumerate(self.scene_ids):
                    c = counts_h[k]
                    if c:
                        out[b] = (cls[k, :c], scores[k, :c], masks[k])
            self.value, self.args, self.host = out, None, None
        return self.value


class SplitForward:
    """Handle of GeoFormer.forward_split, a forward in three parts, all queued on the stream that is current when the
    handle is created (the scene's lane):
      1. (constructor) backbone + semantic head queued; ``backbone_done`` is the event behind them;
      2. ``advance()``: foreground selection (the forward's host read-back), sampling / BFS stretch, set abstraction;
         ``stretch_done`` are the events behind the stretch (end of the sampling, end of every scene's BFS);
      3. ``finish()``: decoder, mask head, proposals -- launched in the co-resident workgroup shapes
         (pointops.co_resident_launches), because a serving loop queues this part behind the NEXT scene's
         ``backbone_done`` so that it runs under that scene's sampling / BFS stretch; returns the outputs.
    A forward that ends early (no foreground, ``epoch <= prepare_epochs``) has its outputs after whichever call saw it
    end; the later calls are no-ops."""

    def __init__(self, steps):
        self._steps, self.outputs, self.backbone_done, self.stretch_done = steps, None, None, ()
        self.backbone_done = self._next()

    def _next(self):
        if self._steps is None:
            return None
        try:
            return next(self._steps)
        except StopIteration as done:
            self.outputs, self._steps = done.value, None
            return None

    def advance(self):
        self.stretch_done = self._next() or ()
        return self

    def finish(self):
        if self._steps is not None:
            with pointops.co_resident_launches():
                self._next()
            if self._steps is not None:
                raise RuntimeError("SplitForward: the forward has more parts than this handle knows")
        return self.outputs


class GeoFormer(nn.Module):
    def __init__(self, cfg=None):
        super().__init__()
        cfg = cfg if cfg is not None else _config.cfg
        self.cfg = cfg
        input_c = cfg.input_channel + (3 if cfg.use_coords else 0)
        m, classes = cfg.m, cfg.classes
        self.prepare_epochs = cfg.prepare_epochs
        self.rank_agreement = None  # set by parallel.convert_sync_batchnorm: callable(flag, device) -> bool over all ranks
        self.fix_module = list(cfg.fix_module)
        norm_fn = functools.partial(BatchNorm1d, eps=1e-4, momentum=0.1)

        # sparse-voxel U-Net
        self.input_conv = spconv.SparseSequential(
            spconv.SubMConv3d(input_c, m, kernel_size=3, padding=1, bias=False, indice_key="subm1"))
        self.unet = UBlock([m * (i + 1) for i in range(7)], norm_fn, 2, ResidualBlock,
                           use_backbone_transformer=True, indice_key_id=1)
        self.output_layer = spconv.SparseSequential(norm_fn(m), nn.ReLU())

        # semantic head
        # (BigLinear = nn.Linear with a split-K weight gradient: these run over every point of the batch)
        self.semantic = nn.Sequential(BigLinear(m, m, bias=True), norm_fn(m), nn.ReLU(),
                                      BigLinear(m, m, bias=True), norm_fn(m), nn.ReLU())
        self.semantic_linear = BigLinear(m, classes, bias=True)

        # mask features, controller of the dynamic convolution
        self.output_dim = m
        self.mask_conv_num = 3
        tower = [conv1d_bn_relu(m, m) for _ in range(self.mask_conv_num)]
        tower.append(PointwiseConv1d(m, self.output_dim, 1))
        self.add_module("mask_tower", nn.Sequential(*tower))
        self.add_module("before_embedding_tower", nn.Sequential(conv1d_bn_relu(cfg.dec_dim, self.output_dim)))
        self.use_coords = True
        self.embedding_conv_num = 2
        od = self.output_dim
        self.weight_nums = [(od + 3) * od, od]
        self.bias_nums = [od, 1]
        self.num_gen_params = sum(self.weight_nums) + sum(self.bias_nums)
        self.controller = PointwiseConv1d(od, self.num_gen_params, kernel_size=1)
        nn.init.normal_(self.controller.weight, std=0.01)
        nn.init.constant_(self.controller.bias, 0)

        # set aggregation, positional embedding, decoder
        self.set_aggregator = PointnetSAModuleVotesSeparate(radius=0.2, nsample=64, npoint=cfg.n_decode_point,
                                                            mlp=[m, 2 * m, 2 * m, 2 * m], normalize_xyz=True)
        self.pos_embedding = PositionEmbeddingCoordsSine(d_pos=cfg.dec_dim, pos_type="fourier", normalize=True)
        layer = TransformerDecoderLayer(d_model=cfg.dec_dim, nhead=cfg.dec_nhead, dim_feedforward=cfg.dec_ffn_dim,
                                        dropout=cfg.dec_dropout, normalize_before=True, use_rel=True)
        self.decoder = TransformerDecoder(layer, num_layers=cfg.dec_nlayers, return_intermediate=True)
        self.query_projection = GenericMLP(input_dim=cfg.dec_dim, hidden_dims=[cfg.dec_dim], output_dim=cfg.dec_dim,
                                           use_conv=True, output_use_activation=True, hidden_use_bias=True)
        self.encoder_to_decoder_projection = GenericMLP(
            input_dim=2 * m, hidden_dims=[2 * m], output_dim=cfg.dec_dim, norm_fn_name="bn1d", activation="relu",
            use_conv=True, output_use_activation=True, output_use_norm=True, output_use_bias=False)
        self.detr_sem_head = GenericMLP(input_dim=cfg.dec_dim, hidden_dims=[cfg.dec_dim, cfg.dec_dim],
                                        norm_fn_name="bn1d", activation="relu", use_conv=True, output_dim=classes)

        self.apply(self.set_bn_init)
        for name in self.fix_module:
            if hasattr(self, name):  # subclasses add modules and repeat the freeze
                for p in getattr(self, name).parameters():
                    p.requires_grad = False

    # -- reference quirks kept on purpose -----------------------------------------------------
    def train(self, mode=True):
        """Frozen sub-modules stay in eval mode; returns None like the reference (geoformer.py:179-184)."""
        super().train(mode)
        for name in self.fix_module:
            if hasattr(self, name):
                for mod in getattr(self, name).modules():
                    mod.eval()

    @staticmethod
    def set_bn_init(mod):
        if mod.__class__.__name__.find("BatchNorm1d") != -1:
            mod.weight.data.fill_(1.0)
            mod.bias.data.fill_(0.0)

    @torch.no_grad()
    def reserve_for(self, max_points, epoch=300):
        """Serving warm-up: one eval forward of a synthetic scene of ``max_points`` points (the yaml's ``max_npoint`` is
        the natural bound), so that the framework's caching allocator holds device blocks large enough for every scene
        up to that size.  Without it a scene larger than any seen before makes the allocator call hipMalloc for its
        largest buffers in the middle of the forward -- 20-30 ms per call on a fast host, several times that on a slow
        one (bench.py secondary.fresh_scenes: 5.5 against 9.3 ms per never-before-seen scene on such a box).  The
        foreground-sized buffers follow the scene's content, not its point count: bound generously (a 1.3x bound left 6
        small hipMalloc calls to 24 fresh scenes of up to 1.28x, the yaml's 250 000 two).  Uses the process's numpy
        generator state and restores it."""
        import numpy as np

        from .. import scene

        dev = next(self.parameters()).device
        b = scene.make_batch([scene.make_scene(int(max_points), 987654)])
        b = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in b.items()}
        state = np.random.get_state()
        was_training = self.training
        try:
            torch.nn.Module.train(self, False)
            with torch.no_grad():
                if dev.type == "cuda":
                    # two scenes of that size back to back, the first one's outputs still alive while the second runs --
                    # what a serving loop that collects scene i's proposals after issuing scene i+1 holds at its peak
                    outs = [self(b, epoch, training=False, defer_proposals=True) for _ in range(2)]
                    for o in outs:
                        ps = o.get("proposal_scores") if isinstance(o, dict) else None
                        if ps is not None and hasattr(ps, "get"):
                            ps.get()
                    del outs
                    torch.cuda.synchronize(dev)
                else:
                    self(b, epoch, training=False)
        finally:
            np.random.set_state(state)
            if was_training:
                self.train(True)

    def invalidate_fused_caches(self):
        """Drop every derived copy the fused inference paths keep (packed conv weights, folded BatchNorm, MLP chains,
        pointer tables).  They are re-derived automatically when a parameter's version counter changes
        (optimizer steps, load_state_dict, in-place ops); call this after editing parameters through ``.data``,
        which leaves the counter untouched."""
        from .. import pointops, sparse

        sparse._PACK_CACHE.clear()
        if torch.cuda.is_available() and torch.cuda.is_initialized():
            # the grow-only per-stream scratch blocks too (~0.8 GB per stream after a 150k-point scene): nothing else
            # returns them; behind a synchronise, since queued kernels may still use them
            torch.cuda.synchronize()
            pointops.release_scratch()
        for mod in self.modules():
            for key in ("_gf_chains", "_gf_chain_walks", "_gf_block", "_gf_block_t", "_gf_affine", "_gf_chain",
                        "_gf_chain_walk", "_gf_tr_params", "_gf_fused", "_gf_fused_params", "_wpack_key", "_wpack"):
                mod.__dict__.pop(key, None)

    def _grad_ctx(self, name):
        """no_grad for frozen sub-modules (geoformer.py:497,566).  The reference re-enables autograd for the others
        even when the caller runs under torch.no_grad() (eval); that only builds a graph nobody uses, so the
        caller's mode is respected here and the fused inference kernels stay eligible."""
        return torch.enable_grad if (name not in self.fix_module and torch.is_grad_enabled()) else torch.no_grad

    def _pointwise_chain(self, name, mods, x):
        """Inference on the GPU: the Conv1d(k=1)/Linear + BatchNorm1d + ReLU stack `mods` as one fused launch
        (csrc/pointwise_mlp.hip); None when the PyTorch modules have to run (training, CPU, odd widths)."""
        if torch.is_grad_enabled() or not x.is_cuda or x.shape[0] == 0:
            return None
        # the walk over the module tree is done once per stack (this runs in launch-bound stretches of the forward);
        # per call only the cheap part: BatchNorm modes and the parameters' version counters
        walks = self.__dict__.setdefault("_gf_chain_walks", {})
        walk = walks.get(name)
        if walk is None or any(a is not b for a, b in zip(walk[0], mods)):
            flat = [m for top in mods for _, m in top.named_modules(remove_duplicate=False)
                    if len(list(m.children())) == 0]
            walk = walks[name] = (list(mods), flat,
                                  [m for m in flat if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)],
                                  [p for m in flat for p in list(m.parameters()) + list(m.buffers())])
        _, flat, bns, params = walk
        if any(m.training for m in bns):
            return None
        key = (params[0].data_ptr(), sum([p._version for p in params]))
        cache = self.__dict__.setdefault("_gf_chains", {})
        hit = cache.get(name)
        if hit is None or hit[0] != key:
            chain = pointops.PointwiseChain(flat) if pointops.PointwiseChain.supported(flat) else None
            hit = (key, chain)
            cache[name] = hit
        return hit[1]

    # -- backbone ---------------------------------------------------------------------------
    def preprocess_input(self, batch_input, batch_size):
        ahead = self._inputs_ahead(batch_input)
        if ahead is not None:
            # (everything up to the SparseConvTensor on the executor's side stream, behind the batch's own events: the
            #  executor's rulebook launches follow on that stream, and the first convolution waits for the last of them)
            main, side, evs = ahead
            with torch.cuda.stream(side):
                for e in evs:
                    side.wait_event(e)
                x = self._preprocess(batch_input, batch_size)
            for t in (x.features, x.indices):
                t.record_stream(main)
            unet_exec.coords_ready_next(evs)
            return x
        return self._preprocess(batch_input, batch_size)

    def _preprocess(self, batch_input, batch_size):
        feats = batch_input["feats"]
        if self.cfg.use_coords:
            feats = torch.cat((feats, batch_input["locs_float"]), 1).float()
        voxel_feats = voxelization(feats, batch_input["v2p_map"], self.cfg.mode)
        return spconv.SparseConvTensor(voxel_feats, batch_input["voxel_locs"].int().contiguous(), batch_input["spatial_shape"],
                                       batch_size)

    def _inputs_ahead(self, batch_input):
        """A batch that says what its tensors wait for -- ``batch_input["inputs_event"]``: a sequence of recorded events,
        empty for tensors that have been resident all along (bench.py's scenes; DeviceFeeder hands over its own event) --
        lets the head of the backbone (voxel features, int32 coordinates, every rulebook launch) start without waiting for
        what the caller's stream still has queued: unet_exec.coords_ready_next / gf_unet_fwd_ahead.  Returns
        (caller's stream, side stream, events) or None: the plain route."""
        evs = batch_input.get("inputs_event") if isinstance(batch_input, dict) else None
        locs = batch_input["voxel_locs"]
        if evs is None or not locs.is_cuda or torch.is_grad_enabled() or os.environ.get("GF_UNET_EXEC", "1") == "0":
            return None
        if unet_exec.phase_pending():
            return None  # (the staggered loop's phased call orders its rulebooks itself)
        main = torch.cuda.current_stream(locs.device)
        if main.query():
            # nothing queued on the caller's stream (a loop that waits for every scene's results): there is nothing to get
            # ahead of, and the cross-stream hand-overs of the route below only cost (-1.5 ... -2.7 % on bench.py's
            # synchronous_no_deferral / test_py_shape legs with them, +1.0 % on the headline loop: alternating runs)
            return None
        return main, unet_exec.side_stream_for(locs.device, main), list(evs)

    def unet_features(self, x, batch_size):
        """input_conv -> unet -> output_layer on a SparseConvTensor (geoformer.py:398-401); returns it with the output
        features.  Inference on the GPU: rulebooks, the 71 convolutions and the two voxel transformers issued by one
        native call (csrc/unet_exec.hip) -- the same launches as the module tree, without the host side of ~150 of
        them; otherwise the module tree."""
        if os.environ.get("GF_UNET_EXEC", "1") != "0" and unet_exec.supported(self, x.features, x.spatial_shape):
            x.features = unet_exec.unet_forward(self, x.features.contiguous(), x._coords(), batch_size, x.spatial_shape)
            return x
        if unet_exec.take_coords_ready() is not None:
            # (a request of _inputs_ahead the executor will not serve: the module tree reads the coordinates on this stream)
            torch.cuda.current_stream().wait_stream(unet_exec.side_stream_for(x.features.device))
        sig = unet_train.supported(self, x)
        if sig:
            # training: the same launches as the module tree below, forward and backward, issued by native code
            # (csrc/unet_train.hip); the two voxel transformers stay framework modules between its three ranges
            feats = unet_train.unet_forward(self, x, batch_size, sig)
            if feats is not None:
                x.features = feats
                return x
        # built lazily by the first strided convolution (spconv.SparseConv3d.get_rules): the host then issues
        # the chain's ~50 small launches while the GPU is busy with the level-1 blocks, and the one read-back
        # of the voxel counts waits behind real work instead of an empty queue
        x.indice_dict["_prebuild"] = self.prebuild_rulebooks
        return self.output_layer(self.unet(self.input_conv(x)))

    def forward_backbone(self, batch_input, batch_size, want_preds=True):
        ctx = self._grad_ctx("unet")
        with ctx():
            x = self.unet_features(self.preprocess_input(batch_input, batch_size), batch_size)
            return self._semantic_head(x, batch_input, want_preds)

    def _semantic_head(self, x, batch_input, want_preds):
        """Voxel -> point gather and the semantic head (geoformer.py:541-547) behind either backbone route."""
        p2v = batch_input["p2v_map"]
        if not want_preds and p2v.dtype == torch.int32 and p2v.is_contiguous():
            # fused inference: nobody needs feats[p2v_map] as a tensor -- the semantic head and the foreground
            # compaction read the voxel rows through the map (returned as (voxel features, map))
            vox = x.features.contiguous()
            chain = self._pointwise_chain("semantic", [self.semantic, self.semantic_linear], vox)
            if chain is not None:
                return (vox, p2v), pointops.pointwise_mlp(vox, chain, rows=p2v), None
        output_feats = pointops.points_from_voxels(x.features, p2v, batch_input.get("v2p_map")).contiguous()
        chain = self._pointwise_chain("semantic", [self.semantic, self.semantic_linear], output_feats)
        if chain is not None:
            semantic_scores = pointops.pointwise_mlp(output_feats, chain)
        else:
            semantic_scores = self.semantic_linear(self.semantic(output_feats))
        semantic_preds = semantic_scores.max(1)[1] if want_preds else None
        return output_feats, semantic_scores, semantic_preds

    @staticmethod
    def prebuild_rulebooks(x, nlevels=6):
        """All six down-sampling rulebooks of the U-Net in one go (one host sync instead of six); the
        SparseConv3d layers find them in the shared indice_dict under their ``spconvL`` keys."""
        from .. import sparse

        if not x.features.is_cuda or x.indices.shape[0] == 0:
            return
        coords = x._coords()
        chain = sparse.down_rules_chain(coords, x.batch_size, x.spatial_shape, nlevels)
        cur = coords
        for l, r in enumerate(chain):
            r.prebuilt_for = cur.data_ptr()
            x.indice_dict[f"spconv{l + 1}"] = r
            cur = r.out_coords

    def _mask_tower_rows(self, feats):
        """Training on the GPU: the mask tower (Conv1d(k=1) + BatchNorm1d + ReLU three times + Conv1d, geoformer.py:64-70)
        evaluated on the point ROWS [N_fg, 16] -- the k=1 convolutions are row GEMMs with the same weights, the
        BatchNorm + ReLU pairs the row-major training kernels (csrc/bn_train.hip) -- instead of on the [1, 16, N_fg]
        layout of the module tree, which costs two transposes of the whole tensor per direction and the channel-major
        BatchNorm form.  Same parameters, same running statistics, autograd through every op.  None: not applicable."""
        if not (feats.is_cuda and torch.is_grad_enabled() and feats.dim() == 2 and feats.dtype == torch.float32
                and os.environ.get("GF_FUSED_BN", "1") != "0"):
            return None
        from .layers import _SplitKLinearFn

        mods = list(self.mask_tower)
        x = feats.contiguous()
        last = mods[-1]
        # (the whole structure is checked before anything runs: a stage must not update its running statistics and then
        # hand the tensor back to the module route)
        if not (isinstance(last, nn.Conv1d) and last.kernel_size == (1,)):
            return None
        for mod in mods[:-1]:
            if not (isinstance(mod, nn.Sequential) and len(mod) == 3 and isinstance(mod[0], nn.Conv1d)
                    and mod[0].kernel_size == (1,) and mod[0].bias is None and isinstance(mod[2], nn.ReLU)
                    and isinstance(mod[1], nn.BatchNorm1d) and mod[1].num_features == mod[0].out_channels
                    and pointops.bn_relu_train_supported(
                        mod[1], x if mod[0].out_channels == x.shape[1] else x.new_empty((x.shape[0], mod[0].out_channels)))):
                return None
        for mod in mods[:-1]:
            x = pointops.bn_relu_train(mod[1], _SplitKLinearFn.apply(x, mod[0].weight[:, :, 0], None))
        return _SplitKLinearFn.apply(x, last.weight[:, :, 0], last.bias).unsqueeze(2)  # [N_fg, output_dim, 1]

    # -- set aggregation ------------------------------------------------------------------------
    def forward_aggregator(self, locs_float_, output_feats_, batch_offsets_, batch_size):
        ctx = self._grad_ctx("set_aggregator")
        offs = _offsets_list(batch_offsets_)
        with ctx():
            locs, gfeat, gxyz, inds = [], [], [], []
            for b in range(batch_size):
                n_b = offs[b + 1] - offs[b]
                if n_b == 0:
                    return None
                npoint = min(n_b, self.cfg.n_downsampling)
                # host RNG, consumed exactly like the reference (geoformer.py:575-577): a random
                # permutation (and truncation) of the scene's foreground points
                draw = pointops.legacy_choice(n_b, npoint) if locs_float_.is_cuda else \
                    np.random.choice(n_b, npoint, replace=False)
                sampling_indices = torch.tensor(draw, dtype=torch.long, device=locs_float_.device)
                self.last_sampling_indices = sampling_indices
                xyz_b = locs_float_[offs[b]:offs[b + 1]][sampling_indices].unsqueeze(0)
                feat_b = output_feats_[offs[b]:offs[b + 1]][sampling_indices].unsqueeze(0)
                l, gf, gx, idx = self.set_aggregator.group_points(xyz_b.contiguous(),
                                                                  feat_b.transpose(1, 2).contiguous())
                locs.append(l); gfeat.append(gf); gxyz.append(gx); inds.append(idx)
            context_locs, pre_enc_inds = torch.cat(locs), torch.cat(inds)
            context_feats = self.set_aggregator.mlp(torch.cat(gfeat), torch.cat(gxyz)).transpose(1, 2)
            return context_locs, context_feats, pre_enc_inds

    def _sampling_split(self):
        """(n_query_points, the aggregator's npoint, whether the sampling is cut after the query picks)"""
        nq = self.cfg.n_query_points
        npoint_sa = self.set_aggregator.npoint
        return nq, npoint_sa, os.environ.get("GF_OVERLAP", "1") != "2" and npoint_sa > nq

    def _first_picks(self, xyz_b, sb, first=None, xyz_ready=None):
        """The sampling launches of one scene on stream `sb` (the current one): the query picks first, then -- queued right
        behind them, before the host spends ~60 us on anything else -- the rest (the stretch's long pole).  Returns
        (event: points ready, first picks, query picks, event: query picks ready, all picks, event: sampling done).
        first / xyz_ready: the first launch is already queued (pointops.draw_sample) / an event the points are ready by."""
        nq, npoint_sa, split = self._sampling_split()
        if xyz_ready is None:
            xyz_ready = torch.cuda.Event()
            xyz_ready.record(sb)
        if first is None:
            first = pointops.furthest_point_sampling(xyz_b, nq if split else npoint_sa)
        src = first[0, :nq].contiguous()
        first_ready = torch.cuda.Event()
        first_ready.record(sb)
        idx = pointops.furthest_point_sampling(xyz_b, npoint_sa, known=first) if split else first
        fps_done = torch.cuda.Event()
        fps_done.record(sb)
        return xyz_ready, first, src, first_ready, idx, fps_done

    def _sample_from_count(self, n, locs_rows, bufs):
        """Eval forward of ONE scene: from the foreground count straight to the first sampling launch -- the device has
        been idle since the count left it.  The draw, the upload of its indices and the gather of the drawn points are one
        native call (pointops.draw_sample), the two sampling launches follow; everything else the forward does with the
        count (views, offsets, the stage's streams) comes after.  Returns what _aggregate_geodesic_overlapped would have
        produced for the scene at this point, or None (generator not drivable in place: that method's own route)."""
        npoint = min(n, self.cfg.n_downsampling)
        drawn = pointops.draw_sample(n, npoint, locs_rows, bufs)
        if drawn is None:
            return None
        sampling_indices, xyz_b = drawn[:2]
        sb = torch.cuda.current_stream()
        if len(drawn) == 3:
            # the first sampling launch went out with the draw; what the side streams wait for before they touch the
            # points is then the end of that launch (the kNN graphs read the foreground rows, not the drawn ones: they
            # wait for `bufs["before"]`, recorded before the draw)
            first_ready = torch.cuda.Event()
            first_ready.record(sb)
            return (sampling_indices, xyz_b) + self._first_picks(xyz_b, sb, first=drawn[2], xyz_ready=first_ready)
        return (sampling_indices, xyz_b) + self._first_picks(xyz_b, sb)

    def _aggregate_geodesic_overlapped(self, locs_float_, output_feats_, batch_offsets_, batch_size, graphs, max_step,
                                       pc_dims=None, sample=True, epilogue=True, early=None, presampled=None,
                                       presampled_before=None):
        """Inference on the GPU.  Furthest point sampling (2047 serial rounds on 16 compute units) and the geodesic
        BFS (<= 256 serial hops, one workgroup per query) are the two long latency-bound launches of the forward, and
        the BFS only needs the first n_query_points picks.  So the sampling is cut after those picks, the BFS goes
        to a second HIP stream with four queries per compute unit (it then fits on the units the sampling leaves
        free: gf_geodesic_bfs_cfg), and the rest of the sampling, ball query, grouping, the shared MLP and the
        decoder's input projections run beside it on the main stream, which joins where the decoder first needs the
        distances (relative_position_embedding).  Same values as forward_aggregator + cal_geodesic, same consumption
        of the host RNG.  GF_OVERLAP=2 keeps the sampling in one piece and starts the BFS after it.
        sample=False: no random sub-sampling of the scene's points first (GeoFormerFS, geoformer_fs.py:300-318);
        epilogue=False: none of the small side-stream launches whose results GeoFormer.forward picks up later."""
        offs = _offsets_list(batch_offsets_)
        grad_ctx = self._grad_ctx("set_aggregator")  # like forward_aggregator: no graph through a frozen aggregator
        nq, npoint_sa, split = self._sampling_split()
        main = torch.cuda.current_stream()
        sides = _SIDE_STREAMS  # process-wide, one set per caller stream: scenes in flight on
        side = sides.get((locs_float_.device, main.cuda_stream))   # different streams do not queue behind each other
        if side is None:
            side = torch.cuda.Stream(device=locs_float_.device)  # (stream priorities made no difference: measured)
            sides[(locs_float_.device, main.cuda_stream)] = side
        # a third stream for small work that needs neither the BFS nor the rest of the sampling (the ball query's
        # point grid, the query positional embedding): behind the BFS on `side` it would gate the decoder
        aux = sides.get((locs_float_.device, main.cuda_stream, "aux"))
        if aux is None:
            aux = sides[(locs_float_.device, main.cuda_stream, "aux")] = torch.cuda.Stream(device=locs_float_.device)
        geo_ready = [None] * batch_size
        staged, geo = [None] * batch_size, [None] * batch_size
        fps_done_evs = []  # (forward_split: the end of every scene's sampling)
        # Several scenes with gradients (the training step): every scene's sampling goes to a stream of its own and its
        # BFS to another, so the scenes' two latency-bound launches run beside each other instead of one scene after
        # the other (4 x (0.4 + 3.3) ms of a batch-4 step in which the device finishes last); the main stream joins
        # them before the grouping.  One scene / inference: the streams of the docstring.
        multi = batch_size > 1 and early is None and not epilogue
        scene_streams = []
        def host_draw(b, n_b):
            """The reference's host draw of scene b (same values, same generator state), restated natively, into a pinned
            buffer of this host thread (the upload that follows is an asynchronous copy)."""
            npoint = min(n_b, self.cfg.n_downsampling)
            pins = getattr(_OFFS_CACHE, "draw_pins", None)
            if pins is None:
                pins = _OFFS_CACHE.draw_pins = {}
            pin = pins.get((main.cuda_stream, b))  # per caller stream: scenes in flight on two streams
            if pin is None or pin.numel() < npoint:
                pin = pins[(main.cuda_stream, b)] = torch.empty(max(npoint, 65536), dtype=torch.int64).pin_memory()
            drawn = pointops.legacy_choice(n_b, npoint, out=pin.numpy())
            if drawn.ctypes.data != pin.data_ptr():  # numpy's own route (exotic generator state): stage it
                pin.numpy()[:npoint] = drawn
            return pin, npoint

        order = list(range(batch_size))
        draws = {}
        if multi:
            # the draws consume the generator in scene order; the device work goes out largest scene first -- its BFS
            # is the stretch's long pole (5.8 of ~10 ms when it was issued third)
            for b in order:
                if offs[b + 1] - offs[b] == 0:
                    return None, None  # (after the draws of the scenes before it, like the scene-by-scene order)
                if sample:
                    draws[b] = host_draw(b, offs[b + 1] - offs[b])
            order.sort(key=lambda b: -(offs[b + 1] - offs[b]))
        for b in order:
            n_b = offs[b + 1] - offs[b]
            if n_b == 0:
                return None, None
            if multi:
                sb = sides.get((locs_float_.device, main.cuda_stream, "scene", b))
                if sb is None:
                    sb = sides[(locs_float_.device, main.cuda_stream, "scene", b)] = torch.cuda.Stream(device=locs_float_.device)
                side_b = sides.get((locs_float_.device, main.cuda_stream, "bfs", b))
                if side_b is None:
                    side_b = sides[(locs_float_.device, main.cuda_stream, "bfs", b)] = torch.cuda.Stream(device=locs_float_.device)
                sb.wait_stream(main)
                scene_streams.append(sb)
            else:
                sb, side_b = main, side
            with torch.cuda.stream(sb):
                if presampled is not None and b == 0 and not multi and sample:
                    # (the caller went from the count to these launches directly: _sample_from_count)
                    sampling_indices, xyz_b, xyz_ready, first, src, first_ready, idx, fps_done = presampled
                    self.last_sampling_indices = sampling_indices
                else:
                    if sample:
                        # (one scene: the device idles on this draw)
                        pin, npoint = draws[b] if b in draws else host_draw(b, n_b)
                        sampling_indices = pin[:npoint].to(locs_float_.device, non_blocking=True)
                        self.last_sampling_indices = sampling_indices
                        xyz_b = locs_float_[offs[b]:offs[b + 1]][sampling_indices].unsqueeze(0).contiguous()
                    else:
                        sampling_indices = None
                        xyz_b = locs_float_[offs[b]:offs[b + 1]].unsqueeze(0).contiguous()
                    xyz_ready, first, src, first_ready, idx, fps_done = self._first_picks(xyz_b, sb)
                fps_done_evs.append(fps_done)
                picks_ready = first_ready
            if early is not None and b == 0:
                # work of the caller that does not depend on the sampling, queued on the third stream now that the first
                # sampling launch is out: first the kNN graphs alone (early(True)) -- the BFS launch below is the next
                # thing the device will be waiting for (the query picks take ~0.27 ms; with everything else of this
                # stretch issued first the host reached the BFS launch 0.33-0.48 ms after the count) -- the rest
                # (early(False) -> (mask features, class probabilities)) behind that launch
                # (the graphs read the foreground rows: with the sampling launched from the count, `before` -- recorded
                #  behind the foreground selection -- is all they wait for; xyz_ready is then the end of the first launch)
                aux.wait_event(presampled_before if presampled_before is not None else xyz_ready)
                with torch.cuda.stream(aux):
                    graphs = early(True)
                    for t in _tensors_of(graphs):
                        t.record_stream(main)
                        t.record_stream(side)
                    graphs_done = torch.cuda.Event()
                    graphs_done.record(aux)
                side.wait_event(graphs_done)
            # (the BFS waits for the query picks only -- not for the rest of the sampling queued behind them)
            side_b.wait_event(first_ready)
            with torch.cuda.stream(side_b):
                D, I, deg = graphs[b][:3]
                g = pointops.geodesic_bfs(D, I, deg, src, 0.05, max_step,
                                          wg_threads=_bfs_wg(int(src.shape[0]), batch_size) if split else 1024)
                g.record_stream(main)
                src.record_stream(side_b)
                geo[b] = g
                ev = torch.cuda.Event()
                ev.record(side_b)
                geo_ready[b] = ev
            if early is not None and b == 0:
                with torch.cuda.stream(aux):
                    early_out = tuple(early(False)) + (graphs,)
                    for t in _tensors_of(early_out[:2]):
                        t.record_stream(main)
                        t.record_stream(side)
                    early_done = torch.cuda.Event()
                    early_done.record(aux)
            grid = None
            if xyz_b.shape[1] >= 4096 and not torch.is_grad_enabled():
                # the ball query's point grid needs the points only: built on the third stream under the first picks
                # (issued after their launch and after the BFS launch -- nothing may delay those)
                aux.wait_event(xyz_ready)
                with torch.cuda.stream(aux):
                    xyz_b.record_stream(aux)
                    grid = pointops.point_grid_build(xyz_b, self.set_aggregator.radius)
                    grid.record_stream(main)
                    grid_done = torch.cuda.Event()
                    grid_done.record(aux)
                grid = (grid, grid_done)
            if multi:
                for t in (xyz_b, idx, first, sampling_indices):
                    if t is not None:
                        t.record_stream(main)
            if early is not None and b == 0:
                main.wait_event(early_done)
            staged[b] = [xyz_b, None, idx, grid, sampling_indices]
            if not epilogue:
                continue
            # small launches that only need the distances / the query picks ride beside the sampling instead of
            # sitting between the decoder and the mask head on the main stream
            self._side_epilogue(b, batch_size, g, xyz_b, src, pc_dims, main, side, aux, picks_ready)
        for sb in scene_streams:
            main.wait_stream(sb)
        # (the sampled features are only read after the sampling: gathered here, off the path to its first launch)
        with grad_ctx():
            for b, st in enumerate(staged):
                feat_b = output_feats_[offs[b]:offs[b + 1]]
                if st[4] is not None:
                    feat_b = pointops.take_rows_unique(feat_b, st[4])  # (a draw without replacement)
                st[1] = feat_b.unsqueeze(0).transpose(1, 2).contiguous()
        staged = [tuple(st[:4]) for st in staged]
        self.__dict__.setdefault("_gf_pending_side", {})[_stream_key(locs_float_.device)] = geo_ready
        self.__dict__.setdefault("_gf_stretch_events", {})[_stream_key(locs_float_.device)] = fps_done_evs + [
            ev for ev in geo_ready if ev is not None]
        cat = lambda ts: ts[0] if len(ts) == 1 else torch.cat(ts)  # noqa: E731
        with grad_ctx():
            fused = []
            for xyz_b, feat_b, idx, grid in staged:
                if grid is not None:
                    main.wait_event(grid[1])
                fused.append(self.set_aggregator.fused_forward(xyz_b, feat_b, idx, grid=None if grid is None else grid[0]))
            if all(f is not None for f in fused):
                context_locs, pre_enc_inds = cat([f[0] for f in fused]), cat([st[2] for st in staged])
                context_feats = cat([f[1] for f in fused]).transpose(1, 2)
                res = ((context_locs, context_feats, pre_enc_inds), geo)
                return res + (early_out,) if early is not None else res
            locs, gfeat, gxyz, inds = [], [], [], []
            for xyz_b, feat_b, idx, _ in staged:
                l, gf, gx, idx = self.set_aggregator.group_points(xyz_b, feat_b, inds=idx)
                locs.append(l); gfeat.append(gf); gxyz.append(gx); inds.append(idx)
            context_locs, pre_enc_inds = cat(locs), cat(inds)
            context_feats = self.set_aggregator.mlp(cat(gfeat), cat(gxyz)).transpose(1, 2)
        res = ((context_locs, context_feats, pre_enc_inds), geo)
        return res + (early_out,) if early is not None else res

    def _side_epilogue(self, b, batch_size, g, xyz_b, src, pc_dims, main, side, aux, first_ready):
        early = self._early()
        if b == 0:
            early.clear()
        with torch.cuda.stream(side):
            # behind the BFS: sqrt of the per-query maximum geodesic distance (mask_heads_forward, geoformer.py:303-306)
            mx = torch.max(g, dim=1)[0]
            mx = torch.sqrt(torch.where(mx < 0, torch.max(mx), mx)).contiguous()
            mx.record_stream(main)
            ev = torch.cuda.Event()
            ev.record(side)
            early[("mx", b)] = (g, mx, ev)
        if batch_size == 1 and pc_dims is not None and self.cfg.dec_dim == 64:
            aux.wait_event(first_ready)
            with torch.cuda.stream(aux):
                # (the folded copy of the projection's parameters is derived on the stream that reads it)
                qpr = self._pointwise_chain("qproj", [self.query_projection], xyz_b)
                if qpr is not None:
                    xyz_b.record_stream(aux)
                    q_locs = xyz_b[:, src.long()]  # the first picks = the query points (same gather as group_points)
                    qpe = self.pos_embedding(q_locs, input_range=pc_dims).float()
                    qpos = pointops.pointwise_mlp(qpe[0].t().contiguous(), qpr)
                    qpos.record_stream(main)
                    src.record_stream(aux)
                    ev = torch.cuda.Event()
                    ev.record(aux)
                    early["qpos"] = (q_locs, qpos, ev)

    def _early(self):
        """Results computed beside the BFS for the forward running on the CALLER's stream (per-stream dict)."""
        if not torch.cuda.is_available():
            return {}
        return self.__dict__.setdefault("_gf_early", {}).setdefault(_stream_key(), {})

    def _join_side_stream(self):
        """The calling stream waits for the geodesic distances (not for the small launches queued behind them)."""
        pend = self.__dict__.get("_gf_pending_side")
        if pend and torch.cuda.is_available():
            for ev in pend.pop(_stream_key(), None) or ():
                torch.cuda.current_stream().wait_event(ev)

    # -- decoder ------------------------------------------------------------------------------
    def relative_position_embedding(self, context_locs, query_locs, pc_dims, geo_dists, pre_enc_inds):
        """[nq, nc, B, d] Fourier embedding of the query->context geodesic distances; unreachable
        pairs get max_geo(query) + |dxyz| per axis (geoformer.py:619-651)."""
        B = context_locs.shape[0]
        self._join_side_stream()  # the geodesic distances may still be in flight on the second stream
        if context_locs.is_cuda and self.cfg.dec_dim == 64 and (not torch.is_grad_enabled()
                                                                 or os.environ.get("GF_FUSED_BWD", "1") != "0"):
            # hand the fused cross-attention kernel the ingredients instead of the 134 MB tensor (training too: its
            # backward recomputes the embedding, csrc/decoder_attn.hip)
            if B == 1 and pre_enc_inds.dtype == torch.int32:
                g1, m1 = pointops.relpos_prepare(geo_dists[0].contiguous(), pre_enc_inds[0].contiguous())
                geo, max_geo = g1.unsqueeze(0), m1.unsqueeze(0)
            elif B > 1 and pre_enc_inds.stride(0) == 0 and all(g is geo_dists[0] for g in geo_dists):
                # B episodes over ONE cached scene (GeoFormerFS.requery_many): gathered once, shared by all of them
                g1 = geo_dists[0][:, pre_enc_inds[0].long()]
                m1 = torch.max(g1, dim=1)[0]
                m1 = torch.where(m1 < 0, torch.max(m1), m1)
                geo, max_geo = g1.unsqueeze(0).expand(B, -1, -1).contiguous(), m1.unsqueeze(0).expand(B, -1).contiguous()
            else:
                geo = torch.stack([geo_dists[b][:, pre_enc_inds[b].long()] for b in range(B)], dim=0).contiguous()
                max_geo = torch.max(geo, dim=2)[0]
                max_geo = torch.where(max_geo < 0, torch.max(max_geo), max_geo).contiguous()
            return RelPosSpec(geo, max_geo, query_locs.contiguous(), context_locs.contiguous(),
                              pc_dims[0].float().contiguous(), pc_dims[1].float().contiguous(),
                              self.pos_embedding.gauss_B.contiguous())
        rel = torch.abs(query_locs[:, :, None, :] - context_locs[:, None, :, :])
        nq, nc = rel.shape[1], rel.shape[2]
        geo = torch.stack([geo_dists[b][:, pre_enc_inds[b].long()] for b in range(B)], dim=0)  # B x nq x nc
        max_geo = torch.max(geo, dim=2)[0]
        max_all = torch.max(max_geo)
        max_geo = torch.where(max_geo < 0, max_all, max_geo)
        geo3 = geo[:, :, :, None].repeat(1, 1, 1, 3)
        geo3 = torch.where(geo3 < 0, max_geo[:, :, None, None] + rel, geo3)
        emb = self.pos_embedding(geo3.reshape(B, nq * nc, -1), input_range=pc_dims).reshape(B, -1, nq, nc)
        return emb.permute(2, 3, 0, 1)

    def forward_decoder(self, context_locs, context_feats, query_locs, pc_dims, geo_dists, pre_enc_inds):
        nq = self.cfg.n_query_points
        if context_locs.shape[0] == 1 and context_locs.is_cuda and not torch.is_grad_enabled():
            # inference, one scene: the two projection stacks as fused launches over token rows; the context's
            # positional embedding is skipped (the pre-norm relative layer never reads `pos`, transformer_detr.py:425-463)
            e2d = self._pointwise_chain("e2d", [self.encoder_to_decoder_projection], context_feats)
            qpr = self._pointwise_chain("qproj", [self.query_projection], context_feats)
            if e2d is not None and qpr is not None:
                ctx = pointops.pointwise_mlp(context_feats[0].contiguous(), e2d)  # [nc, dec_dim]
                # (built by the decoder after its first token stage is queued: the join with the BFS stream sits there)
                rel = LazyRelPos(lambda: self.relative_position_embedding(context_locs, query_locs, pc_dims, geo_dists,
                                                                          pre_enc_inds))
                hit = self._early().pop("qpos", None)  # computed beside the BFS on the third stream (own event)
                if hit is not None and hit[0].shape == query_locs.shape:
                    torch.cuda.current_stream().wait_event(hit[2])
                    qpos = hit[1]
                else:
                    qpe = self.pos_embedding(query_locs, input_range=pc_dims).float()  # [1, dec_dim, nq]
                    qpos = pointops.pointwise_mlp(qpe[0].t().contiguous(), qpr)  # [nq, dec_dim]
                memory = ctx.unsqueeze(1)  # [nc, 1, dec_dim]
                return self.decoder(tgt=memory[:nq], memory=memory, pos=None, query_pos=qpos.unsqueeze(1),
                                    relative_pos=rel)
        context_embedding_pos = self.pos_embedding(context_locs, input_range=pc_dims)
        context_feats = self.encoder_to_decoder_projection(context_feats.permute(0, 2, 1))  # B x C x nc
        query_embedding_pos = self.query_projection(self.pos_embedding(query_locs, input_range=pc_dims).float())
        dec_inputs = context_feats[:, :, :nq].permute(2, 0, 1)
        relative_embedding_pos = self.relative_position_embedding(context_locs, query_locs, pc_dims, geo_dists,
                                                                  pre_enc_inds)
        return self.decoder(tgt=dec_inputs, memory=context_feats.permute(2, 0, 1),
                            pos=context_embedding_pos.permute(2, 0, 1), query_pos=query_embedding_pos.permute(2, 0, 1),
                            relative_pos=relative_embedding_pos)

    # -- dynamic-convolution mask head ------------------------------------------------------------
    def parse_dynamic_params(self, params, out_channels):
        n = params.size(0)
        w1, w2, b1, b2 = torch.split_with_sizes(params, self.weight_nums + self.bias_nums, dim=1)
        return ([w1.reshape(n * out_channels, -1, 1), w2.reshape(n, -1, 1)],
                [b1.reshape(n * out_channels), b2.reshape(n)])

    def mask_heads_forward(self, geo_dist, mask_features, weights, biases, num_insts, coords_, fps_sampling_coords,
                           use_geo=True):
        """logits[q, p] = W2_q relu(W1_q [rel_xyz(q,p); f_p] + b1_q) + b2_q with rel = q_xyz - p_xyz and,
        where p is geodesically unreachable from q, rel += sqrt(max_geo_q) * sign(rel) (geoformer.py:286-324)."""
        n_mask = mask_features.size(0)
        if (mask_features.is_cuda and self.output_dim == 16 and not torch.is_grad_enabled()):
            # inference: one fused HIP kernel (no nq x 19 x N intermediate)
            mx = None
            if use_geo:
                early = self._early()
                hit = next((early.pop(k) for k in list(early) if k[0] == "mx" and early[k][0] is geo_dist), None)
                if hit is not None:
                    torch.cuda.current_stream().wait_event(hit[2])
                    mx = hit[1]  # computed beside the BFS
                else:
                    mx = torch.max(geo_dist, dim=1)[0]
                    mx = torch.sqrt(torch.where(mx < 0, torch.max(mx), mx)).contiguous()
            od = self.output_dim
            logits = pointops.mask_head(
                mask_features.reshape(n_mask, od).contiguous(), coords_.contiguous(),
                geo_dist.contiguous() if use_geo else None, fps_sampling_coords.reshape(-1, 3).contiguous(), mx,
                weights[0].reshape(num_insts, od, od + 3).contiguous(), biases[0].reshape(num_insts, od).contiguous(),
                weights[1].reshape(num_insts, od).contiguous(), biases[1].reshape(num_insts).contiguous())
            return logits.reshape(1, num_insts, n_mask)
        rel = fps_sampling_coords.reshape(-1, 1, 3) - coords_.reshape(1, -1, 3)  # nq x N x 3
        if use_geo:
            mx = torch.max(geo_dist, dim=1)[0]
            mx = torch.sqrt(torch.where(mx < 0, torch.max(mx), mx))
            rel = torch.where((geo_dist < 0).unsqueeze(-1), rel + mx[:, None, None] * torch.sign(rel), rel)
        w1, w2 = weights[0].reshape(num_insts, self.output_dim, -1), weights[1].reshape(num_insts, 1, -1)
        b1, b2 = biases[0].reshape(num_insts, self.output_dim, 1), biases[1].reshape(num_insts, 1, 1)
        feat = mask_features.reshape(n_mask, -1)  # N x C
        # first layer split into its coordinate part (per query) and its feature part (shared input)
        h = torch.matmul(w1[:, :, :3], rel.permute(0, 2, 1)) + torch.matmul(w1[:, :, 3:], feat.t().unsqueeze(0)) + b1
        x = torch.matmul(w2, F.relu(h)) + b2  # nq x 1 x N
        return x.reshape(1, num_insts, n_mask)

    def _mask_head_packed(self, geo_dist, mask_features, params, num_insts, coords_, fps_sampling_coords):
        """mask_heads_forward (geoformer.py:286-324) with the generated parameters read from `params` in place."""
        n_mask = mask_features.size(0)
        early = self._early()
        hit = next((early.pop(k) for k in list(early) if k[0] == "mx" and early[k][0] is geo_dist), None)
        if hit is not None:
            torch.cuda.current_stream().wait_event(hit[2])
            mx = hit[1]  # computed beside the BFS
        else:
            mx = torch.max(geo_dist, dim=1)[0]
            mx = torch.sqrt(torch.where(mx < 0, torch.max(mx), mx)).contiguous()
        logits = pointops.mask_head_packed(mask_features.reshape(n_mask, self.output_dim).contiguous(),
                                           coords_.contiguous(), geo_dist.contiguous(),
                                           fps_sampling_coords.reshape(-1, 3).contiguous(), mx, params.contiguous())
        return logits.reshape(1, num_insts, n_mask)

    def get_mask_prediction(self, geo_dists, param_kernels, mask_features, locs_float_, fps_sampling_locs,
                            batch_offsets_):
        num_layers, n_queries, batch = param_kernels.shape[:3]
        offs = _offsets_list(batch_offsets_)
        outputs = []
        # what the fused training route reads of a scene does not depend on the decoder layer: sliced / reduced once per
        # scene instead of once per (layer, scene) -- 80 small launches and 12 slice-gradient passes over the batch's
        # mask features less per batch-4 step
        fused_train = (mask_features.is_cuda and torch.is_grad_enabled() and self.output_dim == 16 and self.use_coords
                       and os.environ.get("GF_FUSED_BWD", "1") != "0")
        per_scene, train_ctrl = {}, {}
        if fused_train:
            for b in range(batch):
                s, e = offs[b], offs[b + 1]
                if e - s == 0:
                    continue
                g = geo_dists[b].contiguous()
                mx = torch.max(g, dim=1)[0]
                mx = torch.sqrt(torch.where(mx < 0, torch.max(mx), mx)).contiguous()
                per_scene[b] = (mask_features[s:e].reshape(e - s, self.output_dim).contiguous(),
                                locs_float_[s:e].contiguous(), g, fps_sampling_locs[b].reshape(-1, 3).contiguous(), mx)
        for l, pk in enumerate(param_kernels.unbind(0) if fused_train else param_kernels):  # pk: nq x B x C
            pk2 = pk.transpose(0, 1).flatten(0, 1)  # [B*nq, C] token rows
            sem_chain = self._pointwise_chain("detr_sem_head", [self.detr_sem_head], pk2)
            tow_chain = self._pointwise_chain("before_embedding_tower", [self.before_embedding_tower], pk2)
            packed = False
            if sem_chain is not None and tow_chain is not None:
                # inference on the GPU: the two token MLPs as fused launches, the controller as one GEMM.  (Running
                # the class head on the second stream beside the mask head was measured with tools/ab_inprocess.py:
                # no difference -- back-to-back small kernels cost ~1.5 us each, not the ~5 us a profiler shows.)
                rows = pk2.contiguous()
                packed = self.output_dim == 16 and self.use_coords
                cls_done = None
                if packed and rows.is_cuda and not torch.is_grad_enabled() and batch == 1 and not pointops.co_resident():
                    # the class head (a 25 us launch: three dependent 64-wide layers over 256 rows on four workgroups) is
                    # not what the mask head waits for: on the third stream, beside the tower / controller / mask head
                    # (tools/ab_inprocess.py, alternating forwards in one process: 4.37 -> 4.32 and 4.38 -> 4.34 ms; NOT in a
                    #  serving loop's last part, which runs beside the next scene's stretch on the other lane: there the
                    #  extra stream cost the staggered loop 5 % -- 231 -> 220 scenes/s, bisected on one box)
                    main = torch.cuda.current_stream(rows.device)
                    aux = _SIDE_STREAMS.get((rows.device, main.cuda_stream, "aux"))
                    if aux is not None:
                        rows_ready = torch.cuda.Event()
                        rows_ready.record(main)
                        aux.wait_event(rows_ready)
                        with torch.cuda.stream(aux):
                            cls_logits = pointops.pointwise_mlp(rows, sem_chain).reshape(batch, n_queries, -1)
                            cls_done = torch.cuda.Event()
                            cls_done.record(aux)
                        rows.record_stream(aux)
                        cls_logits.record_stream(main)
                if cls_done is None:
                    cls_logits = pointops.pointwise_mlp(rows, sem_chain).reshape(batch, n_queries, -1)
                emb = pointops.pointwise_mlp(rows, tow_chain)
                controllers = F.linear(emb, self.controller.weight[:, :, 0], self.controller.bias)
            else:
                cls_logits = self.detr_sem_head(pk.permute(1, 2, 0)).transpose(1, 2)  # B x nq x classes
                controllers = self.controller(self.before_embedding_tower(pk2.unsqueeze(2))).squeeze(2)
            controllers = controllers.reshape(batch, n_queries, -1)
            ctrl = controllers.unbind(0) if fused_train else controllers
            mask_logits_list = []
            for b in range(batch):
                s, e = offs[b], offs[b + 1]
                if e - s == 0:
                    mask_logits_list.append(None)
                    continue
                if packed and mask_features.is_cuda and not torch.is_grad_enabled():
                    # the controller's output read in place by the kernel (no split / reshape / contiguous copies)
                    ml = self._mask_head_packed(geo_dists[b], mask_features[s:e], controllers[b], n_queries,
                                                locs_float_[s:e], fps_sampling_locs[b])
                elif fused_train:
                    # training: the mask head runs after this loop, once per scene for ALL layers (episodes of
                    # gf_mask_head_episodes / gf_mask_head_bwd_episodes): one forward launch and one backward triple per
                    # scene instead of one per (layer, scene), the features' gradient summed inside the kernel
                    train_ctrl.setdefault(b, []).append(ctrl[b])
                    mask_logits_list.append(None)
                    continue
                else:
                    weights, biases = self.parse_dynamic_params(controllers[b], self.output_dim)
                    ml = self.mask_heads_forward(geo_dists[b], mask_features[s:e], weights, biases, n_queries,
                                                 locs_float_[s:e], fps_sampling_locs[b], use_geo=self.use_coords)
                mask_logits_list.append(ml.squeeze(0))
            if packed and cls_done is not None:
                torch.cuda.current_stream(cls_logits.device).wait_event(cls_done)  # (behind the mask head's launch)
            outputs.append({"cls_logits": cls_logits, "mask_logits": mask_logits_list})
        for b, ctrls in train_ctrl.items():
            mf_b, locs_b, g, fps_b, mx = per_scene[b]
            logits = pointops.mask_head_train_episodes(mf_b, torch.stack(ctrls), locs_b, g, fps_b, mx)  # [L, nq, N_b]
            for l, ml in enumerate(logits.unbind(0)):
                outputs[l]["mask_logits"][b] = ml
        return outputs

    def generate_proposal(self, mask_logits, cls_logits, fg_idxs, batch_offsets, batch_offsets_,
                          semantic_scores_=None, logit_thresh=0.5, score_thresh=0.5, npoint_thresh=100, sem_prob=None,
                          defer=False, knn_flags=(), segments=None):
        """Batch-1 proposal extraction (geoformer.py:193-262): score = mean mask prob * sqrt(cls prob) *
        mean semantic prob of the predicted class over the mask.  defer: return a PendingProposals instead of
        waiting for the device (GPU inference only).  segments (int32 [N], one over-segment id per point of the batch,
        negative = none; honoured without grad only): the mask logits are pooled over the segments' foreground points
        (csrc/segment_pool.hip; postprocess.segment_pool_host on the CPU) and the pooled ones take the raw ones' place
        in everything below; mask_logits itself is left as it is."""
        b = 0
        segments = None if torch.is_grad_enabled() else _segments_arg(segments)
        if mask_logits[b].is_cuda and not torch.is_grad_enabled():
            # inference: two fused HIP launches (csrc/proposal.hip) instead of ~40 PyTorch ones; the acceptance flags
            # come back in one small copy and the row selection is made on the host (nonzero() on the device is six
            # launches around its own read-back)
            offs, offs_ = _offsets_list(batch_offsets), _offsets_list(batch_offsets_)
            num_points = int(offs[b + 1] - offs[b])
            logits = mask_logits[b].contiguous()
            if sem_prob is not None and isinstance(sem_prob, tuple):
                sem_t = sem_prob[1][:, offs_[b]:offs_[b + 1]]  # class-major copy made early, off the critical path
            else:
                sem = sem_prob if sem_prob is not None else F.softmax(semantic_scores_, dim=1)
                sem_t = sem[offs_[b]:offs_[b + 1]].t()
            # Deferred proposals (a loop that collects scene i's after it has issued scene i+1): statistics, selection, the
            # count's copy and later the membership scatter -- ~0.1 ms of small launches that nothing on the caller's stream
            # waits for -- go to the third stream behind the mask head, so that the NEXT scene's backbone does not queue
            # behind them.  (Not in a serving loop's last part: its lanes are balanced as they are.)
            side = None
            if defer and not pointops.co_resident():
                main = torch.cuda.current_stream(logits.device)
                side = _SIDE_STREAMS.get((logits.device, main.cuda_stream, "aux"))
            cls_b, sem_c, fg_c = cls_logits[b].contiguous(), sem_t.contiguous(), fg_idxs.contiguous()

            def pooled(raw):  # (queued on the stream of the statistics)
                n_b = raw.shape[1]
                seg_fg = segments[fg_c[offs_[b]:offs_[b] + n_b]]
                return pointops.segment_pool_batched([raw], seg_fg, [0, n_b])[0]

            if side is not None:
                ready = torch.cuda.Event()
                ready.record(main)
                side.wait_event(ready)
                raw = logits
                with torch.cuda.stream(side):
                    if segments is not None:
                        logits = pooled(raw)
                    cls_pred, _, scores, final = pointops.proposal_stats(logits, cls_b, sem_c, logit_thresh, score_thresh,
                                                                         npoint_thresh, min_class=4, class_major=True)
                    pending = PendingProposals(final, cls_pred, scores, logits, fg_c, logit_thresh, num_points,
                                               knn_flags=knn_flags)
                pending.home = main
                for t in (raw, cls_b, sem_c, fg_c) + tuple(knn_flags) + (() if segments is None else (segments,)):
                    t.record_stream(side)
                return pending
            if segments is not None:
                logits = pooled(logits)
            cls_pred, _, scores, final = pointops.proposal_stats(logits, cls_b, sem_c, logit_thresh, score_thresh,
                                                                 npoint_thresh, min_class=4, class_major=True)
            pending = PendingProposals(final, cls_pred, scores, logits, fg_c, logit_thresh, num_points, knn_flags=knn_flags)
            return pending if defer else pending.get()
        sem = sem_prob if sem_prob is not None and not isinstance(sem_prob, tuple) else F.softmax(semantic_scores_, dim=1)
        num_points = int(batch_offsets[b + 1] - batch_offsets[b])
        logits = mask_logits[b]
        if segments is not None:
            from .. import postprocess

            lo = int(batch_offsets_[b])
            seg_fg = segments[fg_idxs[lo:lo + logits.shape[1]]]
            logits = torch.from_numpy(postprocess.segment_pool_host(logits, seg_fg)).to(logits.device)
        mask_prob = logits.sigmoid()
        cls_prob = F.softmax(cls_logits[b], dim=-1)
        cls_pred = torch.argmax(cls_logits[b], dim=-1)
        sem_b = sem[int(batch_offsets_[b]):int(batch_offsets_[b + 1])]
        mask_bool = mask_prob >= logit_thresh
        npts = torch.sum(mask_bool, dim=1)
        mask_scores = torch.sum(mask_prob * mask_bool.int(), dim=1) / (npts + 1e-6)
        cls_scores = torch.gather(cls_prob, 1, cls_pred.unsqueeze(-1)).squeeze(-1)
        sem_scores = torch.matmul(mask_bool.float(), sem_b) / (npts[:, None] + 1e-6)  # nq x classes
        sem_scores = torch.gather(sem_scores, 1, cls_pred.unsqueeze(-1)).squeeze(-1)
        scores = mask_scores * torch.pow(cls_scores, 0.5) * sem_scores
        final = (cls_pred >= 4) & (npts >= npoint_thresh) & (mask_scores >= score_thresh)
        if torch.count_nonzero(final) == 0:
            return [], [], []
        masks_final = mask_bool[final]
        proposals = torch.zeros((masks_final.shape[0], num_points), dtype=torch.int, device=mask_prob.device)
        inst, pts = torch.nonzero(masks_final, as_tuple=True)
        proposals[inst, fg_idxs[pts]] = 1
        return cls_pred[final], scores[final], proposals

    def generate_proposals_batched(self, mask_logits, cls_logits, fg_idxs, batch_offsets, fg_offsets, scene_ids,
                                   n_scenes, sem_prob, logit_thresh=0.5, score_thresh=0.5, npoint_thresh=100,
                                   defer=False, knn_flags=(), segments=None):
        """generate_proposal for every scene of the batch (geoformer.py:193-262 with b = 0..B-1) in a fixed number of
        launches (csrc/batch_post.hip): statistics over all (scene, query) pairs, per-scene selection, one read-back of
        all counts, one packed membership scatter.  mask_logits: per kept scene [nq, N_b]; cls_logits [S, nq, ncls];
        fg_offsets: host offsets of the kept scenes' foreground rows; scene_ids: the batch index of each kept scene;
        sem_prob: (probabilities, class-major copy).  segments: as generate_proposal's, pooled for all kept scenes in
        one gf_segment_pool_batched call on this stream.  Returns the list of n_scenes tuples, or with defer a
        PendingBatchProposals."""
        from .. import postprocess

        offs = _offsets_list(batch_offsets)
        logits = [ml.contiguous() for ml in mask_logits]
        segments = _segments_arg(segments)
        if segments is not None:
            logits = pointops.segment_pool_batched(logits, segments[fg_idxs], fg_offsets)
        nq = logits[0].shape[0]
        starts = [offs[b] for b in scene_ids]
        npts = [offs[b + 1] - offs[b] for b in scene_ids]
        sem_t = sem_prob[1] if isinstance(sem_prob, tuple) else sem_prob.t().contiguous()
        table = postprocess.proposal_scene_table([t.data_ptr() for t in logits], fg_offsets, starts, npts)
        table_d = pointops._table_dev(table, fg_idxs.device)
        cls_pred, _, scores, final = pointops.proposal_stats_batched(table_d, nq, cls_logits.contiguous(), sem_t,
                                                                     logit_thresh, score_thresh, npoint_thresh,
                                                                     min_class=4)
        sel, cls, sc, counts = pointops.proposal_select_batched(final, cls_pred, scores)
        pending = PendingBatchProposals(n_scenes, scene_ids, table_d, sel, cls, sc, counts, fg_idxs.contiguous(),
                                        logit_thresh, npts,
                                        int(postprocess.scene_rows(table, postprocess.PROP_ROW)["N"].max()), knn_flags)
        pending.keep = logits  # (the scatter reads the logit rows through the table)
        return pending if defer else pending.get()

    # -- forward --------------------------------------------------------------------------------
    def forward(self, batch_input, epoch, training=True, defer_proposals=False, all_scenes=False):
        """defer_proposals (GPU inference): everything is queued on the current stream and
        ``outputs["proposal_scores"]`` is a PendingProposals whose ``get()`` makes the forward's last read-back -- a
        serving loop can queue the next scene on another stream before it collects this one.  The in-flight side-stream
        state is kept per caller stream, so forwards issued on their own streams (from one host thread or several) do
        not interfere; ``last_sampling_indices`` (a test hook) is the one attribute that is per model.

        all_scenes (GPU inference): the proposals of EVERY scene of the batch, not only scene 0's (the reference's
        "only batch 1 when test"): ``outputs["proposal_scores_per_scene"]`` is a list of B tuples (cls_final,
        scores_final, masks_final) -- each what a forward of that scene alone returns, masks int32 [n_b, N_b] over the
        scene's own points, ([], [], []) for a scene without proposals or without foreground -- in place of
        ``proposal_scores``; with defer_proposals a PendingBatchProposals.  Scenes without foreground are dropped from
        the batch after the foreground selection, so they do not stop the others."""
        if all_scenes and (training or not batch_input["locs_float"].is_cuda):
            raise ValueError("forward(all_scenes=True) is the batched eval forward on the GPU (training=False)")
        steps = self._forward_steps(batch_input, epoch, training, defer_proposals, False, all_scenes)
        try:
            while True:
                next(steps)
        except StopIteration as done:
            return done.value

    def forward_split(self, batch_input, epoch, training=True, defer_proposals=False):
        """The forward in three parts for a serving loop (bench.py; class SplitForward): this scene's decoder and mask
        head (matrix work) are queued behind the NEXT scene's backbone and run under that scene's sampling / BFS stretch
        -- a few latency-bound workgroups that otherwise leave the chip idle for 40 % of a forward -- while the next
        scene's backbone is held back until this scene's stretch has ended (conv kernels beside it slow every one of
        its 2047 sampling rounds).  Every call of the handle must see the stream of the first one as the current
        stream.  Same launches as ``forward`` except the cross-attention's workgroup shape (8 waves, so that it fits
        beside a BFS workgroup); values agree to rounding."""
        return SplitForward(self._forward_steps(batch_input, epoch, training, defer_proposals, True))

    def _forward_steps(self, batch_input, epoch, training, defer_proposals, split, all_scenes=False):
        """The forward as a generator: with ``split`` it yields an event behind the backbone + semantic head and the
        events behind the sampling / BFS stretch; returns the outputs."""
        cfg = self.cfg
        outputs = {}
        batch_idxs = batch_input["locs"][:, 0].int()
        locs_float = batch_input["locs_float"]
        batch_offsets = batch_input["offsets"]
        batch_size = len(batch_offsets) - 1
        assert batch_size > 0
        pc_dims = [batch_input["pc_maxs"], batch_input["pc_mins"]]  # swapped on purpose (geoformer.py:412-415)
        # over-segment ids of the points (optional): the eval forward pools the mask logits over them before the proposals
        segments = _segments_arg(batch_input.get("segments"), locs_float.shape[0])
        if training or torch.is_grad_enabled():
            segments = None

        # inference on the GPU: arg-max, foreground test, index list and the four gathers in three launches before
        # the one read-back (csrc/foreground.hip) instead of max / compare / nonzero() / four gathers around it
        fused_fg = (locs_float.is_cuda and not torch.is_grad_enabled() and epoch > self.prepare_epochs
                    and locs_float.dtype == torch.float32)
        output_feats, semantic_scores, semantic_preds = self.forward_backbone(batch_input, batch_size,
                                                                              want_preds=not fused_fg)
        outputs["semantic_scores"] = semantic_scores
        if epoch <= self.prepare_epochs:
            return outputs
        same_fold = cfg.train_fold == cfg.cvfold
        fg_pending = None
        if fused_fg:
            # (the selection's launches and the copy of its count belong to the backbone's part: the device runs them
            # without waiting for the host to come back)
            feats_src, feat_rows = output_feats if isinstance(output_feats, tuple) else (output_feats.contiguous(), None)
            fg_pending = pointops.select_foreground(
                semantic_scores.contiguous(), 4 if same_fold else 3, not same_fold, locs_float.contiguous(),
                batch_idxs.contiguous(), feats_src, feat_rows, deferred=True)
        if split:
            # backbone, semantic head and foreground selection are queued (the read-back of the foreground count comes
            # next): the event marks the end of this scene's throughput-bound work for the loop
            backbone_done = torch.cuda.Event() if locs_float.is_cuda else None
            if backbone_done is not None:
                backbone_done.record()
            yield backbone_done
        if fused_fg:
            presampled = None
            # inference on one scene: the sampling is launched from the count alone (below), before the views / offsets
            from_count = (batch_size == 1 and not training and cfg.n_downsampling
                          and os.environ.get("GF_OVERLAP", "1") != "0")
            if batch_size == 1 and locs_float.is_cuda and cfg.n_downsampling and epoch > self.prepare_epochs:
                # the host has nothing to do until the foreground count is back: the generator words the sampling draw
                # will consume (they do not depend on the count) are drawn ahead now (csrc/host_draw.hip), and the
                # buffers of the draw are allocated
                pointops.legacy_prefetch(int(1.4 * locs_float.shape[0]) + 4096)
                if from_count:
                    nq_, npoint_sa_, split_ = self._sampling_split()
                    draw_bufs = pointops.draw_sample_buffers(int(cfg.n_downsampling), int(locs_float.shape[0]),
                                                             locs_float.device, fps_m=nq_ if split_ else npoint_sa_)
                    draw_bufs["before"] = fg_pending.done  # (recorded behind the foreground selection and the count's copy)
            n_fg = fg_pending.wait()
            if from_count and n_fg > 0:
                presampled = self._sample_from_count(n_fg, fg_pending.bufs[1], draw_bufs)
            fg_idxs, locs_float_, batch_idxs_, output_feats_, semantic_scores_ = fg_pending.views()
        else:
            fg = semantic_preds >= 4 if same_fold else semantic_preds == 3
            fg_idxs = torch.nonzero(fg).view(-1)
        # data-parallel training with SyncBatchNorm layers in the heads: the ranks leave here TOGETHER (parallel.py)
        agree = self.rank_agreement if (training and torch.is_grad_enabled()) else None
        if len(fg_idxs) == 0:
            if agree is not None:
                agree(False, locs_float.device)
            outputs["mask_predictions"] = None
            if all_scenes:
                empty = [([], [], []) for _ in range(batch_size)]
                outputs["proposal_scores_per_scene"] = PendingBatchProposals(batch_size, value=empty) \
                    if defer_proposals else empty
            return outputs
        if not fused_fg:
            batch_idxs_ = batch_idxs[fg_idxs]
            locs_float_ = locs_float[fg_idxs]
            output_feats_ = pointops.take_rows_unique(output_feats, fg_idxs)
            semantic_scores_ = semantic_scores[fg_idxs]
        batch_offsets_ = get_batch_offsets(batch_idxs_, batch_size, host_only=fused_fg and not training)
        offs_ = _offsets_list(batch_offsets_)  # the only read-back of this stretch, before the heavy launches
        nonempty = min(offs_[b + 1] - offs_[b] for b in range(batch_size)) > 0
        n_scenes, scene_ids = batch_size, list(range(batch_size))
        if all_scenes and not nonempty:
            # scenes without foreground leave the batch here (a forward of such a scene alone ends at this point too:
            # no sampling draw, no proposals); the others go on as a batch of their own
            scene_ids = [b for b in range(batch_size) if offs_[b + 1] > offs_[b]]
            offs_ = [offs_[b] for b in scene_ids] + [offs_[-1]]
            batch_offsets_ = torch.tensor(offs_, dtype=torch.int32, device=batch_offsets_.device)
            pc_dims = [pc_dims[0][scene_ids], pc_dims[1][scene_ids]]
            batch_size, nonempty = len(scene_ids), True
        if agree is not None and not agree(nonempty, locs_float.device):
            outputs["mask_predictions"] = None
            return outputs

        def sampling_independent(graphs_only=None):
            """Everything of this stretch that does not need the sampling: mask features, class probabilities (read
            by the proposal scores at the very end), the kNN graphs.  graphs_only True / False: the graphs alone / the other
            two alone (the inference path issues the BFS launch in between)."""
            if graphs_only is True:
                return knn_graphs(locs_float_, batch_offsets_, batch_size, neighbor=64, radius=0.05)
            chain = self._pointwise_chain("mask_tower", [self.mask_tower], output_feats_)
            if chain is not None:
                mf = pointops.pointwise_mlp(output_feats_.contiguous(), chain).unsqueeze(2)
            else:
                mf = self._mask_tower_rows(output_feats_)
                if mf is None:
                    mf = self.mask_tower(output_feats_.unsqueeze(2).permute(2, 1, 0)).permute(2, 1, 0)
            sp = None
            if not training:
                sp = F.softmax(semantic_scores_, dim=1)
                if sp.is_cuda:
                    sp = (sp, sp.t().contiguous())  # + the class-major copy the proposal kernel reads
            if graphs_only is False:
                return mf, sp
            gr = None
            if locs_float_.is_cuda and nonempty:
                gr = knn_graphs(locs_float_, batch_offsets_, batch_size, neighbor=64, radius=0.05)
            return mf, sp, gr

        max_step = 128 if self.training else 256
        geo_dists = None
        overlap = locs_float_.is_cuda and nonempty and os.environ.get("GF_OVERLAP", "1") != "0"
        if overlap and fused_fg and not training:
            # inference: the host goes straight to the sampling draw and the first sampling launch; the work above is
            # issued behind that launch on the third stream and runs beside it (the sampler keeps 16 CUs busy)
            contexts, geo_dists, (mask_features_, sem_prob, graphs) = self._aggregate_geodesic_overlapped(
                locs_float_, output_feats_, batch_offsets_, batch_size, None, max_step, pc_dims, epilogue=True,
                early=sampling_independent, presampled=presampled if fused_fg else None,
                presampled_before=draw_bufs["before"] if (fused_fg and presampled is not None) else None)
        else:
            mask_features_, sem_prob, graphs = sampling_independent()
            if graphs is not None and overlap:
                # (training too: sampling and BFS carry no gradient; grouping and the shared MLP stay PyTorch autograd)
                contexts, geo_dists = self._aggregate_geodesic_overlapped(locs_float_, output_feats_, batch_offsets_,
                                                                          batch_size, graphs, max_step, pc_dims,
                                                                          epilogue=not torch.is_grad_enabled())
            else:
                contexts = self.forward_aggregator(locs_float_, output_feats_, batch_offsets_, batch_size)
        if contexts is None:
            outputs["mask_predictions"] = None
            return outputs
        context_locs, context_feats, pre_enc_inds = contexts
        query_locs = context_locs[:, :cfg.n_query_points, :]

        if geo_dists is None:
            geo_dists = cal_geodesic(pre_enc_inds, locs_float_, batch_offsets_, max_step=max_step, neighbor=64,
                                     radius=0.05, n_queries=cfg.n_query_points, graphs=graphs)
        if split:
            # everything below waits for the geodesic distances anyway; the event marks the end of this scene's
            # sampling / BFS stretch for the loop that holds the next scene's backbone back until then
            stretch = []
            if locs_float.is_cuda:
                # the end of the sampling and of every scene's BFS -- not of the set abstraction queued behind them on
                # this stream (~0.2 ms that the next scene's backbone need not wait for)
                stretch = list(self.__dict__.get("_gf_stretch_events", {}).pop(_stream_key(locs_float.device), ()))
                if not stretch:
                    ev = torch.cuda.Event()
                    ev.record()
                    stretch = [ev]
            yield stretch
        dec_outputs = self.forward_decoder(context_locs, context_feats, query_locs, pc_dims, geo_dists, pre_enc_inds)
        self._join_side_stream()  # no-op unless a subclass' decoder skipped relative_position_embedding

        if training:
            idxs_sub, idxs_sub_raw = random_downsample(batch_offsets_, batch_size, n_subsample=30000,
                                                         host_offsets=_offsets_list(batch_offsets_))
            geo_sub = [geo_dists[b][:, idxs_sub_raw[b]] for b in range(batch_size)]
            del geo_dists
            batch_idxs_sub = batch_idxs_[idxs_sub]
            # the reference calls an undefined self.get_batch_offsets here (geoformer.py:482); intended
            # semantics = utils.get_batch_offsets
            offsets_sub = get_batch_offsets(batch_idxs_sub, batch_size)
            outputs["fg_idxs"] = fg_idxs[idxs_sub]
            outputs["num_insts"] = cfg.n_query_points * batch_size
            outputs["batch_idxs"] = batch_idxs_sub
            outputs["n_fg_total"] = int(offs_[-1])  # (host integer: the forward read the scenes' offsets back already)
            trunc = knn_truncated(graphs)
            if trunc is not None:  # read by the criterion together with its own end-of-step values
                outputs["knn_truncated"] = trunc
            outputs["mask_predictions"] = self.get_mask_prediction(geo_sub, dec_outputs,
                                                                   pointops.take_rows_unique(mask_features_, idxs_sub),
                                                                   locs_float_[idxs_sub], query_locs, offsets_sub)
        else:
            dec_outputs = dec_outputs[-1:, ...]
            outputs["fg_idxs"] = fg_idxs
            outputs["num_insts"] = cfg.n_query_points * batch_size
            outputs["batch_idxs"] = batch_idxs_
            preds = self.get_mask_prediction(geo_dists, dec_outputs, mask_features_, locs_float_, query_locs,
                                             batch_offsets_)
            outputs["mask_predictions"] = preds
            if all_scenes:
                outputs["proposal_scores_per_scene"] = self.generate_proposals_batched(
                    preds[-1]["mask_logits"], preds[-1]["cls_logits"], fg_idxs, batch_offsets, offs_, scene_ids,
                    n_scenes, sem_prob, logit_thresh=0.5, score_thresh=cfg.TEST_SCORE_THRESH,
                    npoint_thresh=cfg.TEST_NPOINT_THRESH, defer=defer_proposals,
                    knn_flags=[f for f in (knn_truncated(graphs),) if f is not None], segments=segments)
            else:
                outputs["proposal_scores"] = self.generate_proposal(
                    preds[-1]["mask_logits"], preds[-1]["cls_logits"], fg_idxs, batch_offsets, batch_offsets_,
                    semantic_scores_=semantic_scores_, logit_thresh=0.5, score_thresh=cfg.TEST_SCORE_THRESH,
                    npoint_thresh=cfg.TEST_NPOINT_THRESH, sem_prob=sem_prob, defer=defer_proposals,
                    knn_flags=[f for f in (knn_truncated(graphs),) if f is not None], segments=segments)
        if locs_float.is_cuda:
            self._early().clear()
        return outputs
