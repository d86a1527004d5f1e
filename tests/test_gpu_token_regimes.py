"""Every launch regime of the token-side kernels against float64: the inference decoder stage's self-attention
(k_decoder_stage_b: two_pass<8>, two_pass<16>, the online loop), the cross-attention forward (bf16-split 16-wave, fp32
16-wave, fp32 8-wave) and its backward at every query split of dab_plan, and the dynamic-conv mask head below, at and
above one 64-point block (the TINY forward instance, the single partial block of the backward).

The regimes are picked from the input sizes by host-side plans in csrc/.  The first part of this file mirrors those plans
in Python and a test without the gpu mark checks that the case lists below reach every regime, so that a retuned plan
constant fails here instead of leaving a path without a test."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "geoformer_amd", "csrc")


# ---- mirrors of the launch plans ---------------------------------------------------------------------------------------
def stage_b_path(nq):
    """k_decoder_stage_b (decoder_layer.hip): QT = ceil(nq / 16) key tiles; two passes over at most 8 or 16 tiles, the
    online soft-max loop beyond."""
    qt = (nq + 15) // 16
    return "two_pass8" if qt <= 8 else "two_pass16" if qt <= 16 else "online"


def dab_qsplit(B, nq, nc):
    """dab_plan (decoder_attn.hip): the number of query slices each context-tile wave of the backward walks."""
    ntiles = (nc + 15) // 16
    qs = (256 * 4 + B * ntiles - 1) // (B * ntiles)
    return max(1, min(qs, nq, 8))


def mask_head_tiny(N):
    """gf_mask_head_episodes (mask_head.hip): the TINY instance of k_mask_head below one 64-point block."""
    return N < 64


def mask_head_bwd_qsplit(N, nq):
    """gf_mask_head_bwd_episodes: query slices of k_mask_head_bwd_feat (one block of 64 points per wave)."""
    nblocks = (N + 63) // 64
    qs = (2 * 256 * 4 + nblocks - 1) // nblocks
    return max(1, min(qs, nq, 16))


# the plans as the sources state them: (file, pattern); a change to one of these lines means the mirror above and the
# case lists below must be checked again
_PLAN_SOURCE = [
    ("decoder_layer.hip", r"const int QT = \(T \+ 15\) >> 4;"),
    ("decoder_layer.hip", r"if \(QT <= 16\) \{"),
    ("decoder_layer.hip", r"if \(QT <= 8\) dl_attn_two_pass<8>"),
    ("decoder_attn.hip", r"int qs = \(256 \* 4 \+ B \* ntiles - 1\) / \(B \* ntiles\);"),
    ("decoder_attn.hip", r"if \(qs > nq\) qs = nq;\s*if \(qs > 8\) qs = 8;\s*if \(qs < 1\) qs = 1;"),
    ("mask_head.hip", r"if \(N < 64\)\s*\\\s*GF_LAUNCH_OP\(GF_OP_MASK_HEAD, \(k_mask_head<GEO_, SPLIT_, true>\)"),
    ("mask_head.hip", r"int qsplit = \(2 \* 256 \* 4 \+ nblocks - 1\) / nblocks;\s*if \(qsplit > nq\) qsplit = nq;\s*"
                      r"if \(qsplit > 16\) qsplit = 16;"),
]

# ---- case lists ----------------------------------------------------------------------------------------------------------
SELF_ATTN_NQ = [1, 15, 16, 17, 127, 128, 129, 255, 256, 257, 300, 512]
# qsplit 1 (the shipped training yaml's batch 16 x 2048 contexts is the same split as 8 x 2048 at 32 queries), 2 (bench.py's
# batch-4 training step), 2 with a ragged last context tile and nq odd, 3 with 50 % 3 != 0, 4, and qsplit = nq = 5 < 8
CROSS_BWD_SHAPES = [(8, 32, 2048), (4, 128, 2048), (4, 127, 2047), (3, 50, 2048), (2, 256, 2048), (1, 5, 17)]
CROSS_FWD_SHAPES = [(1, 1, 1), (2, 7, 15), (4, 128, 2048), (16, 128, 333)]
CROSS_FWD_KERNELS = ["bf3_16wave", "fp32_16wave", "fp32_8wave"]
MASK_N = [1, 17, 63, 64, 65]
MASK_NQ = [1, 5, 37]


def test_case_lists_reach_every_regime():
    for name, pattern in _PLAN_SOURCE:
        with open(os.path.join(CSRC, name)) as f:
            assert re.search(pattern, f.read()), f"{name}: the launch plan changed; update the mirror and the cases of {__file__}"
    # self-attention: both two-pass widths with their last tile full and partial, and the online loop
    paths = {(stage_b_path(nq), nq % 16 == 0, (nq + 15) // 16) for nq in SELF_ATTN_NQ}
    assert ("two_pass8", True, 8) in paths  # the 8th tile filled
    assert any(p == "two_pass8" and not full for p, full, _ in paths)
    assert ("two_pass16", True, 16) in paths
    assert any(p == "two_pass16" and not full for p, full, _ in paths)  # a masked partial tile
    assert any(p == "online" and not full for p, full, _ in paths) and any(p == "online" and full for p, full, _ in paths)
    assert {stage_b_path(nq) for nq in SELF_ATTN_NQ} == {"two_pass8", "two_pass16", "online"}
    # cross-attention backward: qsplit 1..4, qsplit = nq < 8, and a slice count that does not divide nq
    splits = [dab_qsplit(*s) for s in CROSS_BWD_SHAPES]
    assert {1, 2, 3, 4} <= set(splits)
    assert any(qs == nq < 8 for qs, (_, nq, _) in zip(splits, CROSS_BWD_SHAPES))
    assert any(nq % qs for qs, (_, nq, _) in zip(splits, CROSS_BWD_SHAPES))
    assert any(nc % 16 for _, _, nc in CROSS_BWD_SHAPES)
    # cross-attention forward: one partial context tile, one query, batch 4 and 16
    assert any(nc < 16 for _, _, nc in CROSS_FWD_SHAPES) and any(nq == 1 for _, nq, _ in CROSS_FWD_SHAPES)
    assert {4, 16} <= {B for B, _, _ in CROSS_FWD_SHAPES}
    # mask head: both forward instances, the backward's single partial block with the queries split across waves
    assert {mask_head_tiny(N) for N in MASK_N} == {True, False}
    assert any(N < 64 and mask_head_bwd_qsplit(N, nq) == nq > 1 for N in MASK_N for nq in MASK_NQ)
    assert any(N < 64 and nq % mask_head_bwd_qsplit(N, nq) for N in MASK_N for nq in MASK_NQ)


# ---- inference self-attention stage --------------------------------------------------------------------------------------
def _decoder_layer(seed, ff=256):
    from geoformer_amd.model.layers import TransformerDecoderLayer

    torch.manual_seed(seed)
    layer = TransformerDecoderLayer(64, nhead=4, dim_feedforward=ff, dropout=0.1, use_rel=True)
    norm = torch.nn.LayerNorm(64)
    with torch.no_grad():
        for p in list(layer.parameters()) + list(norm.parameters()):
            if p.dim() > 1:
                torch.nn.init.xavier_uniform_(p)
            else:
                p.uniform_(-0.3, 0.3)
        for m in [layer.norm1, layer.norm2, layer.norm3, norm]:
            m.weight.uniform_(0.5, 1.5)
    return layer.cuda().eval(), norm.cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("nq", SELF_ATTN_NQ, ids=lambda nq: f"nq{nq}-{stage_b_path(nq)}")
def test_decoder_token_stage_pre_matches_float64(hip, nq, B):
    """gf_decoder_token_stage with only the pre half (the decoder's first launch: stage A's norm1 and q/k/v projections,
    stage B's self-attention, out_proj + residual, norm2 and the query half of attn_mlp[0]) against its float64
    restatement, at every self-attention path of stage B: two_pass<8> (nq <= 128, the 8th tile filled at 113..128),
    two_pass<16> (nq <= 256, a masked partial tile at 129..255) and the online soft-max loop (nq > 256)."""
    from geoformer_amd import pointops
    from tests.util import decoder_pre_reference

    layer, norm = _decoder_layer(nq + B)
    g = torch.Generator(device="cuda").manual_seed(nq * 10 + B)
    tgt = torch.randn(nq, B, 64, device="cuda", generator=g)
    qp = torch.randn(nq, B, 64, device="cuda", generator=g)
    ff = layer.linear1.out_features
    _, pre = pointops.decoder_stage_tables(layer, norm)
    state = pointops.decoder_token_state(nq, B, tgt.device)
    q1 = torch.empty((B, nq, 64), dtype=torch.float32, device="cuda")
    pointops.decoder_token_stage(None, tgt, qp, nq, B, 4, ff, None, pre, state, None, q1)
    st = state.view(B, 5, nq, 64)  # per scene: X (the target), TGT2 (norm2's output), QKV
    with torch.no_grad():
        r_x, r_t2n, r_q1 = decoder_pre_reference(layer, tgt.transpose(0, 1), qp.transpose(0, 1))
    for what, got, want in (("tgt", st[:, 0], r_x), ("norm2", st[:, 1], r_t2n), ("q1_out", q1, r_q1)):
        err = float((got.double() - want).abs().max())
        assert err < 1e-4, (what, err)


# ---- cross-attention -----------------------------------------------------------------------------------------------------
def _cross_attn_inputs(B, nq, nc, seed):
    """Seeded operands of the cross-attention (the formulation of test_gpu_heads.py's backward test); query 0 of scene 0
    reaches no context, so every context of its row takes the max_geo fall-back."""
    rng = np.random.default_rng(seed)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)  # noqa: E731
    geo = f32(rng.uniform(0, 6, (B, nq, nc)))
    geo[rng.uniform(size=geo.shape) < 0.25] = -1.0
    geo[0, 0] = -1.0
    max_geo = f32(np.where(geo.max(2) < 0, geo.max(), geo.max(2)))
    qloc, cloc = f32(rng.uniform(-3, 3, (B, nq, 3))), f32(rng.uniform(-3, 3, (B, nc, 3)))
    lo, hi = f32(rng.uniform(-3.5, -3, (B, 3))), f32(rng.uniform(6, 7, (B, 3)))
    gaussB = f32(rng.standard_normal((3, 32)))
    Q1, K1, Kv = (f32(rng.standard_normal(s) * 0.7) for s in ((B, nq, 64), (B, nc, 64), (B, nc, 64)))
    W1, W2, Wv = (f32(rng.standard_normal((64, 64)) / 8) for _ in range(3))
    gout = f32(rng.standard_normal((B, nq, 64)))
    return dict(geo=geo, max_geo=max_geo, qloc=qloc, cloc=cloc, lo=lo, hi=hi, gaussB=gaussB, Q1=Q1, K1=K1, Kv=Kv, W1=W1,
                W2=W2, Wv=Wv, gout=gout)


def _cross_attn_reference(t, Q1, K1, Kv, W1, W2, Wv, parts=False):
    """transformer_detr.py:443-454 over the hoisted projections, in the dtype of the tensors t(...) returns; with parts,
    also the embedding R, the pre-activation of H, the soft-max weights and v."""
    g3 = t("geo")[..., None].repeat(1, 1, 1, 3)
    rel = (t("qloc")[:, :, None, :] - t("cloc")[:, None, :, :]).abs()
    g3 = torch.where(g3 < 0, t("max_geo")[:, :, None, None] + rel, g3)
    nrm = (g3 - t("lo")[:, None, None, :]) / (t("hi") - t("lo"))[:, None, None, :]
    proj = (nrm * 6.2831855) @ t("gaussB")
    R = torch.cat([proj.sin(), proj.cos()], -1)
    Hp = R @ W1.t() + Q1[:, :, None, :] - K1[:, None, :, :]
    a = torch.softmax((torch.relu(Hp) @ W2.t()) / 8.0, dim=2)
    v = R @ Wv.t() + Kv[:, None, :, :]
    out = (a * v).sum(2)
    return (out, R, Hp, a, v) if parts else out


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", CROSS_FWD_KERNELS)
@pytest.mark.parametrize("B,nq,nc", CROSS_FWD_SHAPES, ids=[f"B{B}-nq{nq}-nc{nc}" for B, nq, nc in CROSS_FWD_SHAPES])
def test_decoder_cross_attention_forward_kernels_match_float64(hip, B, nq, nc, kernel):
    """The three inference cross-attention kernels against float64: k_decoder_cross_attn_bf3 (the default 16-wave launch),
    k_decoder_cross_attn<16> (gf_dev_cross_attn_bf3(0)) and the 8-wave k_decoder_cross_attn<8> the serving loop launches
    (co_resident_launches).  One context in one partial tile, fewer than 16 contexts, a single query, batches of 4 and
    16, and an all-unreachable query row (the max_geo fall-back for every context)."""
    from geoformer_amd import pointops

    z = _cross_attn_inputs(B, nq, nc, B * 1000 + nq + nc)
    t = lambda k: torch.from_numpy(z[k]).cuda().double()  # noqa: E731  (float64 on the device)
    with torch.no_grad():
        ref = _cross_attn_reference(t, *(t(k) for k in ("Q1", "K1", "Kv", "W1", "W2", "Wv")))
    dv = lambda k: torch.from_numpy(z[k]).cuda()  # noqa: E731
    wpack = pointops.decoder_pack_weights(dv("W1"), dv("W2"), dv("Wv"))
    args = [dv(k) for k in ("geo", "max_geo", "qloc", "cloc", "lo", "hi", "gaussB", "Q1", "K1", "Kv")]
    b2 = torch.zeros(64, device="cuda")
    if kernel == "fp32_8wave":
        with pointops.co_resident_launches():
            out = pointops.decoder_cross_attn(*args, wpack, b2)
    else:
        hip.gf_dev_cross_attn_bf3(1 if kernel == "bf3_16wave" else 0)
        try:
            out = pointops.decoder_cross_attn(*args, wpack, b2)
        finally:
            hip.gf_dev_cross_attn_bf3(-1)
    err = float((out.double() - ref).abs().max())
    assert err < 1e-4, err


@pytest.mark.gpu
@pytest.mark.parametrize("B,nq,nc", CROSS_BWD_SHAPES,
                         ids=[f"B{B}-nq{nq}-nc{nc}-qsplit{dab_qsplit(B, nq, nc)}" for B, nq, nc in CROSS_BWD_SHAPES])
def test_decoder_cross_attention_backward_every_query_split(hip, B, nq, nc):
    """gf_decoder_cross_attn_bwd against float64 autograd at every query split of dab_plan: qsplit 1 (plain stores of
    dK1 / dKv; the split of the shipped training batch), 2 (bench.py's batch-4 training step; also with nq = 127 and a
    ragged context tile), 3 (50 queries: the last slice is short), 4, and qsplit = nq = 5.  Query 0 of scene 0 reaches
    no context.  Outputs to 1e-4; gradients to 1e-4 x max(1, max |ref|), dQ1 / dK1 / dW1 with a flip budget (below).

    The ReLU of H is the one place where fp32 cannot follow float64: a pair whose pre-activation lies within the fp32
    error of H of zero may take the other side of the mask, and then its whole term |W2^T dsim| (up to ~1.5e-4 here)
    moves into or out of dQ1, dK1 and dW1.  So those three are held ELEMENTWISE to 1e-4 x max(1, max |ref|) plus that
    flip budget: the float64 sum of |W2^T dsim| over the pairs whose pre-activation is below 1e-5 in magnitude (a few
    hundred of the 67 M values at 2048 contexts, so most elements get no budget at all).  Measured: dQ1 / dK1 / dW1 reach
    1.35e-4 at (4, 128, 2048), 1.32e-4 at (4, 127, 2047), 1.1e-4 at (2, 256, 2048); the same formulation in float32
    torch reaches 1.31e-4, 0.69e-4 and 1.1e-4 on the same kind of rows; and every element of the kernel's three gradients
    is within 1e-6 x max(1, max |ref|) of float64 once its flip budget is added.  A 1e-6 threshold would not cover
    the kernel's flips at (4, 128, 2048)."""
    from geoformer_amd import pointops

    assert dab_qsplit(B, nq, nc) in (1, 2, 3, 4, nq)
    z = _cross_attn_inputs(B, nq, nc, B * 100 + nq + nc)
    t = lambda k, g=False: torch.from_numpy(z[k]).cuda().double().requires_grad_(g)  # noqa: E731  (float64 on the device)
    names = ("Q1", "K1", "Kv", "W1", "W2", "Wv")
    leaves = [t(k, True) for k in names]
    ref, R, Hp, a, v = _cross_attn_reference(t, *leaves, parts=True)
    gout = t("gout")
    want = torch.autograd.grad((ref * gout).sum(), leaves)
    with torch.no_grad():
        ref = ref.detach()
        flip = (Hp.abs() < 1e-5).double() * ((a * gout[:, :, None, :] * (v - ref[:, :, None, :]) / 8.0) @ leaves[4]).abs()
        budget = {"Q1": flip.sum(2), "K1": flip.sum(1), "W1": torch.einsum("bijc,bijk->ck", flip, R.abs())}
        del Hp, a, v, flip
    dv = lambda k, g=False: torch.from_numpy(z[k]).cuda().requires_grad_(g)  # noqa: E731
    mine = [dv(k, True) for k in names]
    out = pointops.decoder_cross_attn_train(*(dv(k) for k in ("geo", "max_geo", "qloc", "cloc", "lo", "hi", "gaussB")),
                                            *mine)
    err = float((out.detach().double() - ref).abs().max())
    assert err < 1e-4, err
    got = torch.autograd.grad((out * dv("gout")).sum(), mine)
    for name, g_, w_ in zip(names, got, want):
        scale = max(1.0, float(w_.abs().max()))
        err = (g_.double() - w_).abs()
        excess = float((err - 1e-4 * scale - budget.get(name, 0.0)).max())
        assert excess <= 0.0, (name, float(err.max()), scale, excess)


# ---- mask head -----------------------------------------------------------------------------------------------------------
def _mask_head_inputs(N, nq, use_geo, E=1):
    rng = np.random.default_rng(N * 100 + nq * 3 + E + use_geo)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)  # noqa: E731
    feat = f32(rng.standard_normal((N, 16)))
    coords = f32(rng.uniform(-3, 3, (N, 3)))
    qxyz = f32(coords[rng.integers(0, N, nq)])
    geo = mx = None
    if use_geo:
        geo = f32(rng.uniform(0, 5, (nq, N)))
        geo[rng.uniform(size=geo.shape) < 0.3] = -1.0
        geo[-1, 0] = 2.5  # some query reaches something, so the global maximum is a distance
        if nq > 1:
            geo[0] = -1.0  # a query that reaches nothing takes the global maximum
        m = geo.max(1)
        mx = f32(np.sqrt(np.where(m < 0, m.max(), m)))
    params = f32(rng.standard_normal((E, nq, 337)) * 0.3)
    gout = f32(rng.standard_normal((nq, N)) * (rng.uniform(size=(nq, N)) < 0.5))
    return feat, coords, geo, qxyz, mx, params, gout


def _mask_head_reference(F_, P, coords, geo, qxyz, mx):
    """geoformer.py:286-324 in float64 (test_gpu_heads.py's formula) for one parameter set P [nq, 337] (packed
    w1 | w2 | b1 | b2)."""
    nq, N = qxyz.shape[0], F_.shape[0]
    t64 = lambda a: torch.from_numpy(a.astype(np.float64))  # noqa: E731
    w1 = P[:, :304].reshape(nq, 16, 19)
    w2, b1, b2 = P[:, 304:320], P[:, 320:336], P[:, 336]
    rel = t64(qxyz)[:, None, :] - t64(coords)[None]
    if geo is not None:
        rel = torch.where(t64(geo)[..., None] < 0, rel + t64(mx)[:, None, None] * torch.sign(rel), rel)
    x = torch.cat([rel, F_[None].expand(nq, N, 16)], 2)
    h = torch.relu(torch.einsum("qck,qnk->qnc", w1, x) + b1[:, None, :])
    return torch.einsum("qc,qnc->qn", w2, h) + b2[:, None]


@pytest.mark.gpu
@pytest.mark.parametrize("use_geo", [True, False], ids=["geo", "nogeo"])
@pytest.mark.parametrize("nq", MASK_NQ)
@pytest.mark.parametrize("N", MASK_N, ids=lambda N: f"N{N}-{'tiny' if mask_head_tiny(N) else 'blocks'}")
def test_mask_head_forward_small_scenes(hip, N, nq, use_geo):
    """The mask head's forward below, at and just above one 64-point block (N < 64: the TINY instance of k_mask_head),
    under split=True (bf16 three-piece products) and split=False (fp32 MFMA), dense parameters and three episodes in
    one launch (mask_head_episodes: every episode's slice), against float64."""
    from geoformer_amd import pointops

    E = 3
    feat, coords, geo, qxyz, mx, params, _ = _mask_head_inputs(N, nq, use_geo, E)
    d = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    refs = [_mask_head_reference(torch.from_numpy(feat).double(), torch.from_numpy(params[e]).double(), coords, geo, qxyz,
                                 mx).numpy() for e in range(E)]
    P = params[0]
    w1, w2, b1, b2 = P[:, :304].reshape(nq, 16, 19), P[:, 304:320], P[:, 320:336], P[:, 336]
    for split in (True, False):
        out = pointops.mask_head(d(feat), d(coords), d(geo), d(qxyz), d(mx), d(w1), d(b1), d(w2), d(b2),
                                 split=split).cpu().numpy()
        assert np.abs(out - refs[0]).max() < 1e-4, ("dense", split, np.abs(out - refs[0]).max())
        eps = pointops.mask_head_episodes(d(feat), d(coords), d(geo), d(qxyz), d(mx), d(params), split=split).cpu().numpy()
        for e in range(E):
            assert np.abs(eps[e] - refs[e]).max() < 1e-4, ("episode", e, split, np.abs(eps[e] - refs[e]).max())


@pytest.mark.gpu
@pytest.mark.parametrize("use_geo", [True, False], ids=["geo", "nogeo"])
@pytest.mark.parametrize("nq", MASK_NQ)
@pytest.mark.parametrize("N", MASK_N, ids=lambda N: f"N{N}-{'one-partial-block' if N < 64 else 'blocks'}")
def test_mask_head_backward_small_scenes(hip, N, nq, use_geo):
    """gf_mask_head_bwd below, at and just above one 64-point block: with N < 64 the feature gradient is ONE partial
    block whose queries are split over min(nq, 16) waves (atomics into dfeat, a short last slice at nq = 37); against
    float64 autograd, with test_gpu_heads.py's bounds."""
    from geoformer_amd import pointops

    feat, coords, geo, qxyz, mx, params, gout = _mask_head_inputs(N, nq, use_geo)
    F_ = torch.from_numpy(feat.astype(np.float64)).requires_grad_()
    P = torch.from_numpy(params[0].astype(np.float64)).requires_grad_()
    ref = _mask_head_reference(F_, P, coords, geo, qxyz, mx)
    (ref * torch.from_numpy(gout.astype(np.float64))).sum().backward()
    d = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    f, p = d(feat).requires_grad_(), d(params[0]).requires_grad_()
    out = pointops.mask_head_train(f, p, d(coords), d(geo), d(qxyz), d(mx))
    assert np.abs(out.detach().cpu().numpy() - ref.detach().numpy()).max() < 1e-4
    (out * d(gout)).sum().backward()
    gf, gp = f.grad.cpu().numpy(), p.grad.cpu().numpy()
    rf, rp = F_.grad.numpy(), P.grad.numpy()
    assert np.abs(gf - rf).max() < 1e-4 * max(1.0, np.abs(rf).max()), (np.abs(gf - rf).max(), np.abs(rf).max())
    assert np.abs(gp - rp).max() < 2e-5 * max(1.0, np.abs(rp).max()), (np.abs(gp - rp).max(), np.abs(rp).max())


# ---- whole eval forward above 256 queries --------------------------------------------------------------------------------
@pytest.mark.gpu
def test_forward_with_300_queries_matches_oracle_backend(hip, oracle):
    """One eval forward with n_query_points = 300 (every decoder token stage through stage B's online soft-max loop) and
    n_decode_point = 512 on a batch of two small scenes, against the same forward through the oracle's operators on the
    host: foreground set, FPS picks and geodesic rows bit-exact, floats to the bounds of the edge-case forward test."""
    from geoformer_amd import scene
    from geoformer_amd.model import GeoFormer, load_config
    from oracle import cpu_backend
    from tests.util import synthetic_state_dict

    assert stage_b_path(300) == "online"

    def run(device):
        m = GeoFormer(load_config("test_geoformer_scannet.yaml", n_decode_point=512, n_query_points=300))
        m.load_state_dict(synthetic_state_dict(m.state_dict(), 0))
        with torch.no_grad():
            m.semantic_linear.bias[4:] += 2.0  # most points foreground
        m.to(device)
        m.eval()
        batch = scene.make_batch([scene.make_small_scene(6000, 31), scene.make_small_scene(4000, 32)])
        batch = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in batch.items()}
        cap = {}
        dec = m.forward_decoder

        def dec_w(cl, cf, ql, pc, geo, pei):
            cap["pei"], cap["cl"] = pei.detach().cpu(), cl.detach().cpu()
            cap["geo"] = [g.detach().cpu() for g in geo]
            return dec(cl, cf, ql, pc, geo, pei)

        m.forward_decoder = dec_w
        np.random.seed(23)
        with torch.no_grad():
            out = m(batch, 300, training=False)
        return out, cap

    got, cg = run("cuda")
    with cpu_backend.installed():
        ref, cc = run("cpu")
    assert (got["semantic_scores"].cpu() - ref["semantic_scores"]).abs().max() < 1e-4
    assert torch.equal(got["fg_idxs"].cpu(), ref["fg_idxs"]) and got["fg_idxs"].numel() > 1024
    assert torch.equal(cg["pei"], cc["pei"]) and torch.equal(cg["cl"], cc["cl"])
    for a, b in zip(cg["geo"], cc["geo"]):
        assert torch.equal(a, b)
    mg, mc = got["mask_predictions"][-1], ref["mask_predictions"][-1]
    assert (mg["cls_logits"].cpu() - mc["cls_logits"]).abs().max() < 1e-4
    for a, b in zip(mg["mask_logits"], mc["mask_logits"]):
        assert (a.cpu() - b).abs().max() < 1e-4 * max(1.0, float(b.abs().max()))
