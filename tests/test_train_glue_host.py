"""The hand-written autograd functions between the training kernels that are plain PyTorch (split-K linear, chunked
pointwise convolution, row gather without repeats), called directly in float64 on the host against plain autograd of the
same expression: every input gradient to 1e-12 relative, at row counts on both sides of each chunking threshold, with a
remainder chunk, and with incoming gradients that are contiguous, transposed views or expanded."""
import pytest
import torch
import torch.nn.functional as F

TOL = 1e-12


def _rel(got, ref):
    assert got.shape == ref.shape
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)


def _loss(y, mode, G):
    """A scalar whose gradient reaches y as G: as it lies ("contig"), as a transposed view of a [..., C, rows] producer
    ("transposed"), or as the expanded scalar of y.sum() ("expanded")."""
    if mode == "contig":
        return (y * G).sum()
    if mode == "transposed":
        return (y.transpose(-1, -2) * G.transpose(-1, -2).contiguous()).sum()
    assert mode == "expanded"
    return y.sum()


_LINEAR_SHAPES = [((255,), 16, 13), ((256,), 16, 13), ((4096,), 16, 16), ((4133,), 16, 13), ((16389,), 16, 13),
                  ((70000,), 16, 13), ((16, 300), 64, 64)]


@pytest.mark.parametrize("gmode", ["contig", "transposed", "expanded"])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("lead,cin,cout", _LINEAR_SHAPES)
def test_split_k_linear_matches_plain_autograd_float64(lead, cin, cout, bias, gmode):
    from geoformer_amd.model.layers import _SplitKLinearFn

    g = torch.Generator().manual_seed(sum(lead) + cin + cout)
    x = torch.randn(*lead, cin, dtype=torch.float64, generator=g)
    w = torch.randn(cout, cin, dtype=torch.float64, generator=g) / cin ** 0.5
    b = torch.randn(cout, dtype=torch.float64, generator=g) if bias else None
    G = torch.randn(*lead, cout, dtype=torch.float64, generator=g)
    leaves = [t.clone().requires_grad_() for t in (x, w)] + ([b.clone().requires_grad_()] if bias else [None])
    ref_leaves = [t.clone().requires_grad_() for t in (x, w)] + ([b.clone().requires_grad_()] if bias else [None])
    y = _SplitKLinearFn.apply(*leaves)
    assert "_SplitKLinearFn" in y.grad_fn.name()
    yr = F.linear(*ref_leaves)
    assert _rel(y.detach(), yr.detach()) <= TOL
    _loss(y, gmode, G).backward()
    _loss(yr, gmode, G).backward()
    for name, got, ref in zip(("gx", "gw", "gb"), leaves, ref_leaves):
        if got is not None:
            assert _rel(got.grad, ref.grad) <= TOL, name


@pytest.mark.parametrize("views", [False, True])
@pytest.mark.parametrize("B,Ci,Co,L", [(1, 16, 16, 32768), (1, 16, 16, 32845), (2, 19, 32, 40001), (1, 16, 8, 100),
                                       (3, 7, 5, 385)])
def test_pointwise_split_k_matches_plain_autograd_float64(B, Ci, Co, L, views):
    """views: x and the incoming gradient both arrive as transposed views of [B, L, C] tensors."""
    from geoformer_amd.model.layers import _PointwiseSplitKFn

    g = torch.Generator().manual_seed(B + Ci + Co + L)
    xt = torch.randn(B, L, Ci, dtype=torch.float64, generator=g)
    w = torch.randn(Co, Ci, dtype=torch.float64, generator=g) / Ci ** 0.5
    G = torch.randn(B, Co, L, dtype=torch.float64, generator=g)

    def run(fn):
        if views:
            leaf = xt.clone().requires_grad_()
            x = leaf.transpose(1, 2)
            assert not x.is_contiguous()
        else:
            leaf = xt.transpose(1, 2).contiguous().requires_grad_()
            x = leaf
        wl = w.clone().requires_grad_()
        y = fn(x, wl)
        _loss(y, "transposed" if views else "contig", G).backward()
        return y, leaf.grad, wl.grad

    y, gx, gw = run(_PointwiseSplitKFn.apply)
    assert "_PointwiseSplitKFn" in y.grad_fn.name()
    yr, gxr, gwr = run(lambda x, wl: torch.einsum("oi,bil->bol", wl, x))
    assert _rel(y.detach(), yr.detach()) <= TOL
    assert _rel(gx, gxr) <= TOL
    assert _rel(gw, gwr) <= TOL


@pytest.mark.parametrize("shape,gmode", [((5003, 16), "contig"), ((5003, 16), "transposed"), ((5003,), "contig")])
def test_take_rows_unique_fn_matches_plain_indexing_float64(shape, gmode):
    from geoformer_amd.pointops import _TakeRowsUniqueFn

    g =torch.Generator().manual_seed(shape[0])
    x = torch.randn(*shape, dtype=torch.float64, generator=g)
    idx = torch.randperm(shape[0], generator=g)[:3001]  # unsorted, no repeats
    assert bool((idx[1:] < idx[:-1]).any())
    G = torch.randn(3001, *shape[1:], dtype=torch.float64, generator=g)
    a, r = x.clone().requires_grad_(), x.clone().requires_grad_()
    y = _TakeRowsUniqueFn.apply(a, idx)
    assert "_TakeRowsUniqueFn" in y.grad_fn.name()
    yr = r[idx]
    assert torch.equal(y.detach(), yr.detach())
    _loss(y, gmode, G).backward()
    _loss(yr, gmode, G).backward()
    assert _rel(a.grad, r.grad) <= TOL
