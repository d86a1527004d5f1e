"""GPU: the backbone at widths other than the shipped m = 16.

GeoFormer's U-Net levels are m, 2m, ... 7m wide, and at every width-dependent site the Python side picks a native kernel
or the module route by a width predicate.  Each predicate promises that the kernel behind it is
exact for every width it admits; these tests hold the kernels to that at the widths the other configurations reach:
the inference voxel transformer (gf_backbone_transformer) against a float64 restatement of its modules from 16 to 384
channels, and the eval forward, the native U-Net training executor and a whole training step at m = 8, 12, 24, 32,
each of which also asserts which routes it took."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------------------------------------------------------
# inference voxel transformer (csrc/backbone_attn.hip, bt_forward) against float64

_TR_CASES = [(c, 2) for c in (16, 48, 128, 144, 192, 224, 384)] + [(16, 1), (16, 4), (224, 1), (224, 4)]
_LAYOUTS = {"one-token": [1], "tile-edges": [15, 16, 17], "empty-middle": [40, 0, 33], "many-key-tiles": [1500]}


def _tr_stack(c, n_layers, seed):
    from geoformer_amd.model.layers import BackboneTransformer

    torch.manual_seed(seed)
    before = torch.nn.Linear(c, 128)
    tr = BackboneTransformer(d_model=128, N=n_layers, heads=4, d_ff=64)
    after = torch.nn.Linear(128, c)
    with torch.no_grad():
        for p in tr.parameters():
            if p.dim() == 1:  # Norm alpha/bias and Linear biases away from their 1/0 defaults
                p.add_(torch.randn_like(p) * 0.2)
    tr.eval()
    return before, tr, after


def _tr_reference_float64(before, tr, after, feats, xyz, counts):
    """The modules' own forward (BackboneTransformer.forward's per-scene loop, layers.py) on float64 copies of them; the
    loop is restated only because the module computes its positional input in float32."""
    before, tr, after = (copy.deepcopy(m).double() for m in (before, tr, after))
    out = torch.zeros(feats.shape[0], after.out_features, dtype=torch.float64)
    s = 0
    with torch.no_grad():
        for n in counts:
            if n:
                pts = xyz[s:s + n].double()
                rel = (pts.unsqueeze(1) - pts.unsqueeze(0)).mean(dim=1)
                x = (before(feats[s:s + n].double()) + tr.position_linear(rel)).unsqueeze(0)
                for layer in tr.layers:
                    x = layer(x, mask=None)
                out[s:s + n] = after(tr.norm(x).squeeze(0))
            s += n
    return out


@pytest.mark.parametrize("layout", list(_LAYOUTS), ids=list(_LAYOUTS))
@pytest.mark.parametrize("c,n_layers", _TR_CASES, ids=[f"c{c}-L{n}" for c, n in _TR_CASES])
def test_backbone_transformer_matches_float64(hip, c, n_layers, layout):
    """gf_backbone_transformer against the same Linear -> BackboneTransformer -> Linear modules in float64 on the host.
    Widths above 128 exercise the output projection's column tiles beyond one per wave (k_bt_layer's last phase) and the
    first product's generic path (k_bt_pre); 1 and 4 layers the ends of BT_MAXL; 15/16/17 tokens the tile edges; an empty
    scene between two others the tile tables; 1 500 tokens a long online soft-max over 94 key tiles."""
    from geoformer_amd import pointops

    counts = _LAYOUTS[layout]
    before, tr, after = _tr_stack(c, n_layers, 1000 + c + 7 * n_layers)
    assert pointops.backbone_transformer_supported(c, tr)
    M = sum(counts)
    g = torch.Generator().manual_seed(c + M)
    coords = torch.cat([torch.cat([torch.full((n, 1), b), torch.randint(0, 16, (n, 3), generator=g)], 1)
                        for b, n in enumerate(counts)]).int()
    feats = torch.randn(M, c, generator=g)
    ref = _tr_reference_float64(before, tr, after, feats, coords[:, 1:], counts)
    # the bound below is absolute: it means what it says only on outputs of order one
    assert 0.2 < float(ref.abs().max()) < 10.0
    for m in (before, tr, after):
        m.cuda()
    with torch.no_grad():
        table, nl = pointops.backbone_transformer_params(before, tr, after)
        assert nl == n_layers
        offs = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32).cuda()
        out = pointops.backbone_transformer(feats.cuda(), coords.cuda(), offs, len(counts), table, nl)
    torch.cuda.synchronize()
    assert out.shape == (M, c)
    err = (out.cpu().double() - ref).abs()
    worst = int(err.max(0).values.argmax())
    assert float(err.max()) < 1e-4, f"max |diff| {float(err.max()):.3g}, worst column {worst} of {c}"


# ------------------------------------------------------------------------------------------------------------------
# the model at other widths: every route the width predicates choose, against the oracle-backed host forward / step

def _record_transformer_routes(monkeypatch, model, fn_name):
    """Widths of the levels whose voxel transformer ran natively (calls of pointops.<fn_name>) and of those that took the
    module route (calls of their before_transformer_linear, which the native forms read but never call)."""
    from geoformer_amd import pointops

    native, modules = [], []
    fn = getattr(pointops, fn_name)

    def wrapped(feats, *args, **kw):
        native.append(int(feats.shape[1]))
        return fn(feats, *args, **kw)

    monkeypatch.setattr(pointops, fn_name, wrapped)
    for u in model.modules():
        if getattr(u, "before_transformer_linear", None) is not None:
            u.before_transformer_linear.register_forward_hook(lambda mod, inp, out: modules.append(int(inp[0].shape[1])))
    return native, modules


# m -> (levels whose inference transformer is fused, levels on the module route): a level of width c is fused iff
# pointops.backbone_transformer_supported(c, ...) -- c % 16 == 0 and c <= 384
_EVAL_ROUTES = {8: ([48], [56]), 24: ([144], [168]), 32: ([192, 224], [])}


@pytest.mark.parametrize("width", sorted(_EVAL_ROUTES), ids=[f"m{w}" for w in sorted(_EVAL_ROUTES)])
def test_eval_forward_matches_oracle_backend_at_width(hip, oracle, monkeypatch, width):
    """The whole eval forward of a model of width m (levels m .. 7m) on two scenes: the GPU forward against the same
    forward through the oracle's operators on the host, as test_gpu_model.py's edge-case test does at m = 16.  At these
    widths the native U-Net executor and the fused mask head are not taken (their predicates admit m = 16 only), so the
    per-level modules, the inference voxel transformer at the widths above and the module fallbacks run."""
    from geoformer_amd import scene
    from geoformer_amd.model import GeoFormer, load_config
    from oracle import cpu_backend
    from tests.util import synthetic_state_dict

    routes = {}

    def run(device):
        m = GeoFormer(load_config("test_geoformer_scannet.yaml", m=width, n_decode_point=512, n_query_points=64))
        m.load_state_dict(synthetic_state_dict(m.state_dict(), 0))
        m.to(device)
        m.eval()
        if device == "cuda":
            routes["native"], routes["modules"] = _record_transformer_routes(monkeypatch, m, "backbone_transformer")
        batch = scene.make_batch([scene.make_small_scene(8192, 9), scene.make_small_scene(5000, 10)])
        batch = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in batch.items()}
        cap = {}
        dec = m.forward_decoder

        def dec_w(cl, cf, ql, pc, geo, pei):
            cap["pei"], cap["cl"] = pei.detach().cpu(), cl.detach().cpu()
            cap["geo"] = [g.detach().cpu() for g in geo]
            return dec(cl, cf, ql, pc, geo, pei)

        m.forward_decoder = dec_w
        np.random.seed(21)
        with torch.no_grad():
            out = m(batch, 300, training=False)
        return out, cap

    got, cg = run("cuda")
    torch.cuda.synchronize()
    fused, mod = _EVAL_ROUTES[width]
    assert sorted(routes["native"]) == fused and sorted(routes["modules"]) == mod, routes
    with cpu_backend.installed():
        ref, cc = run("cpu")
    # (the bounds are the m = 16 test's 1e-4, relative to the magnitude where a width makes the outputs larger than one)
    sr = ref["semantic_scores"]
    assert float((got["semantic_scores"].cpu() - sr).abs().max()) < 1e-4 * max(1.0, float(sr.abs().max()))
    assert torch.equal(got["fg_idxs"].cpu(), ref["fg_idxs"]) and got["fg_idxs"].numel() > 1000
    assert torch.equal(cg["pei"], cc["pei"]) and torch.equal(cg["cl"], cc["cl"])  # FPS picks of both scenes
    for a, b in zip(cg["geo"], cc["geo"]):
        assert torch.equal(a, b)  # reach sets and fp32 path sums, bit for bit
    mg, mc = got["mask_predictions"][-1], ref["mask_predictions"][-1]
    cr = mc["cls_logits"]
    assert float((mg["cls_logits"].cpu() - cr).abs().max()) < 1e-4 * max(1.0, float(cr.abs().max()))
    for a, b in zip(mg["mask_logits"], mc["mask_logits"]):
        assert (a.cpu() - b).abs().max() < 1e-4 * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize("width", [8, 12], ids=["m8", "m12"])
def test_unet_train_exec_matches_module_route_at_width(hip, width):
    """gf_unet_train_fwd / _bwd at the other widths unet_train.supported admits (levels 8..56 and 12..84: most of them not
    multiples of 16) against the module tree in training mode, with test_gpu_unet_exec.py's bounds."""
    import copy

    from geoformer_amd import scene, unet_train
    from geoformer_amd.model import GeoFormer, load_config
    from tests.test_gpu_unet_exec import _train_backbone
    from tests.util import synthetic_state_dict

    m = GeoFormer(load_config("geoformer_scannet.yaml", batch_size=2, m=width))
    m.load_state_dict(synthetic_state_dict(m.state_dict(), 3))
    m.cuda()
    m.train()
    for mod in m.modules():  # (the voxel transformers' dropout would make two forwards differ)
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    batch = scene.make_batch([scene.make_small_scene(6000, 7), scene.make_small_scene(9000, 8)])
    batch = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in batch.items()}
    assert unet_train.supported(m, m.preprocess_input(batch, 2))
    state = copy.deepcopy(m.state_dict())
    f_ref, g_ref, s_ref = _train_backbone(m, batch, native=False, seed=1)
    assert "_gf_unet_train_prog" not in m.__dict__
    m.load_state_dict(state)  # the running statistics back to where they were
    f_nat, g_nat, s_nat = _train_backbone(m, batch, native=True, seed=1)
    assert "_gf_unet_train_prog" in m.__dict__  # the native executor ran
    assert f_nat.shape == f_ref.shape and f_nat.shape[1] == width
    assert float((f_nat - f_ref).abs().max()) <= 2e-6 * max(1.0, float(f_ref.abs().max()))
    for n in s_ref:
        assert float((s_nat[n] - s_ref[n]).abs().max()) <= 1e-6 * max(1.0, float(s_ref[n].abs().max())), n
    assert set(g_nat) == set(g_ref)
    top = max(float(g.norm()) for g in g_ref.values())
    for n, gr in g_ref.items():
        gn = g_nat[n]
        assert gn.shape == gr.shape, n
        ref = float(gr.norm())
        assert float((gn - gr).norm()) <= 5e-3 * max(ref, 1e-5 * top), (n, float((gn - gr).norm()), ref)


# m -> (levels whose training transformer is native, levels on the module route): at 8 inside the native U-Net
# executor, at 24 from the module tree (unet_train.supported: 2 * 168 > 256)
_TRAIN_ROUTES = {8: ([48], [56]), 24: ([144], [168])}


@pytest.mark.parametrize("width", sorted(_TRAIN_ROUTES), ids=[f"m{w}" for w in sorted(_TRAIN_ROUTES)])
def test_training_step_matches_oracle_backend_at_width(hip, oracle, monkeypatch, width):
    """A whole training step (forward, criterion, backward) of a model of width m on the GPU against the same step through
    the oracle's operators on the host, with test_training_step.py's bounds: loss, per-module gradient norms and every
    gradient element."""
    from oracle import cpu_backend
    from tests.test_training_step import _compare_grads, _grads, _setup, _step, _summ

    with cpu_backend.installed():
        _, m, crit, batch = _setup("cpu", width=width)
        loss_c, _, n_c = _step(m, crit, batch, 5)
        g_c = _grads(m)
    _, mg, critg, batchg = _setup("cuda", width=width)
    native, modules = _record_transformer_routes(monkeypatch, mg, "backbone_transformer_train")
    loss_g, _, n_g = _step(mg, critg, batchg, 5)
    fused, mod = _TRAIN_ROUTES[width]
    assert sorted(native) == fused and sorted(modules) == mod, (native, modules)
    assert ("_gf_unet_train_prog" in mg.__dict__) == (width == 8)  # the native U-Net training executor
    assert abs(loss_g - loss_c) < 1e-3 * max(1.0, abs(loss_c))
    gc, gg = _summ(n_c), _summ(n_g)
    for k in gc:
        assert abs(gg[k] - gc[k]) <= 2e-3 * max(gc[k], 1e-3), (k, gc[k], gg[k])
    _compare_grads(g_c, _grads(mg), 4e-3)  # every parameter, element by element
