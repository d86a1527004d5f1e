"""Training step (BASELINE config 3 shape: rulebook + forward + criterion + backward + Adam).

CPU: the build's model/criterion through the oracle-backed operators (host logic, autograd plumbing).
GPU: the same step through the HIP forward/backward kernels; loss and per-module gradient norms must agree
with the CPU/oracle run (dropout 0 as SURVEY.md section 7 prescribes for training parity)."""
import numpy as np
import pytest
import torch


def _setup(device, full=False, batch4=False, width=None):
    """width: the backbone width (STRUCTURE.m) in place of the yaml's 16."""
    from geoformer_amd import scene
    from geoformer_amd.model import GeoFormer, InstSetCriterion, load_config
    from tests.util import synthetic_state_dict

    if full:  # the train yaml as shipped (nq=128, nc=2048), two room-sized scenes (batch4: BASELINE config 3's four)
        cfg = load_config("geoformer_scannet.yaml", batch_size=4 if batch4 else 2, dec_dropout=0.0, prepare_epochs=1)
    else:
        cfg = load_config("geoformer_scannet.yaml", batch_size=2, dec_dropout=0.0, n_decode_point=128, n_query_points=16,
                          prepare_epochs=1)
    if width is not None:
        cfg.m = width
    torch.manual_seed(0)
    m = GeoFormer(cfg)
    m.load_state_dict(synthetic_state_dict(m.state_dict(), 1))
    for mod in m.modules():  # backbone-transformer dropouts off as well
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    m.to(device)
    m.train()
    if full and batch4:
        batch = scene.make_batch([scene.make_scene(n, sd) for n, sd in ((150_000, 50), (120_000, 51), (180_000, 52),
                                                                        (100_000, 53))])
    elif full:
        batch = scene.make_batch([scene.make_scene(150_000, 41), scene.make_scene(110_000, 42)])
    else:
        batch = scene.make_batch([scene.make_small_scene(2500, 31), scene.make_small_scene(2000, 32)])
    batch = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in batch.items()}
    return cfg, m, InstSetCriterion(cfg), batch


def _step(m, crit, batch, epoch, preds=None, cap=None):
    """preds: class decisions (integers) of another run, handed to this one after checking that its own differ on
    near-ties only -- with 10^5 points per scene two fp32 evaluations of the semantic head disagree on a handful of
    arg-max ties, and one point more or less in a scene's foreground changes the host-RNG draws of the whole step.
    cap: dict that receives this run's own decisions."""
    if preds is not None or cap is not None:
        fb = m.forward_backbone

        def fb_w(batch_input, batch_size, want_preds=True):
            feats, sem, own = fb(batch_input, batch_size, want_preds=True)
            if cap is not None:
                cap["preds"] = own.detach().cpu()
            if preds is None:
                return feats, sem, own
            diff = torch.nonzero(own.cpu() != preds).view(-1)
            top2 = torch.sort(sem.detach().cpu()[diff].double(), dim=1)[0][:, -2:]
            assert diff.numel() <= 32 and (diff.numel() == 0 or float((top2[:, 1] - top2[:, 0]).max()) < 1e-3), diff.numel()
            return feats, sem, preds.to(own.device)

        m.forward_backbone = fb_w
    np.random.seed(3)
    out = m(batch, epoch)
    loss, info = crit(out, batch, epoch)
    m.zero_grad()
    loss.backward()
    norms = {n: float(p.grad.norm()) for n, p in m.named_parameters() if p.grad is not None}
    return float(loss), info, norms


def _grads(m):
    return {n: p.grad.detach().cpu().double().numpy() for n, p in m.named_parameters() if p.grad is not None}


def _compare_grads(g_ref, g_got, tol, etol=0.15):
    """Per parameter, element-wise: the cosine between the two gradients and their norms to `tol`, every single element to
    `etol` of the parameter's largest entry -- a sign flip or a permutation inside a module cannot hide behind a norm.
    (Two fp32 evaluations put a few pre-activations of the deepest levels -- a few dozen voxels -- on different sides of a
    ReLU, which moves single elements of those levels' gradients by several percent of the largest entry (up to 9e-2 on
    the 2 500-point test scenes; a sign flip or a permutation would be > 100 %) while direction and norm hold 3e-3.)  Gradients that are zero by construction (biases in front of a normalisation / soft-max) are
    rounding noise on both sides: everything is measured against a floor of 1e-5 of the largest parameter gradient."""
    gmax = max(float(np.linalg.norm(v)) for v in g_ref.values())
    floor = 1e-5 * gmax
    bad = []
    for n, r in g_ref.items():
        g = g_got.get(n)
        rn = float(np.linalg.norm(r))
        if g is None:
            if rn > floor:
                bad.append((n, "missing", rn))
            continue
        scale = max(float(np.abs(r).max()), rn / np.sqrt(r.size), floor)
        err = float(np.abs(g - r).max()) / scale
        gn = float(np.linalg.norm(g))
        cos = float((g * r).sum()) / max(gn * rn, 1e-300)
        nerr = abs(gn - rn) / max(rn, floor)
        if err > etol or nerr > tol or (rn > 100 * floor and cos < 1 - tol):
            bad.append((n, round(err, 5), round(nerr, 6), round(1 - cos, 8)))
    extra = [n for n in g_got if n not in g_ref and float(np.linalg.norm(g_got[n])) > floor]
    assert not bad and not extra, "\n".join(str(b) for b in bad[:12] + extra[:8])


def _summ(norms):
    groups = {}
    for n, v in norms.items():
        groups.setdefault(n.split(".")[0], 0.0)
        groups[n.split(".")[0]] += v * v
    return {k: v ** 0.5 for k, v in groups.items()}


def test_training_step_cpu_oracle_backend(oracle):
    from oracle import cpu_backend

    with cpu_backend.installed():
        cfg, m, crit, batch = _setup("cpu")
        loss0, info0, n0 = _step(m, crit, batch, 1)  # epoch <= prepare_epochs: backbone + semantic head only
        assert np.isfinite(loss0) and set(info0) == {"sem_loss", "loss"}
        assert any(k.startswith("unet") for k in n0) and not any(k.startswith("decoder") for k in n0)
        loss1, info1, n1 = _step(m, crit, batch, 5)
        assert np.isfinite(loss1) and {"focal_loss", "dice_loss", "cls_loss"} <= set(info1)
        g = _summ(n1)
        for k in ("unet", "input_conv", "set_aggregator", "decoder", "controller", "mask_tower"):
            assert g[k] > 0 and np.isfinite(g[k]), k
        opt = torch.optim.Adam(m.parameters(), lr=1e-3)
        opt.step()
        loss2, _, _ = _step(m, crit, batch, 5)
        assert np.isfinite(loss2)


@pytest.mark.gpu
def test_training_step_gpu_matches_oracle_backend(hip, oracle):
    from oracle import cpu_backend

    with cpu_backend.installed():
        cfg, m, crit, batch = _setup("cpu")
        loss_c, _, n_c = _step(m, crit, batch, 5)
        g_c = _grads(m)
    cfg, mg, critg, batchg = _setup("cuda")
    loss_g, _, n_g = _step(mg, critg, batchg, 5)
    assert abs(loss_g - loss_c) < 1e-3 * max(1.0, abs(loss_c))
    gc, gg = _summ(n_c), _summ(n_g)
    for k in gc:
        assert abs(gg[k] - gc[k]) <= 2e-3 * max(gc[k], 1e-3), (k, gc[k], gg[k])
    _compare_grads(g_c, _grads(mg), 4e-3)  # every parameter, element by element
    torch.optim.Adam(mg.parameters(), lr=1e-3).step()


@pytest.mark.gpu
def test_training_step_full_size_gpu_matches_oracle_backend(hip, oracle):
    """BASELINE config 3 at scene size (two scenes, 260k points, the train yaml's nq=128 / nc=2048): the level-1
    counted-loop kernels in the forward and the input gradient, the weight gradient over ~900k rules, the fused
    backward of cross-attention and mask head over 30 000-point samples, the device criterion -- loss and per-module
    gradient norms against the same step through the oracle's operators on the host."""
    from oracle import cpu_backend
    from oracle import oracle as orc

    L = orc.lib()
    L.orc_set_threads.restype = int
    L.orc_set_threads(64)
    cap = {}
    cfg, mg, critg, batchg = _setup("cuda", full=True)
    loss_g, _, n_g = _step(mg, critg, batchg, 5, cap=cap)
    with cpu_backend.installed():
        cfg, m, crit, batch = _setup("cpu", full=True)
        loss_c, _, n_c = _step(m, crit, batch, 5, preds=cap["preds"])
        g_c = _grads(m)
    del m, batch
    assert abs(loss_g - loss_c) < 1e-3 * max(1.0, abs(loss_c)), (loss_g, loss_c)
    gc, gg = _summ(n_c), _summ(n_g)
    for k in gc:
        assert abs(gg[k] - gc[k]) <= 2e-3 * max(gc[k], 1e-3), (k, gc[k], gg[k])
    _compare_grads(g_c, _grads(mg), 3e-3)  # every parameter, element by element


@pytest.mark.gpu
def test_training_step_batch4_550k_gpu_matches_oracle_backend(hip, oracle):
    """BASELINE config 3 as named: batch 4 (150k + 120k + 180k + 100k = 550k points), the train yaml with
    batch_size 4: loss, per-module gradient norms and every parameter's gradient element by element against the same
    step through the oracle's operators on the host."""
    from oracle import cpu_backend
    from oracle import oracle as orc

    L = orc.lib()
    L.orc_set_threads.restype = int
    L.orc_set_threads(64)
    cap = {}
    cfg, mg, critg, batchg = _setup("cuda", full=True, batch4=True)
    assert int(batchg["locs"].shape[0]) > 540_000
    loss_g, _, n_g = _step(mg, critg, batchg, 5, cap=cap)
    with cpu_backend.installed():
        cfg, m, crit, batch = _setup("cpu", full=True, batch4=True)
        loss_c, _, n_c = _step(m, crit, batch, 5, preds=cap["preds"])
        g_c = _grads(m)
    del m, batch
    assert abs(loss_g - loss_c) < 1e-3 * max(1.0, abs(loss_c)), (loss_g, loss_c)
    gc, gg = _summ(n_c), _summ(n_g)
    for k in gc:
        assert abs(gg[k] - gc[k]) <= 2e-3 * max(gc[k], 1e-3), (k, gc[k], gg[k])
    _compare_grads(g_c, _grads(mg), 3e-3)


def _fs_setup(device):
    """Few-shot training-mode episode (BASELINE config 4, training variant): geoformer_fs_scannet.yaml with a batch of
    two query scenes, one full-scene support per query (its labelled cuboids as support mask), frozen backbone."""
    from geoformer_amd import scene
    from geoformer_amd.model import GeoFormerFS, load_config
    from geoformer_amd.model.criterion_fs import FSInstSetCriterion
    from tests.util import synthetic_state_dict

    cfg = load_config("geoformer_fs_scannet.yaml", batch_size=2, dec_dropout=0.0, n_decode_point=128, n_query_points=16)
    torch.manual_seed(0)
    m = GeoFormerFS(cfg)
    m.load_state_dict(synthetic_state_dict(m.state_dict(), 4))
    m.semantic_linear.bias.data[4:] += 1.0  # train fold == cv fold: foreground = classes >= 4
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    m.to(device)
    m.train()
    q = scene.make_batch([scene.make_small_scene(3000, 41), scene.make_small_scene(2600, 42)])
    sup = scene.make_batch([scene.make_small_scene(2400, 43), scene.make_small_scene(2800, 44)])
    for d in (q, sup):
        d["batch_offsets"] = d["offsets"]
    sup["support_masks"] = (sup["instance_labels"] >= 0).long()
    mv = lambda d: {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in d.items()}  # noqa: E731
    return cfg, m, FSInstSetCriterion(cfg), mv(sup), mv(q)


def _fs_step(m, crit, sup, q):
    np.random.seed(5)
    out = m(sup, q, training=True)
    loss, info = crit(out, q, 5)
    m.zero_grad()
    loss.backward()
    norms = {n: float(p.grad.norm()) for n, p in m.named_parameters() if p.grad is not None}
    return float(loss), info, norms


def test_fs_training_episode_cpu_oracle_backend(oracle):
    from oracle import cpu_backend

    with cpu_backend.installed():
        cfg, m, crit, sup, q = _fs_setup("cpu")
        loss, info, norms = _fs_step(m, crit, sup, q)
    assert np.isfinite(loss) and {"focal_loss", "dice_loss", "loss"} <= set(info)
    trainable = {n for n, p in m.named_parameters() if p.requires_grad}
    assert set(norms) <= trainable and sum(p.numel() for n, p in m.named_parameters() if p.requires_grad) == 42706
    assert any(n.startswith("similarity_net") or n.startswith("encoder_to_decoder") for n in norms)


@pytest.mark.gpu
def test_fs_training_episode_gpu_matches_oracle_backend(hip, oracle):
    """The few-shot training step through the HIP operators, the fused cross-attention / mask-head backward and the
    device criterion against the same step through the oracle's operators and the host criterion."""
    from oracle import cpu_backend

    with cpu_backend.installed():
        cfg, m, crit, sup, q = _fs_setup("cpu")
        loss_c, _, n_c = _fs_step(m, crit, sup, q)
    cfg, mg, critg, supg, qg = _fs_setup("cuda")
    loss_g, _, n_g = _fs_step(mg, critg, supg, qg)
    assert abs(loss_g - loss_c) < 1e-3 * max(1.0, abs(loss_c)), (loss_g, loss_c)
    assert set(n_g) == set(n_c)
    for k in n_c:
        assert abs(n_g[k] - n_c[k]) <= 3e-3 * max(n_c[k], 1e-3), (k, n_c[k], n_g[k])
