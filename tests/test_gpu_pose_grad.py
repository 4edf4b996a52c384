"""GPU: gradients with respect to the listener and source poses.

* Golden: the renderer behind the analytic stub network reproduces the
  reference autograd's pose gradients (tests/golden/pose_grad, written by
  tools/gen_pose_grad_golden.py) within TOL = 1e-4 relative L2 per pose, the
  spectrum parity budget; the CPU oracle's floor on the same fixtures is 0
  (tests/test_pose_grad_cpu.py).
* Chain rule on the real networks: the full render's pose gradients equal
  k * sum_n of the network-input gradients of the same render run from
  detached sample() outputs, to 2e-4 * sum_n |grad| (the worst case of
  reordering a 2048-term fp32 sum is n 2^-24 = 1.2e-4).
* Without pose gradients nothing changes; refusals for sharded rays, staged
  poses and graph replay."""
import numpy as np
import pytest
import torch

import hashgrid_dx_cases as hdc
from avr_amd import AVRRender
from avr_amd.graph import GraphedRender
from avr_amd.model import AVRModel, AVRModel_complex
from avr_amd.options import KernelOptions
from avr_amd.renderer import draw_jitter
from avr_amd.workloads import MESHRIR, RAF

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
TOL = 1e-4
SHAPE = dict(n_azi=6, n_ele=5, n_samples=64)  # config 1: R = 32, S = 64
T = 254


def _grid():
    return dict(otype="HashGrid", n_levels=8, n_features_per_level=2, log2_hashmap_size=12, base_resolution=4)


def _net(width, depth):
    return dict(otype="FullyFusedMLP", activation="ReLU", output_activation="None", n_neurons=width,
                n_hidden_layers=depth)


def _model(kind, options=None):
    if kind == "meshrir":
        cfg = dict(signal_output_dim=T, leaky_relu=0.03, pos_encoding_sigma=_grid(), dir_encoding_sig=_grid(),
                   tx_encoding_sig=_grid(), sigma_encoder_network=_net(128, 3), sigma_decoder_network=_net(128, 3),
                   signal_network=_net(512, 3))
        model = AVRModel(cfg, options=options)
    else:
        cfg = dict(signal_output_dim=T, leaky_relu=0.03, sigma_encoder_network=_net(128, 3),
                   sigma_decoder_network=_net(128, 1), signal_network=_net(512, 3),
                   **{k: _grid() for k in ("pos_encoding_sigma", "pos_encoding_sig", "dir_encoding_sig",
                                           "tx_pos_encoding_sigma", "tx_pos_encoding_sig", "tx_dir_encoding_sig")})
        model = AVRModel_complex(cfg, options=options)
    model = model.to(DEV)
    g = torch.Generator().manual_seed(41)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith("encoding.params"):
                p.copy_(((torch.rand(p.shape, generator=g) * 2 - 1) * 1e-1).to(DEV))
    return model


def _poses(kind, seed, B=2):
    g = torch.Generator().manual_seed(seed)
    ro = (torch.rand(B, 3, generator=g) * 2 - 1).to(DEV)
    tx = (torch.rand(B, 3, generator=g) * 2 - 1).to(DEV)
    dtx = None
    if kind == "raf":
        dtx = torch.nn.functional.normalize(torch.randn(B, 3, generator=g), dim=-1).to(DEV)
    probe = torch.randn(B, T // 2 + 1, 2, generator=g).to(DEV)
    return ro, tx, dtx, probe


def _render_cfg(kind):
    return dict(MESHRIR if kind == "meshrir" else RAF, **SHAPE)


# ------------------------------------------------------------------ golden
@pytest.mark.parametrize("name", hdc.GOLDEN_CASES)
def test_pose_gradients_match_reference_autograd(name):
    cfg, z = hdc.load_golden(name)
    names = ["rays_o", "position_tx"] + (["direction_tx"] if "direction_tx" in z.files else [])
    poses = [torch.from_numpy(z[n]).to(DEV).requires_grad_(True) for n in names]
    r = AVRRender(hdc.stub_of(z).to(DEV), **cfg)
    out = r(*poses, u_azi=torch.from_numpy(z["u_azi"]))
    (out * torch.from_numpy(z["G"]).to(DEV)).sum().backward()
    o = out.detach().cpu().numpy()
    err_out = float(np.linalg.norm(o - z["out"]) / np.linalg.norm(z["out"]))
    print(f"pose grad {name}: out rel l2 {err_out:.3e}")
    assert err_out < TOL
    for n, p in zip(names, poses):
        ref = z["grad_" + n]
        got = p.grad.cpu().numpy()
        err = np.linalg.norm(got - ref, axis=-1) / np.linalg.norm(ref, axis=-1)
        print(f"pose grad {name}: grad_{n} rel l2 per pose {err}")
        assert np.isfinite(got).all() and np.all(err < TOL), (n, err)


# -------------------------------------------------------------- chain rule
def _render_from_inputs(r, pts, view, tx, dtx, geom):
    """AVRRender._render after sample(), on the given network inputs."""
    net = r.network_fn
    kw = dict(ray_layout=(geom["B"], geom["n_rays"], int(r.n_samples)))
    net_in = (pts, view, tx) if dtx is None else (pts, view, tx, dtx)
    if r.fused_head:
        attn, h, weight, dtype = net.forward_fused(*net_in, **kw)
        if r._head_supported(geom, h, weight, dtype):
            link = getattr(net, "_relu_link", None) if r.head_relu_link else None
            net.__dict__.pop("_relu_link", None)
            return r.render_from_hidden(attn, h, weight, dtype, geom, link)
        return r.render_from_network_output(attn, net.finish_signal(h), geom)
    attn, signal = net(*net_in, **kw)
    return r.render_from_network_output(attn, signal, geom)


@pytest.mark.parametrize("fused_head", [True, False], ids=["head", "plain"])
@pytest.mark.parametrize("kind", ["meshrir", "raf"])
def test_pose_gradient_is_the_chain_rule_of_the_network_inputs(kind, fused_head):
    model = _model(kind)
    cfg = _render_cfg(kind)
    r = AVRRender(model, fused_head=fused_head, **cfg)
    ro, tx, dtx, probe = _poses(kind, 42)
    u = draw_jitter(cfg["n_azi"], cfg["n_ele"])
    k = 2.0 / (cfg["xyz_max"] - cfg["xyz_min"])
    # path A: the full render with poses that require grad
    pa = [None if t is None else t.clone().requires_grad_(True) for t in (ro, tx, dtx)]
    out_a = r(pa[0], pa[1], pa[2], u_azi=u)
    (out_a * probe).sum().backward()
    # path B: the same render from detached network inputs
    pts, view, txs, dts, geom = r.sample(ro, tx, dtx, u_azi=u)
    assert pts.grad_fn is None and not pts.requires_grad
    leaves = [None if t is None else t.clone().requires_grad_(True) for t in (pts, txs, dts)]
    out_b = _render_from_inputs(r, leaves[0], view, leaves[1], leaves[2], geom)
    assert torch.equal(out_a.detach(), out_b.detach())
    (out_b * probe).sum().backward()
    for name, p, leaf, scale in zip(("rays_o", "position_tx", "direction_tx"), pa, leaves, (k, k, 1.0)):
        if p is None:
            continue
        g = leaf.grad.double()
        want = scale * g.sum(dim=1)
        bound = 2e-4 * scale * g.abs().sum(dim=1)
        err = (p.grad.double() - want).abs()
        print(f"chain rule {kind} head={fused_head} {name}: max err/bound {float((err / bound).max()):.3e}")
        assert p.grad.dtype == torch.float32 and torch.isfinite(p.grad).all()
        assert bool((p.grad.abs().amax(dim=1) > 0).all())
        assert bool((err <= bound).all()), name


# ------------------------------------------------ unchanged without pose grads
def _step(r, poses, u, probe):
    for p in r.parameters():
        p.grad = None
    out = r(*[t for t in poses if t is not None], u_azi=u)
    (out * probe).sum().backward()
    grads = {n: p.grad.clone() for n, p in r.named_parameters() if p.grad is not None}
    assert any("encoding" in n for n in grads)
    return out.detach(), grads


def test_plain_poses_take_the_unchanged_path():
    kind = "meshrir"
    model = _model(kind, options=KernelOptions(hashgrid_bwd="partitioned"))
    cfg = _render_cfg(kind)
    r = AVRRender(model, **cfg)
    ro, tx, dtx, probe = _poses(kind, 43)
    u = draw_jitter(cfg["n_azi"], cfg["n_ele"])
    s = r.sample(ro, tx, u_azi=u)
    assert all(t.grad_fn is None and not t.requires_grad for t in s[:3])
    out1, g1 = _step(r, (ro, tx), u, probe)
    out2, g2 = _step(r, (ro, tx), u, probe)
    assert torch.equal(out1, out2)
    repeatable = all(torch.equal(g1[n], g2[n]) for n in g1)
    print(f"plain path parameter gradients bitwise repeatable: {repeatable}")
    out3, g3 = _step(r, (ro.clone().requires_grad_(True), tx.clone().requires_grad_(True)), u, probe)
    assert torch.equal(out1, out3)
    # sample() itself: the same values with and without the autograd node
    sg = r.sample(ro.clone().requires_grad_(True), tx, u_azi=u)
    assert sg[0].requires_grad and not sg[1].requires_grad and not sg[2].requires_grad
    assert all(torch.equal(a, b) for a, b in zip(s[:3], sg[:3]))
    for n in g1:
        if repeatable:
            assert torch.equal(g1[n], g3[n]), n
        else:  # the parent's own run-to-run tolerance (fp32 atomics of the small grids)
            scale = float(g1[n].abs().max())
            assert float((g1[n] - g3[n]).abs().max()) <= 1e-5 * scale, n


# ----------------------------------------------------------------- refusals
def test_unsupported_pose_gradient_paths_are_refused():
    kind = "meshrir"
    cfg = _render_cfg(kind)
    r = AVRRender(_model(kind), **cfg)
    ro, tx, _, _ = _poses(kind, 44)
    rg = ro.clone().requires_grad_(True)
    r.ray_range = (0, 16)
    with pytest.raises(NotImplementedError, match="sharded"):
        r(rg, tx)
    with torch.no_grad():
        assert r.sample(rg, tx)[0].shape == (2, 16 * 64, 3)  # (no gradient recorded: sampled as before)
    r.ray_range = None
    r._staged = (0, torch.zeros(18, device=DEV))
    try:
        with pytest.raises(NotImplementedError, match="staged"):
            r.sample(ro, tx.clone().requires_grad_(True))
    finally:
        r._staged = None
    with pytest.raises(NotImplementedError, match="GraphedRender"):
        GraphedRender(r).render_ir(rg, tx)
