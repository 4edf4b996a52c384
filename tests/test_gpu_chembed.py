"""GPU: channel embeddings (csrc/chembed.hip, avr_amd/chembed.py, AVRModel's
`ch_idx`): the per-pose bias + ReLU kernels against the torch composition,
their backward against threshold_backward and a float64 sum, out-of-range
indices, 64-bit offsets, graph capture, and the model with the kernels on
against the torch-op path, through AVRRender and through one TrainStep."""
import pytest
import torch

import chembed_cases as cc
from avr_amd import AVRRender, KernelOptions
from avr_amd import options as avr_options
from avr_amd.chembed import bias_relu_bwd, bias_relu_fwd
from avr_amd.model import AVRModel, _unit
from avr_amd.training import TrainStep
from avr_amd.workloads import RAF, WORKLOADS

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NAN, INF = float("nan"), float("inf")

DTYPES = [torch.float16, torch.bfloat16, torch.float32]
WIDTHS = [8, 128, 520]
# rows_per_group 130: no row tile of the kernels divides it, so tiles straddle
# groups; 4100: more rows than one backward chunk (and 4 rows over a multiple)
GROUPS = [(3, 130, [2, 0, 2]), (2, 4100, [2, 0])]
C = 4


def _case(dtype, W, G, rpg, idx, seed=0):
    """y with NaN, +-inf and elements where y + e is exactly 0 or changes sign
    within one rounding step of the dtype; table fp32; gy."""
    g = torch.Generator(device=DEV).manual_seed(seed + W + rpg)
    N = G * rpg
    table = torch.randn(C, W, device=DEV, generator=g) / W ** 0.5
    idx = torch.tensor(idx, device=DEV)
    e = table[idx].repeat_interleave(rpg, 0)
    y = torch.randn(N, W, device=DEV, generator=g)
    flat, ef = y.view(-1), e.reshape(-1)
    near = torch.arange(0, N * W, 7, device=DEV)
    eps = torch.finfo(dtype).eps
    flat[near] = -ef[near] * (1 + eps * torch.randint(-2, 3, near.shape, device=DEV, generator=g))
    flat[3::1013] = NAN
    flat[5::1019] = INF
    flat[11::1021] = -INF
    y = y.to(dtype)
    gy = torch.randn(N, W, device=DEV, generator=g).to(dtype)
    return y, table, idx, gy


def _composition(y, table, idx, rpg):
    """gather, add (fp32 by promotion), relu, cast."""
    return torch.relu(y + table[idx].repeat_interleave(rpg, 0)).to(y.dtype)


def _same_values(a, b):
    """Equal by value with NaN at the same positions."""
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=0.0),
                                                                     torch.nan_to_num(b, nan=0.0))


@pytest.mark.parametrize("G,rpg,idx", GROUPS, ids=["3x130", "2x4100"])
@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16", "f32"])
def test_forward_equals_composition(dtype, W, G, rpg, idx):
    y, table, idx, _ = _case(dtype, W, G, rpg, idx)
    out = bias_relu_fwd(y, table, idx, rpg)
    ref = _composition(y, table, idx, rpg)
    assert out.dtype == dtype and torch.isnan(ref).any() and torch.isinf(ref).any() and (ref == 0).any()
    assert _same_values(out, ref)


@pytest.mark.parametrize("G,rpg,idx", GROUPS, ids=["3x130", "2x4100"])
@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16", "f32"])
def test_backward(dtype, W, G, rpg, idx):
    y, table, idx, gy = _case(dtype, W, G, rpg, idx, seed=1)
    out = _composition(y, table, idx, rpg)
    g_table = torch.full((C, W), NAN, device=DEV)
    g, gt = bias_relu_bwd(gy, out, idx, rpg, C, g_table=g_table)
    assert gt is g_table and g.dtype == dtype
    ref = torch.ops.aten.threshold_backward(gy, out, 0)
    assert torch.equal(g, ref)
    # float64 sums; worst-case fp32 summation error of n terms: n * 2^-24 * sum |g|
    g64 = ref.double().view(G, rpg, W)
    want = torch.zeros(C, W, dtype=torch.float64, device=DEV).index_add_(0, idx, g64.sum(1))
    mass = torch.zeros(C, W, dtype=torch.float64, device=DEV).index_add_(0, idx, g64.abs().sum(1))
    n = torch.zeros(C, dtype=torch.float64, device=DEV).index_add_(
        0, idx, torch.full((G,), float(rpg), dtype=torch.float64, device=DEV))
    bound = n[:, None] * 2.0 ** -24 * mass
    err = (g_table.double() - want).abs()
    print(f"g_table max err / bound: {float((err / bound.clamp_min(1e-300)).max()):.3e}")
    assert torch.isfinite(g_table).all() and bool((err <= bound).all())
    assert not g_table[1].any() and not g_table[3].any()  # channels no group names: exact zeros
    g2, gt2 = bias_relu_bwd(gy, out, idx, rpg, C)
    assert torch.equal(g2, g) and torch.equal(gt2.view(torch.int32), g_table.view(torch.int32))


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_out_of_range_indices(dtype):
    W, rpg = 128, 130
    y, table, _, gy = _case(dtype, W, 3, rpg, [0, 0, 0], seed=2)
    y = torch.nan_to_num(y, nan=0.5, posinf=1.0, neginf=-1.0)
    bad = torch.tensor([C, 0, -1], device=DEV)
    out = bias_relu_fwd(y, table, bad, rpg)
    assert torch.isnan(out[:rpg]).all() and torch.isnan(out[2 * rpg:]).all()
    mid = _composition(y[rpg:2 * rpg], table, torch.tensor([0], device=DEV), rpg)
    assert torch.equal(out[rpg:2 * rpg], mid)
    g, gt = bias_relu_bwd(gy, out, bad, rpg, C, g_table=torch.full((C, W), NAN, device=DEV))
    assert torch.equal(g, torch.ops.aten.threshold_backward(gy, out, 0))
    _, alone = bias_relu_bwd(gy[rpg:2 * rpg].contiguous(), mid, torch.tensor([0], device=DEV), rpg, C)
    assert torch.equal(gt.view(torch.int32), alone.view(torch.int32))  # the bad groups add nothing
    assert gt[0].any() and not gt[1:].any()


def test_offsets_beyond_2_31_bytes():
    """N * W * 2 bytes just over 2^31: the last rows and one g_table column
    (the only large-memory test: y, out, g of 2.1 GB each)."""
    G, W = 8, 512
    N = 2_097_160
    rpg = N // G
    assert N * W * 2 > 2 ** 31 and N % G == 0
    g = torch.Generator(device=DEV).manual_seed(5)
    table = torch.randn(C, W, device=DEV, generator=g) / W ** 0.5
    idx = torch.tensor([1, 3, 0, 2, 1, 1, 0, 3], device=DEV)
    y = torch.empty(N, W, dtype=torch.float16, device=DEV).normal_(generator=g)
    out = bias_relu_fwd(y, table, idx, rpg)
    tail = _composition(y[-64:], table, idx[-1:], 64)
    assert torch.equal(out[-64:], tail) and tail.any()
    head = _composition(y[:64], table, idx[:1], 64)
    assert torch.equal(out[:64], head)
    g_, gt = bias_relu_bwd(y, out, idx, rpg, C)  # gy = y
    assert torch.equal(g_[-64:], torch.ops.aten.threshold_backward(y[-64:], tail, 0))
    col = 509
    c64 = g_[:, col].double().view(G, rpg)
    want = torch.zeros(C, dtype=torch.float64, device=DEV).index_add_(0, idx, c64.sum(1))
    mass = torch.zeros(C, dtype=torch.float64, device=DEV).index_add_(0, idx, c64.abs().sum(1))
    n = torch.zeros(C, dtype=torch.float64, device=DEV).index_add_(
        0, idx, torch.full((G,), float(rpg), dtype=torch.float64, device=DEV))
    err = (gt[:, col].double() - want).abs()
    assert bool((err <= n * 2.0 ** -24 * mass).all()), (err, n * 2.0 ** -24 * mass)


def test_forward_captures_into_a_graph():
    W, G, rpg = 128, 3, 130
    y, table, idx, _ = _case(torch.bfloat16, W, G, rpg, [2, 0, 2], seed=3)
    out = torch.empty_like(y)
    bias_relu_fwd(y, table, idx, rpg, out=out)  # library loaded, nothing lazy left
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            bias_relu_fwd(y, table, idx, rpg, out=out)
    torch.cuda.current_stream().wait_stream(s)
    first = out.clone()
    idx.copy_(torch.tensor([1, 3, 0], device=DEV))
    graph.replay()
    torch.cuda.synchronize()
    eager = bias_relu_fwd(y, table, idx, rpg)
    assert _same_values(out, eager) and not _same_values(out, first)


def test_backward_takes_a_gradient_at_an_odd_offset():
    """A contiguous upstream gradient that is not 16-byte aligned (a view 8
    bytes into a buffer) is copied, not refused: same results as the torch ops."""
    from avr_amd.chembed import bias_relu_torch, group_bias_relu

    W, G, rpg = 128, 3, 130
    y, table, idx, gy = _case(torch.float16, W, G, rpg, [2, 0, 2], seed=4)
    y = torch.nan_to_num(y, nan=0.5, posinf=1.0, neginf=-1.0)
    buf = torch.empty(gy.numel() + 4, dtype=gy.dtype, device=DEV)
    odd = buf[4:].view_as(gy).copy_(gy)
    assert odd.is_contiguous() and odd.data_ptr() % 16 == 8
    grads = []
    for fn in (group_bias_relu, bias_relu_torch):
        yr, tr = y.clone().requires_grad_(True), table.clone().requires_grad_(True)
        fn(yr, tr, idx, rpg).backward(odd)
        grads.append((yr.grad, tr.grad))
    assert torch.equal(grads[0][0], grads[1][0])
    assert _rel(grads[0][1], grads[1][1]) < 2e-4 and grads[0][1].dtype == torch.float32


# ---------------------------------------------------------------- model
W1 = WORKLOADS["c1_meshrir_plumbing"]  # 32 rays x 64 samples
MODES = {"add_das": cc.ADD_DAS, "add_all": cc.ADD_ALL, "concat_all": cc.CONCAT_ALL}


def _model_inputs(model, B=2):
    r = AVRRender(model, **W1.render)
    g = torch.Generator(device=DEV).manual_seed(3)
    ro = torch.rand(B, 3, device=DEV, generator=g) * 2 - 1
    tx = torch.rand(B, 3, device=DEV, generator=g) * 2 - 1
    torch.manual_seed(0)
    pts, view, txs, _, _ = r.sample(ro, tx, None)
    return pts, view, txs, (B, W1.n_rays, W1.n_samples)


def _run(model, args, ch, layout, chembed):
    avr_options.apply(model, KernelOptions(chembed=chembed))
    model.zero_grad(set_to_none=True)
    attn, sig = model(*args, ch_idx=ch, ray_layout=layout)
    (attn.float().sum() + (sig.float() * 1e-2).sum()).backward()
    grads = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    return attn.detach(), sig.detach(), grads


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_model_kernel_path_equals_torch_path(dtype, mode):
    """chembed=True against chembed=False, and ray_layout=None against the
    layout path.  Outputs and every MLP weight gradient are bitwise equal
    (same rounded values, same selection).  The embedding gradients are fp32
    sums in another order: 2e-4 norm-relative, the bar of
    test_ray_layout_grouped_encoding_matches_flat for such differences.  The
    hash grids' gradients cannot be compared bitwise: their backward
    (csrc/hashgrid.hip, "slot order within a chunk free") adds in fp32 in an
    order that changes from run to run, so two identical calls already differ
    in the last bits.  The gradient fed to a grid is bitwise equal wherever
    the grid is evaluated on the same rows, so those are held to the 1e-5
    that tests/test_gpu_model.py allows this run-to-run effect; only between
    the layouts are the per-ray / per-pose grids evaluated once per group,
    and they get the 2e-3 test_ray_layout_grouped_encoding_matches_flat
    allows AVRModel's fp16 grids (the group's summed gradient is rounded to
    fp16 once)."""
    torch.manual_seed(11)
    model = AVRModel(cc.small_model_cfg(MODES[mode]), mlp_dtype=dtype).to(DEV)
    pts, view, txs, layout = _model_inputs(model)
    ch = torch.tensor([5, 1], device=DEV)
    on = _run(model, (pts, view, txs), ch, layout, True)
    off = _run(model, (pts, view, txs), ch, layout, False)
    flat = _run(model, (pts, view, txs), ch, None, True)
    emb = set(cc.embedding_params(model))
    assert emb and emb <= on[2].keys() == off[2].keys() == flat[2].keys()
    assert torch.isfinite(on[1]).all() and on[1].any()
    for what, other, grouped in (("torch ops", off, 1e-5), ("flat", flat, 2e-3)):
        assert torch.equal(on[0], other[0]) and torch.equal(on[1], other[1])
        for n, g in on[2].items():
            if n in emb or n.endswith("_encoding.params"):
                assert g.dtype == torch.float32
                err = _rel(g, other[2][n])
                print(f"{mode} vs {what} {n}: {err:.3e}")
                bar = 2e-4 if n in emb else grouped if n in ("_dir_encoding.params", "_tx_encoding.params") else 1e-5
                assert err < bar, (what, n, err)
            else:
                assert torch.equal(g, other[2][n]), (what, n)
    # rows of channels no pose names get exact zeros; int32 indices are taken
    for n in emb:
        rows = [i for i in range(8) if i not in (5, 1)]
        assert not on[2][n][rows].any() and on[2][n][5].any() and on[2][n][1].any(), n
    with torch.no_grad():
        a32, s32 = model(pts, view, txs, ch_idx=ch.int(), ray_layout=layout)
        a64, s64 = model(pts, view, txs, ch_idx=ch, ray_layout=layout)
    assert torch.equal(a32, a64) and torch.equal(s32, s64)


@pytest.mark.parametrize("mode", list(MODES))
def test_model_fp32_matches_restatement(mode):
    """Elementwise: rtol 1e-4, and an absolute term for elements that are
    cancelling sums, which carry the rounding error of their terms and not of
    their own small value: a K-term fp32 dot product is off by at most
    K 2^-24 sum |x w| (K <= 512: 3e-5 of the term mass) per layer, over the
    three to four layers between an embedding and the output, so
    atol = 1e-4 max |reference|."""
    torch.manual_seed(12)
    model = AVRModel(cc.small_model_cfg(MODES[mode]), mlp_dtype=torch.float32).to(DEV)
    pts, view, txs, layout = _model_inputs(model)
    ch = torch.tensor([5, 1], device=DEV)
    n = pts.size(1)
    with torch.no_grad():
        attn, sig = model(pts, view, txs, ch_idx=ch, ray_layout=layout)
        enc = [e(_unit(x.reshape(-1, 3))).float() for e, x in (
            (model._pos_encoding, pts), (model._dir_encoding, view), (model._tx_encoding, txs))]
        ra, rs = cc.ref_model(model, *enc, ch, n, torch.float32)
    for name, got, ref in (("attn", attn.reshape(-1, 1), ra), ("signal", sig.reshape(rs.shape), rs)):
        atol = 1e-4 * float(ref.abs().max())
        worst = float(((got - ref).abs() / (atol + 1e-4 * ref.abs())).max())
        print(f"{mode} {name}: max |err| / (atol + rtol |ref|) = {worst:.3e}, norm-relative {_rel(got, ref):.3e}")
        torch.testing.assert_close(got, ref, rtol=1e-4, atol=atol)
    with torch.no_grad():  # another channel is another output
        _, other = model(pts, view, txs, ch_idx=torch.tensor([5, 2], device=DEV), ray_layout=layout)
    assert torch.equal(other[0], sig[0]) and not torch.equal(other[1], sig[1])


def _render_inputs(B=2):
    g = torch.Generator(device=DEV).manual_seed(9)
    return (torch.rand(B, 3, device=DEV, generator=g) * 2 - 1, torch.rand(B, 3, device=DEV, generator=g) * 2 - 1)


def test_render_with_fused_head_follows_the_channel():
    torch.manual_seed(13)
    model = AVRModel(cc.small_model_cfg(cc.ADD_DAS), mlp_dtype=torch.bfloat16).to(DEV)
    r = AVRRender(model, **W1.render).to(DEV)
    assert r.fused_head
    ro, tx = _render_inputs()
    outs = []
    for ch in ([0, 0], [0, 3]):
        torch.manual_seed(1)  # the same ray jitter
        with torch.no_grad():
            outs.append(r(ro, tx, ch_idx=torch.tensor(ch, device=DEV)))
    assert torch.isfinite(outs[0]).all() and outs[0].any()
    assert torch.equal(outs[0][0], outs[1][0]) and not torch.equal(outs[0][1], outs[1][1])


def test_model_without_a_mode_ignores_ch_idx():
    torch.manual_seed(14)
    model = AVRModel(cc.small_model_cfg(cc.NO_MODE), mlp_dtype=torch.bfloat16).to(DEV)
    r = AVRRender(model, **W1.render).to(DEV)
    ro, tx = _render_inputs()
    outs = []
    for kw in ({}, {"ch_idx": torch.tensor([5, 1], device=DEV)}):
        torch.manual_seed(1)
        with torch.no_grad():
            outs.append(r(ro, tx, **kw))
    assert torch.equal(outs[0], outs[1])


TRAIN = dict(lr=2e-4, weight_decay=0, T_max=300000, eta_min=8e-5, spec_loss_weight=1, amplitude_loss_weight=1,
             angle_loss_weight=1, time_loss_weight=20, energy_loss_weight=3, multistft_loss_weight=2)


def _train_setup(seed):
    torch.manual_seed(seed)
    cfg = dict(cc.small_model_cfg(cc.ADD_DAS), signal_output_dim=800)
    model = AVRModel(cfg, mlp_dtype=torch.bfloat16).to(DEV)
    r = AVRRender(model, **dict(RAF, n_azi=8, n_ele=4, n_samples=16)).to(DEV)
    return r, TrainStep(r, TRAIN, dict(fs=16000, speed=346.8))


def test_train_step_and_checkpoints(tmp_path):
    r, step = _train_setup(0)
    g = torch.Generator(device=DEV).manual_seed(7)
    rx = torch.rand(2, 3, device=DEV, generator=g) * 2 - 1
    tx = torch.rand(2, 3, device=DEV, generator=g) * 2 - 1
    t = torch.arange(800, device=DEV)
    ori = torch.fft.rfft(torch.randn(2, 800, device=DEV, generator=g) * torch.exp(-t / 120.0) * 0.05)
    emb = {n: p.detach().clone() for n, p in r.named_parameters() if "embedding" in n}
    assert len(emb) == 6
    torch.manual_seed(1)
    total, losses = step(ori, rx, tx, ch_idx=torch.tensor([5, 1]))
    assert torch.isfinite(total) and all(torch.isfinite(x) for x in losses)
    rest = [i for i in range(8) if i not in (5, 1)]
    for n, p in r.named_parameters():
        if n in emb:
            assert not torch.equal(p[5], emb[n][5]) and not torch.equal(p[1], emb[n][1]), n
            assert torch.equal(p[rest], emb[n][rest]), n
    want = {k: v.detach().clone() for k, v in r.state_dict().items()}
    for ref_layout in (False, True):
        path = step.save_checkpoint(str(tmp_path / f"ck{int(ref_layout)}.tar"), reference_layout=ref_layout)
        sd = torch.load(path, weights_only=True)["audionerf_network_state_dict"]
        if ref_layout:
            assert "network_fn._model_signal.hidden_layers.0.params" in sd
            assert "network_fn._model_signal.layer_embeddings.2" in sd and not any(k.endswith(".weight") for k in sd)
        r2, step2 = _train_setup(100 + int(ref_layout))
        step2.load_checkpoint(path)
        assert step2.current_iteration == 1
        got = r2.state_dict()
        assert got.keys() == want.keys()
        for k in want:
            assert torch.equal(got[k], want[k]), k
        assert len(step2.optimizer.state) == len(step.optimizer.state)
