"""GPU: directional receivers.  The multi-channel ray reduction and its
backward against the float64 references of tests/spatial_cases.py and, bit for
bit, against the single-channel kernel; the `ray_gain` keyword end to end
against the reference's gain-scaled renders (tests/golden/spatial); and the
guarantee that a render without a gain is untouched.

Bounds (u = 2^-24, derived, not measured):
* forward: a chain of n_r fused multiply-adds over the rays of a split on the
  weights fl(w*g), one rounding more than the single-channel kernel's w:
  |err| <= 2 (n_r + 2) u sum |g w x|.
* backward, grad_w: q = sum_c g_c gz_c costs C roundings, the dot with x over
  the n_live samples of a row is the existing kernel's tree (its n_live + 8),
  later channel blocks add their share: |err| <= 2 (n_live + 8 + C) u sum_c |g_c| sum_t |gz_c x|.
* backward, grad_signal: C roundings in q, one in w*q, one add per later
  block, and one store rounding (2^-11 fp16, 2^-8 bf16, relative) per block,
  each on a partial sum that sum_c |w g_c gz_c| bounds; 2^-25 covers an fp16
  subnormal result."""
import ctypes

import numpy as np
import pytest
import torch

import render_stage_cases as rsc
import spatial_cases as sc
from golden_util import digest_check, rel_l2
from test_gpu_render_stages import CODE, DEV, U, _nan, _reduce_operands, _st, ctx

from avr_amd import AVRRender, _lib, spatial
from avr_amd.graph import GraphedRender
from avr_amd.model import AVRModel
from avr_amd.parallel import RayShardedRender
from avr_amd.renderer import _render_core_mc_fwd, get_tables, reduce_mc_splits, render_params
from avr_amd.workloads import MESHRIR_MODEL, WORKLOADS, _grid, make_inputs

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _ids(lst):
    return [c.id for c in lst]


def _blocks(C):
    n = 0
    while C > 0:
        C -= 4 if C >= 4 else 2 if C >= 2 else 1
        n += 1
    return n


def _mc_fwd(o, case, C, gain_dev, n_split, part):
    stride = 0 if gain_dev.dim() == 2 else C * case.R
    _lib.call("avr_ray_reduce_mc_fwd", ctypes.byref(o["p"]), case.B, C, o["x"].data_ptr(), CODE[case.dtype],
              o["w_dev"].data_ptr(), o["d_dev"].data_ptr(), gain_dev.data_ptr(), stride, n_split, part.data_ptr(), _st())


# ------------------------------------------------------------ stage, forward
@pytest.mark.parametrize("C", sc.CHANNELS)
@pytest.mark.parametrize("case", sc.MC_FWD, ids=_ids(sc.MC_FWD))
def test_ray_reduce_mc_fwd(case, C):
    o = _reduce_operands(case)
    B, R, S, T = case.B, case.R, case.S, case.T
    assert case.vector == (case.offset == 0 and S * T % case.vec == 0)
    for per_pose in (False, True):
        gain = sc.synth_gain(case, C, per_pose)
        assert (gain == 0).any() and np.abs(gain).max() <= 1
        g_dev = torch.from_numpy(gain).to(DEV)
        for n_split in case.n_splits:
            part = _nan(n_split, B, C, S, T)
            _mc_fwd(o, case, C, g_dev, n_split, part)
            torch.cuda.synchronize()
            got = part.cpu().numpy()
            assert not np.isnan(got).any(), "elements the stage owns were not written"
            ref, mag, n_r = sc.ref_reduce_mc_fwd(o["x64"], o["w"], o["delay"], o["host"]["shift"], gain, n_split)
            bound = 2.0 * (n_r[:, None, None, None, None] + 2) * U * mag
            err = np.abs(got.astype(np.float64) - ref)
            print(f"mc_fwd {case.id} C={C} per_pose={per_pose} n_split={n_split}: "
                  f"{float((err / np.maximum(bound, 1e-300)).max()):.2f} of bound")
            assert np.all(got[mag == 0] == 0)
            assert np.all(err <= bound)
            if (R + n_split - 1) // n_split * (n_split - 1) >= R:
                assert np.all(got[-1] == 0)  # the empty last split
            # channel c is the single-channel kernel on w*g[c], bit for bit
            g3 = g_dev if per_pose else g_dev.unsqueeze(0).expand(B, C, R)
            for c in range(C):
                wg = (o["w_dev"] * g3[:, c, :, None]).contiguous()
                one = _nan(n_split, B, S, T)
                _lib.call("avr_ray_reduce_fwd", ctypes.byref(o["p"]), B, o["x"].data_ptr(), CODE[case.dtype],
                          wg.data_ptr(), o["d_dev"].data_ptr(), n_split, one.data_ptr(), _st())
                assert torch.equal(part[:, :, c], one), (c, n_split)


# ----------------------------------------------------------- stage, backward
@pytest.mark.parametrize("C", sc.CHANNELS)
@pytest.mark.parametrize("case", sc.MC_BWD, ids=_ids(sc.MC_BWD))
def test_ray_reduce_mc_bwd(case, C):
    """C = 9 runs as blocks of 4 + 4 + 1: the later ones add into both outputs."""
    o = _reduce_operands(case)
    B, R, S = case.B, case.R, case.S
    tdt = rsc.TORCH_DTYPE[case.dtype]
    n = o["x"].numel()
    gz = sc.synth_gz(case, C)
    gz_dev = torch.from_numpy(gz).to(DEV)
    for per_pose in (False, True):
        gain = sc.synth_gain(case, C, per_pose)
        g_dev = torch.from_numpy(gain).to(DEV)
        gbuf = _nan(n + 8, dtype=tdt)
        gx = gbuf[case.offset:case.offset + n].view(o["x"].shape)
        gw = _nan(B, R, S)
        _lib.call("avr_ray_reduce_mc_bwd", ctypes.byref(o["p"]), B, C, o["x"].data_ptr(), CODE[case.dtype],
                  gz_dev.data_ptr(), o["w_dev"].data_ptr(), o["d_dev"].data_ptr(), g_dev.data_ptr(),
                  C * R if per_pose else 0, gx.data_ptr(), gw.data_ptr(), _st())
        torch.cuda.synchronize()
        assert not torch.isnan(gx).any() and not torch.isnan(gw).any()
        assert torch.isnan(gbuf[:case.offset]).all() and torch.isnan(gbuf[case.offset + n:]).all()  # nothing outside
        ref_gx, ref_gw, mag_x, mag_w, n_live = sc.ref_reduce_mc_bwd(o["x64"], gz, o["w"], o["delay"],
                                                                    o["host"]["shift"], gain)
        err_w = np.abs(gw.cpu().numpy().astype(np.float64) - ref_gw)
        bound_w = 2.0 * (n_live + 8 + C) * U * mag_w
        nb = _blocks(C)
        err_x = np.abs(gx.cpu().double().numpy() - ref_gx)
        bound_x = ((C + 1 + nb) * U + nb * sc.STORE_U[case.dtype]) * mag_x + (2.0 ** -25 if case.dtype == "float16" else 0)
        print(f"mc_bwd {case.id} C={C} per_pose={per_pose}: grad_w "
              f"{float((err_w / np.maximum(bound_w, 1e-300)).max()):.2f} of bound, grad_x "
              f"{float((err_x / np.maximum(bound_x, 1e-300)).max()):.2f} of bound")
        assert np.all(err_w <= bound_w)
        assert np.all(err_x <= bound_x)
        assert np.all(gx.cpu().float().numpy()[mag_x == 0] == 0)


# -------------------------------------------------------------------- limits
def _limit_operands(R, S=2, T=62, B=1):
    cfg = rsc.render_cfg("meshrir", S, T, n_azi=R, n_ele=1)
    p, tb, host = ctx(cfg, T, R)
    rng = rsc.case_rng("limit", R)
    x = rng.standard_normal((B, R, S, T)).astype(np.float32)
    w = rng.uniform(-1, 1, (B, R, S)).astype(np.float32)
    delay = rng.integers(0, T // 2, (B, R, S)).astype(np.int32)
    gain = rng.uniform(-1, 1, (4, R)).astype(np.float32)
    return p, host, x, w, delay, gain


def test_largest_split_at_four_channels_and_one_ray_more():
    p0, *_ = _limit_operands(8)
    n, cap = reduce_mc_splits(p0, 1, 4, 0)
    assert cap == 65536 // 20 and reduce_mc_splits(p0, 1, 1, 0)[1] == 4096  # (4 + 4 CB) bytes per ray in 64 KiB
    p, host, x, w, delay, gain = _limit_operands(cap)
    B, R, S, T = x.shape
    dev = [torch.from_numpy(a).to(DEV) for a in (x, w, delay, gain)]
    part = _nan(1, B, 4, S, T)
    _lib.call("avr_ray_reduce_mc_fwd", ctypes.byref(p), B, 4, dev[0].data_ptr(), 0, dev[1].data_ptr(),
              dev[2].data_ptr(), dev[3].data_ptr(), 0, 1, part.data_ptr(), _st())
    torch.cuda.synchronize()
    ref, mag, n_r = sc.ref_reduce_mc_fwd(x, w, delay, host["shift"], gain, 1)
    assert float(np.abs(ref).max()) > 0
    assert np.all(np.abs(part.cpu().numpy() - ref) <= 2.0 * (n_r[0] + 2) * U * mag)
    # the chooser stays within the cap, and refuses what 16 splits cannot hold
    def params(R):
        return render_params(rsc.render_cfg("meshrir", 2, 62, n_azi=R, n_ele=1), 62, n_rays=R)

    assert reduce_mc_splits(params(16 * cap), 1, 4, 0)[0] == 16
    with pytest.raises(RuntimeError, match="too many rays"):
        reduce_mc_splits(params(16 * cap + 1), 1, 4, 0)
    # one ray more in a single split: refused before any launch
    p1, host, x, w, delay, gain = _limit_operands(cap + 1)
    dev = [torch.from_numpy(a).to(DEV) for a in (x, w, delay, gain)]
    part = _nan(1, B, 4, S, T)
    with pytest.raises(RuntimeError, match=r"status 1001.*too many rays per split"):
        _lib.call("avr_ray_reduce_mc_fwd", ctypes.byref(p1), B, 4, dev[0].data_ptr(), 0, dev[1].data_ptr(),
                  dev[2].data_ptr(), dev[3].data_ptr(), 0, 1, part.data_ptr(), _st())
    torch.cuda.synchronize()
    assert torch.isnan(part).all()


@pytest.mark.parametrize("C", [0, 17])
def test_channel_count_out_of_range_is_refused(C):
    case = sc.MC_BWD[-1]
    o = _reduce_operands(case)
    gain = torch.zeros(max(C, 1), case.R, device=DEV)
    part = _nan(1, case.B, max(C, 1), case.S, case.T)
    with pytest.raises(RuntimeError, match=r"status 1001.*C must be 1..16"):
        _mc_fwd(o, case, C, gain, 1, part)
    gx, gw = torch.empty_like(o["x"]), _nan(case.B, case.R, case.S)
    gz = torch.zeros(case.B, max(C, 1), case.S, case.T, device=DEV)
    with pytest.raises(RuntimeError, match=r"status 1001.*C must be 1..16"):
        _lib.call("avr_ray_reduce_mc_bwd", ctypes.byref(o["p"]), case.B, C, o["x"].data_ptr(), 0, gz.data_ptr(),
                  o["w_dev"].data_ptr(), o["d_dev"].data_ptr(), gain.data_ptr(), 0, gx.data_ptr(), gw.data_ptr(), _st())
    with pytest.raises(RuntimeError, match="C must be 1..16"):
        reduce_mc_splits(o["p"], case.B, C, 0)
    torch.cuda.synchronize()
    assert torch.isnan(part).all() and torch.isnan(gw).all()


# ---------------------------------------------------------------- end to end
class Net(torch.nn.Module):
    def __init__(self, attn, signal):
        super().__init__()
        self.attn, self.signal = attn, signal

    def forward(self, pts, view, tx, dir_tx=None):
        return self.attn, self.signal


def _setup(case, grads=False):
    w, inp = case.workload, case.inputs()
    attn = torch.from_numpy(inp["attn"]).to(DEV).requires_grad_(grads)
    sig = torch.from_numpy(inp["signal"]).to(DEV).requires_grad_(grads)
    dtx = None if inp["direction_tx"] is None else torch.from_numpy(inp["direction_tx"]).to(DEV)
    r = AVRRender(Net(attn, sig), **w.render)
    pose = (torch.from_numpy(inp["rays_o"]).to(DEV), torch.from_numpy(inp["position_tx"]).to(DEV), dtx)
    return r, pose, attn, sig, torch.from_numpy(case["gain"]).to(DEV)


@pytest.mark.parametrize("name", sc.render_case_names())
def test_render_matches_the_reference_golden(name):
    case = sc.SpatialCase(name)
    w = case.workload
    r, pose, attn, sig, gain = _setup(case)
    with torch.no_grad():
        torch.manual_seed(case.seed)
        out, ir = r.render_ir(*pose, ray_gain=gain)
        torch.manual_seed(case.seed)
        fwd = r(*pose, ray_gain=gain)
        torch.manual_seed(case.seed)
        *_, geom = r.sample(*pose)
        p = r._params(w.T, w.n_rays)
        _, _, delay = _render_core_mc_fwd(attn.view(w.batch, -1), sig, gain, p, get_tables(p, DEV), geom["rays_o"],
                                          geom["position_tx"], geom["dirs"])
    F = w.T // 2 + 1
    assert out.shape == (w.batch, case.C, F, 2) and ir.shape == (w.batch, case.C, 2 * (F - 1))
    assert torch.equal(out, fwd)
    o, i = out.cpu().numpy(), ir.cpu().numpy()
    for c in range(case.C):
        l2o, l2i = rel_l2(o[:, c], case["out"][:, c]), rel_l2(i[:, c], case["ir"][:, c])
        print(f"{name} channel {c}: spectrum {l2o:.2e} ir {l2i:.2e}")
        assert l2o < TOL and l2i < TOL
    # the integer delays do not depend on the gain: bit-exact, every entry
    np.testing.assert_array_equal(delay.cpu().numpy().astype(np.int16), case["delay"])


@pytest.mark.parametrize("name", sc.render_case_names())
def test_backward_matches_the_reference_golden(name):
    """The bars of tests/test_gpu_render.py::test_backward_matches_reference_golden."""
    case = sc.SpatialCase(name)
    r, pose, attn, sig, gain = _setup(case, grads=True)
    torch.manual_seed(case.seed)
    out, ir = r.render_ir(*pose, ray_gain=gain)
    assert ir.shape[:2] == out.shape[:2] and ir.requires_grad
    (out * torch.from_numpy(case.grad_probe()).to(DEV)).sum().backward()
    ga = attn.grad.float().cpu().numpy()
    gs = sig.grad.float().cpu().numpy()
    scale_a = np.sqrt(float((case["grad_attn"].astype(np.float64) ** 2).sum()) / ga.size)
    scale_s = np.sqrt(float(case["grad_signal_sumsq"]) / gs.size)
    tol_s = 2e-3 if case.workload.signal_dtype == "float16" else TOL  # fp16 gradient storage rounds at 2^-11
    digest_check(case, "grad_attn", ga, rtol=0, atol=TOL * 50 * scale_a + 1e-4 * np.abs(ga).max())
    digest_check(case, "grad_signal", gs, rtol=tol_s, atol=tol_s * scale_s)
    s64 = gs.astype(np.float64).sum()
    assert abs(s64 - float(case["grad_signal_sum"])) <= 1e-3 * np.sqrt(float(case["grad_signal_sumsq"]) * gs.size) + 1e-6
    dot = float((gs.astype(np.float64) * case.inputs()["signal"].astype(np.float64)).sum())
    ref_dot = float(case["grad_signal_dot_signal"])
    assert abs(dot - ref_dot) <= 1e-3 * abs(ref_dot) + 1e-6


def test_single_channel_gain_with_and_without_channel_axis():
    """[R] keeps [B,F,2]; [1,R] and [B,1,R] give [B,1,F,2]; all equal channel 1
    of the pair golden within the parity bar, and their gradients agree."""
    case = sc.SpatialCase("c1_pair")
    r, pose, attn, sig, gain = _setup(case, grads=True)
    g1 = gain[0, 1]  # pose 0's second capsule for every pose: [R]
    outs = []
    for g in (g1, g1[None], g1[None, None].expand(case.workload.batch, 1, -1)):
        torch.manual_seed(case.seed)
        outs.append(r(*pose, ray_gain=g))
    assert outs[0].dim() == 3 and outs[1].shape == outs[2].shape == (outs[0].size(0), 1) + outs[0].shape[1:]
    assert torch.equal(outs[0], outs[1][:, 0]) and torch.equal(outs[0], outs[2][:, 0])
    assert rel_l2(outs[0][0].detach().cpu().numpy(), case["out"][0, 1]) < TOL
    # against the multi-channel kernel's channel with the same gains
    torch.manual_seed(case.seed)
    pair = r(*pose, ray_gain=torch.stack([g1, g1 * 0.5]))
    assert rel_l2(pair[:, 0].detach().cpu().numpy(), outs[0].detach().cpu().numpy()) < 1e-5
    G = torch.from_numpy(case.grad_probe()[:, 0]).to(DEV)
    (outs[0] * G).sum().backward()
    ga1, gs1 = attn.grad.clone(), sig.grad.clone()
    attn.grad = sig.grad = None
    (pair[:, 0] * G).sum().backward()
    assert rel_l2(attn.grad.cpu().numpy(), ga1.cpu().numpy()) < 1e-5
    assert rel_l2(sig.grad.cpu().numpy(), gs1.cpu().numpy()) < 1e-5


def test_callable_gain_sees_the_renders_directions():
    case = sc.SpatialCase("c1_foa")
    r, pose, *_ = _setup(case)
    seen = {}

    def fn(dirs):
        seen["dirs"], seen["gain"] = dirs, spatial.foa(dirs)
        return seen["gain"]

    with torch.no_grad():
        torch.manual_seed(7)
        a = r(*pose, ray_gain=fn)
        torch.manual_seed(7)
        b = r(*pose, ray_gain=seen["gain"])
        torch.manual_seed(7)
        *_, geom = r.sample(*pose)
        torch.manual_seed(8)
        c = r(*pose, ray_gain=seen["gain"])
    assert seen["dirs"].is_cuda and torch.equal(seen["dirs"], geom["dirs"])
    assert a.shape[1] == 4 and torch.equal(a, b)
    assert not torch.equal(a, c)  # another jitter draw: other directions
    with torch.no_grad():
        torch.manual_seed(7)
        st = r(*pose, ray_gain=spatial.cardioid_pair(90, 110))
    assert st.shape == (a.size(0), 2) + a.shape[2:] and torch.isfinite(st).all()


# ----------------------------------------------------------------- invariance
def test_no_gain_is_the_existing_path_and_ones_change_nothing():
    case = sc.SpatialCase("c1_foa")
    r, pose, attn, sig, _ = _setup(case)
    R = case.workload.n_rays
    with torch.no_grad():
        torch.manual_seed(3)
        *_, geom = r.sample(*pose)
        want = r.render_from_network_output(attn, sig, geom)
        torch.manual_seed(3)
        none = r(*pose, ray_gain=None)
        torch.manual_seed(3)
        plain, ir = r.render_ir(*pose)
        torch.manual_seed(3)
        ones, ir1 = r.render_ir(*pose, ray_gain=torch.ones(R))
        torch.manual_seed(3)
        again = r(*pose, ray_gain=torch.ones(R, device=DEV))
        torch.manual_seed(3)
        foa1 = r(*pose, ray_gain=spatial.foa)
        torch.manual_seed(3)
        foa2 = r(*pose, ray_gain=spatial.foa)
    assert want.shape == (case.workload.batch, case.workload.F, 2)
    assert torch.equal(none, want) and torch.equal(plain, want)
    assert torch.equal(ones, want) and torch.equal(again, want) and torch.equal(ir1, ir)
    assert torch.equal(foa1, foa2)  # two runs repeat
    # W has unit gains: the omnidirectional render, up to the DFT's slicing at batch B*C
    assert rel_l2(foa1[:, 0].cpu().numpy(), want.cpu().numpy()) < 1e-5


@pytest.mark.parametrize("exact", [False, True], ids=["fused", "exact"])
def test_ones_gain_through_the_fused_heads(exact):
    w = WORKLOADS["c1_meshrir_plumbing"]
    small = {k: _grid(12) for k in ("pos_encoding_sigma", "dir_encoding_sig", "tx_encoding_sig")}
    torch.manual_seed(0)
    # T = 1022: long enough that the delays of these poses fall inside the signal
    model = AVRModel(dict(MESHRIR_MODEL, signal_output_dim=1022, **small), mlp_dtype=torch.float16).to(DEV)
    with torch.no_grad():
        for enc in (model._pos_encoding, model._dir_encoding, model._tx_encoding):
            enc.params.uniform_(-1, 1)
    r = AVRRender(model, exact_head=exact, **w.render)
    inp = make_inputs(w.replace(batch=2), 1)
    ro, tx = torch.from_numpy(inp["rays_o"]).to(DEV), torch.from_numpy(inp["position_tx"]).to(DEV)
    calls = []
    real = r.render_from_hidden
    r.render_from_hidden = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    with torch.no_grad():
        torch.manual_seed(2)
        plain = r(ro, tx)
        torch.manual_seed(2)
        ones = r(ro, tx, ray_gain=torch.ones(w.n_rays))
        torch.manual_seed(2)
        half = r(ro, tx, ray_gain=torch.full((1, w.n_rays), 0.5))
        torch.manual_seed(2)
        two = r(ro, tx, ray_gain=torch.ones(2, w.n_rays))
    assert len(calls) == 3  # one channel stays on the head kernels, two leave them
    assert float(plain.abs().max()) > 0
    assert torch.equal(ones, plain)
    assert half.shape == (2, 1) + plain.shape[1:] and rel_l2(half[:, 0].cpu().numpy(), 0.5 * plain.cpu().numpy()) < 1e-5
    assert two.shape == (2, 2) + plain.shape[1:] and torch.equal(two[:, 0], two[:, 1])
    assert rel_l2(two[:, 0].cpu().numpy(), plain.cpu().numpy()) < 2e-3  # the head's summation differs


def test_propagate_nonfinite_poisons_every_channel():
    case = sc.SpatialCase("c1_foa")
    r, pose, attn, sig, gain = _setup(case)
    bad = sig.clone()
    bad[1, 0, 0] = float("nan")  # one element of pose 1: the whole batch is poisoned, as without a gain
    strict = AVRRender(Net(attn, bad), propagate_nonfinite=True, **case.workload.render)
    with torch.no_grad():
        torch.manual_seed(case.seed)
        out, ir = strict.render_ir(*pose, ray_gain=gain)
        torch.manual_seed(case.seed)
        plain = strict.render_ir(*pose)[0]
    assert out.shape[1] == 4 and torch.isnan(out).all() and torch.isnan(ir).all() and torch.isnan(plain).all()


def test_sharded_and_graphed_renders_refuse_a_gain():
    case = sc.SpatialCase("c1_foa")
    r, pose, *_ = _setup(case)
    with pytest.raises(NotImplementedError):
        RayShardedRender(r, shard=(0, 2))(*pose, ray_gain=spatial.foa)
    with pytest.raises(NotImplementedError):
        GraphedRender(r).render_ir(*pose, ray_gain=spatial.foa)
