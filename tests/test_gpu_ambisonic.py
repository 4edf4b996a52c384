"""GPU: binaural rendering.  The one-pass 16-channel ray reduction on the
fp32 MFMA against the float64 reference of tests/spatial_cases.py and, bit for
bit, against the vector kernel; the complex decode and its adjoint against
float64; `ambisonic(3)`, `sh_decoder=` and `mc_reduce=` end to end.

Bounds (u = 2^-24, derived, not measured):
* reduction: the bound of tests/test_gpu_spatial.py, a chain of n_r fused
  multiply-adds on the weights fl(w*g): |err| <= 2 (n_r + 2) u sum |g w x|.
* decode: K complex terms of four fmaf each, every real output a chain of 2K
  fused multiply-adds: |err| <= (2K + 2) u sum_k |dec||amb| per component
  (the adjoint with E terms is inside the same bound for E <= K)."""
import ctypes

import numpy as np
import pytest
import torch

import ambisonic_cases as ac
import render_stage_cases as rsc
import spatial_cases as sc
from golden_util import rel_l2
from test_gpu_render_stages import CODE, DEV, U, _nan, _reduce_operands, _st, ctx

from avr_amd import AVRRender, _lib, spatial
from avr_amd.auralize import auralize_path, convolve_trajectory
from avr_amd.graph import GraphedRender
from avr_amd.parallel import RayShardedRender
from avr_amd.renderer import (_render_core_mc_fwd, get_tables, reduce_mc16_max_rays, reduce_mc_splits,
                              render_params, sh_decode)

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _ids(lst):
    return [c.id for c in lst]


def _reduce(entry, o, case, C, gain_dev, n_split, part, sig=None):
    stride = 0 if gain_dev.dim() == 2 else C * case.R
    sig = o["x"] if sig is None else sig
    _lib.call(entry, ctypes.byref(o["p"]), case.B, C, sig.data_ptr(), CODE[case.dtype], o["w_dev"].data_ptr(),
              o["d_dev"].data_ptr(), gain_dev.data_ptr(), stride, n_split, part.data_ptr(), _st())


# ------------------------------------------------------------------- stage
@pytest.mark.parametrize("C", ac.CHANNELS)
@pytest.mark.parametrize("case", ac.MC16_FWD, ids=_ids(ac.MC16_FWD))
def test_ray_reduce_mc16_fwd(case, C):
    o = _reduce_operands(case)
    B, R, S, T = case.B, case.R, case.S, case.T
    assert case.vector and case.offset == 0 and S * T % case.vec == 0
    for per_pose in (False, True):
        gain = sc.synth_gain(case, C, per_pose)
        g_dev = torch.from_numpy(gain).to(DEV)
        for n_split in case.n_splits:
            part = _nan(n_split, B, C, S, T)
            _reduce("avr_ray_reduce_mc16_fwd", o, case, C, g_dev, n_split, part)
            torch.cuda.synchronize()
            got = part.cpu().numpy()
            assert not np.isnan(got).any(), "elements the stage owns were not written"
            ref, mag, n_r = sc.ref_reduce_mc_fwd(o["x64"], o["w"], o["delay"], o["host"]["shift"], gain, n_split)
            bound = 2.0 * (n_r[:, None, None, None, None] + 2) * U * mag
            err = np.abs(got.astype(np.float64) - ref)
            print(f"mc16_fwd {case.id} C={C} per_pose={per_pose} n_split={n_split}: "
                  f"{float((err / np.maximum(bound, 1e-300)).max()):.2f} of bound")
            assert np.all(got[mag == 0] == 0)
            assert np.all(err <= bound)
            if (R + n_split - 1) // n_split * (n_split - 1) >= R:
                assert np.all(got[-1] == 0)  # the empty last split
            # the strong claim: the vector kernel's sums, bit for bit
            vec = _nan(n_split, B, C, S, T)
            _reduce("avr_ray_reduce_mc_fwd", o, case, C, g_dev, n_split, vec)
            diff = int((part != vec).sum())
            print(f"  elements that differ from avr_ray_reduce_mc_fwd: {diff} of {part.numel()}")
            assert torch.equal(part, vec)


# ---------------------------------------------------------------- refusals
def _limit_operands(R, S=2, T=62, B=1, C=16):
    cfg = rsc.render_cfg("meshrir", S, T, n_azi=R, n_ele=1)
    p, tb, host = ctx(cfg, T, R)
    rng = rsc.case_rng("mc16-limit", R)
    x = rng.standard_normal((B, R, S, T)).astype(np.float32)
    w = rng.uniform(-1, 1, (B, R, S)).astype(np.float32)
    delay = rng.integers(0, T // 2, (B, R, S)).astype(np.int32)
    gain = rng.uniform(-1, 1, (C, R)).astype(np.float32)
    return p, host, x, w, delay, gain


def test_largest_split_and_one_ray_more():
    cap = reduce_mc16_max_rays()
    assert cap == (160 * 1024 // 68) // 32 * 32  # 68 bytes of LDS per ray, whole batches of ray groups
    p, host, x, w, delay, gain = _limit_operands(cap)
    B, R, S, T = x.shape
    dev = [torch.from_numpy(a).to(DEV) for a in (x, w, delay, gain)]
    part = _nan(1, B, 16, S, T)
    _lib.call("avr_ray_reduce_mc16_fwd", ctypes.byref(p), B, 16, dev[0].data_ptr(), 0, dev[1].data_ptr(),
              dev[2].data_ptr(), dev[3].data_ptr(), 0, 1, part.data_ptr(), _st())
    torch.cuda.synchronize()
    ref, mag, n_r = sc.ref_reduce_mc_fwd(x, w, delay, host["shift"], gain, 1)
    assert float(np.abs(ref).max()) > 0
    assert np.all(np.abs(part.cpu().numpy() - ref) <= 2.0 * (n_r[0] + 2) * U * mag)
    # one ray more in a single split: refused before any launch
    p1, host, x, w, delay, gain = _limit_operands(cap + 1)
    dev = [torch.from_numpy(a).to(DEV) for a in (x, w, delay, gain)]
    part = _nan(1, B, 16, S, T)
    with pytest.raises(RuntimeError, match=r"status 1001.*too many rays per split"):
        _lib.call("avr_ray_reduce_mc16_fwd", ctypes.byref(p1), B, 16, dev[0].data_ptr(), 0, dev[1].data_ptr(),
                  dev[2].data_ptr(), dev[3].data_ptr(), 0, 1, part.data_ptr(), _st())
    torch.cuda.synchronize()
    assert torch.isnan(part).all()


@pytest.mark.parametrize("C", [0, 17])
def test_channel_count_out_of_range_is_refused(C):
    case = ac.MC16_FWD[-2]
    o = _reduce_operands(case)
    gain = torch.zeros(max(C, 1), case.R, device=DEV)
    part = _nan(1, case.B, max(C, 1), case.S, case.T)
    with pytest.raises(RuntimeError, match=r"status 1001.*C must be 1..16"):
        _reduce("avr_ray_reduce_mc16_fwd", o, case, C, gain, 1, part)
    torch.cuda.synchronize()
    assert torch.isnan(part).all()


@pytest.mark.parametrize("case", ac.MC16_REFUSED, ids=_ids(ac.MC16_REFUSED))
def test_row_without_a_16_byte_form_is_refused(case):
    """S*T = 2044 halves: aligned, but a column's rows change phase within
    the tensor, so only the element-wise form could run it and none is built."""
    o = _reduce_operands(case)
    assert case.offset == 0 and case.S * case.T % case.vec != 0
    gain = torch.ones(16, case.R, device=DEV)
    for n_split in case.n_splits:
        part = _nan(n_split, case.B, 16, case.S, case.T)
        with pytest.raises(RuntimeError, match=r"status 1002.*16-byte form"):
            _reduce("avr_ray_reduce_mc16_fwd", o, case, 16, gain, n_split, part)
        torch.cuda.synchronize()
        assert torch.isnan(part).all()


def test_unaligned_signal_is_refused():
    """Only the 16-byte form is built: a signal one element off alignment is a
    configuration error before any launch, never another kernel."""
    case = ac.MC16_FWD[-2]
    o = _reduce_operands(case)
    buf = torch.zeros(o["x"].numel() + 8, device=DEV)
    off1 = buf[1:1 + o["x"].numel()].view(o["x"].shape)
    assert off1.data_ptr() % 16 == 4
    gain = torch.ones(16, case.R, device=DEV)
    part = _nan(1, case.B, 16, case.S, case.T)
    with pytest.raises(RuntimeError, match=r"status 1002.*16-byte form"):
        _reduce("avr_ray_reduce_mc16_fwd", o, case, 16, gain, 1, part, sig=off1)
    torch.cuda.synchronize()
    assert torch.isnan(part).all()


# ------------------------------------------------------------------ decode
@pytest.mark.parametrize("F", [128, 130])
@pytest.mark.parametrize("K", [4, 9, 16])
def test_sh_decode_forward_and_adjoint(K, F):
    B, E = 2, 2
    rng = rsc.case_rng("sh-decode", K, F)
    dec = rng.standard_normal((E, K, F, 2)).astype(np.float32)
    amb = rng.standard_normal((B, K, F, 2)).astype(np.float32)
    go = rng.standard_normal((B, E, F, 2)).astype(np.float32)
    dec[0, 1] = 0.0  # a silent channel of one ear
    d_dev, a_dev, g_dev = (torch.from_numpy(a).to(DEV) for a in (dec, amb, go))
    out, ga = _nan(B, E, F, 2), _nan(B, K, F, 2)
    _lib.call("avr_sh_decode_fwd", B, E, K, F, d_dev.data_ptr(), a_dev.data_ptr(), out.data_ptr(), _st())
    _lib.call("avr_sh_decode_bwd", B, E, K, F, d_dev.data_ptr(), g_dev.data_ptr(), ga.data_ptr(), _st())
    torch.cuda.synchronize()
    ref, mag = ac.ref_decode(ac.as_complex(dec), ac.as_complex(amb))
    ref_a, mag_a = ac.ref_decode_adjoint(ac.as_complex(dec), ac.as_complex(go))
    for name, got, r, m in (("fwd", out, ref, mag), ("adjoint", ga, ref_a, mag_a)):
        got = got.cpu().numpy()
        assert not np.isnan(got).any()
        err = np.maximum(np.abs(got[..., 0] - r.real), np.abs(got[..., 1] - r.imag))
        bound = (2 * K + 2) * U * m
        print(f"sh_decode {name} K={K} F={F}: {float((err / bound).max()):.2f} of bound")
        assert np.all(err <= bound)
    # the autograd wrapper is these two launches
    a_req = a_dev.clone().requires_grad_(True)
    y = sh_decode(a_req, torch.view_as_complex(d_dev))
    assert torch.equal(y.detach(), out)
    (y * g_dev).sum().backward()
    assert torch.equal(a_req.grad, ga)
    with pytest.raises(RuntimeError, match=r"status 1001.*K must be 1..16"):
        _lib.call("avr_sh_decode_fwd", B, E, 17, F, d_dev.data_ptr(), a_dev.data_ptr(), out.data_ptr(), _st())


# ---------------------------------------------------------------- end to end
class Net(torch.nn.Module):
    def __init__(self, attn, signal):
        super().__init__()
        self.attn, self.signal = attn, signal

    def forward(self, pts, view, tx, dir_tx=None):
        return self.attn, self.signal


def _setup(case, grads=False, **kw):
    w, inp = case.workload, case.inputs()
    attn = torch.from_numpy(inp["attn"]).to(DEV).requires_grad_(grads)
    sig = torch.from_numpy(inp["signal"]).to(DEV).requires_grad_(grads)
    dtx = None if inp["direction_tx"] is None else torch.from_numpy(inp["direction_tx"]).to(DEV)
    r = AVRRender(Net(attn, sig), **w.render, **kw)
    pose = (torch.from_numpy(inp["rays_o"]).to(DEV), torch.from_numpy(inp["position_tx"]).to(DEV), dtx)
    return r, pose, attn, sig, torch.from_numpy(case["gain"]).to(DEV)


def _decoder(case, order=3):
    """A two-ear MagLS decoder of the structural head on the case's bins."""
    w = case.workload
    grid = ac.fibonacci_sphere(256)
    H = spatial.spherical_head_hrtf(grid, w.render["fs"], w.T)
    return spatial.sh_decoder(H, grid, order, fs=w.render["fs"])


def _render(r, pose, seed, method="__call__", **kw):
    torch.manual_seed(seed)
    return getattr(r, method)(*pose, **kw)


def test_sh3_golden_under_both_reductions():
    """The bars of tests/test_gpu_spatial.py's golden test on 16 channels,
    with the vector kernels and with the one-pass MFMA kernel; the two renders
    are the same bits."""
    case = ac.AmbisonicCase("c1_sh3")
    w = case.workload
    got = {}
    for mode in ("vector", "mfma"):
        r, pose, attn, sig, gain = _setup(case, mc_reduce=mode)
        with torch.no_grad():
            out, ir = _render(r, pose, case.seed, "render_ir", ray_gain=gain)
            torch.manual_seed(case.seed)
            *_, geom = r.sample(*pose)
            p = r._params(w.T, w.n_rays)
            core, _, delay = _render_core_mc_fwd(attn.view(w.batch, -1), sig, gain, p, get_tables(p, DEV),
                                                 geom["rays_o"], geom["position_tx"], geom["dirs"], mc_reduce=mode)
        F = w.T // 2 + 1
        assert out.shape == (w.batch, 16, F, 2) and ir.shape == (w.batch, 16, 2 * (F - 1))
        assert torch.equal(core.view_as(out), out)
        o, i = out.cpu().numpy(), ir.cpu().numpy()
        for c in range(16):
            l2o, l2i = rel_l2(o[:, c], case["out"][:, c]), rel_l2(i[:, c], case["ir"][:, c])
            print(f"c1_sh3 {mode} channel {c}: spectrum {l2o:.2e} ir {l2i:.2e}")
            assert l2o < TOL and l2i < TOL
        np.testing.assert_array_equal(delay.cpu().numpy().astype(np.int16), case["delay"])
        got[mode] = (out, ir)
    assert torch.equal(got["vector"][0], got["mfma"][0]) and torch.equal(got["vector"][1], got["mfma"][1])
    with pytest.raises(ValueError, match="mc_reduce"):
        AVRRender(Net(attn, sig), mc_reduce="fast", **w.render)


def test_auto_changes_no_result_where_the_vector_form_does_not_apply():
    """raf_c5: five channels, S*T = 650 is no multiple of 4, so "auto" stays
    on the vector kernels and "mfma" is refused by the launcher."""
    case = sc.SpatialCase("raf_c5")
    outs = {}
    for mode in ("auto", "vector"):
        r, pose, attn, sig, gain = _setup(case, mc_reduce=mode)
        with torch.no_grad():
            outs[mode] = _render(r, pose, case.seed, ray_gain=gain)
    assert torch.equal(outs["auto"], outs["vector"])
    r, pose, attn, sig, gain = _setup(case, mc_reduce="mfma")
    with pytest.raises(RuntimeError, match=r"status 1002.*16-byte form"), torch.no_grad():
        _render(r, pose, case.seed, ray_gain=gain)
    # and where it applies, "auto" (default) and "vector" are the same bits too
    case = ac.AmbisonicCase("c1_sh3")
    for mode in ("auto", "vector"):
        r, pose, attn, sig, gain = _setup(case, **({} if mode == "auto" else {"mc_reduce": mode}))
        assert r.mc_reduce == mode
        with torch.no_grad():
            outs[mode] = _render(r, pose, case.seed, ray_gain=gain)
    assert torch.equal(outs["auto"], outs["vector"])


def test_binaural_render_is_the_decode_of_the_ambisonic_render():
    case = ac.AmbisonicCase("c1_sh3")
    w = case.workload
    r, pose, attn, sig, _ = _setup(case)
    dec = _decoder(case)
    F = w.T // 2 + 1
    assert dec.shape == (2, 16, F)
    amb = spatial.ambisonic(3)
    with torch.no_grad():
        a = _render(r, pose, case.seed, ray_gain=amb)
        out, ir = _render(r, pose, case.seed, "render_ir", ray_gain=amb, sh_decoder=dec)
        fwd = _render(r, pose, case.seed, ray_gain=amb, sh_decoder=dec.to(DEV))
    assert a.shape == (w.batch, 16, F, 2)
    assert out.shape == (w.batch, 2, F, 2) and ir.shape == (w.batch, 2, w.T)
    assert torch.equal(fwd, out)
    ref, mag = ac.ref_decode(dec.numpy(), ac.as_complex(a.cpu().numpy()))
    got = out.cpu().numpy()
    err = np.maximum(np.abs(got[..., 0] - ref.real), np.abs(got[..., 1] - ref.imag))
    print(f"binaural decode: {float((err / ((2 * 16 + 2) * U * mag)).max()):.2f} of bound")
    assert float(np.abs(ref).max()) > 0 and np.all(err <= (2 * 16 + 2) * U * mag)
    want_ir = np.fft.irfft(ref, n=w.T, axis=-1)
    assert rel_l2(ir.cpu().numpy(), want_ir) < 1e-5
    # with autograd recording the IR is taken differentiably: the same values
    out_g, ir_g = _render(r, pose, case.seed, "render_ir", ray_gain=amb, sh_decoder=dec)
    assert torch.equal(out_g, out) and rel_l2(ir_g.cpu().numpy(), ir.cpu().numpy()) < 1e-6


def test_per_pose_head_rotation():
    case = ac.AmbisonicCase("c1_sh3")
    r, pose, *_ = _setup(case)
    heads = spatial.head_rotation(torch.tensor([0.3, -1.1]), 0.2)
    with torch.no_grad():
        rot = _render(r, pose, case.seed, ray_gain=spatial.ambisonic(3, rotation=heads))
        plain = _render(r, pose, case.seed, ray_gain=spatial.ambisonic(3))
        torch.manual_seed(case.seed)
        *_, geom = r.sample(*pose)
        g = torch.stack([spatial.ambisonic(3, rotation=heads[i])(geom["dirs"]) for i in range(2)])
        by_hand = _render(r, pose, case.seed, ray_gain=g)
    assert rot.shape == plain.shape == (2, 16) + plain.shape[2:]
    assert torch.equal(rot[:, 0], plain[:, 0])  # W does not turn
    assert rel_l2(rot[:, 1:4].cpu().numpy(), plain[:, 1:4].cpu().numpy()) > 1e-2
    assert rel_l2(rot.cpu().numpy(), by_hand.cpu().numpy()) < 1e-5
    with pytest.raises(ValueError):  # three rotations for two poses
        _render(r, pose, case.seed, ray_gain=spatial.ambisonic(3, rotation=spatial.head_rotation(torch.zeros(3))))


def test_gradients_through_the_decode():
    """attn and signal gradients of a loss on the binaural spectrum against
    autograd through a torch einsum on the ambisonic render."""
    case = ac.AmbisonicCase("c1_sh3")
    w = case.workload
    r, pose, attn, sig, _ = _setup(case, grads=True)
    dec = _decoder(case).to(DEV)
    amb = spatial.ambisonic(3)
    G = torch.from_numpy(rsc.case_rng("binaural-probe").standard_normal((w.batch, 2, w.T // 2 + 1, 2))
                         .astype(np.float32)).to(DEV)
    out = _render(r, pose, case.seed, ray_gain=amb, sh_decoder=dec)
    (out * G).sum().backward()
    ga, gs = attn.grad.clone(), sig.grad.clone()
    attn.grad = sig.grad = None
    a = _render(r, pose, case.seed, ray_gain=amb)
    y = torch.view_as_real(torch.einsum("ekf,bkf->bef", dec, torch.view_as_complex(a)))
    assert rel_l2(y.detach().cpu().numpy(), out.detach().cpu().numpy()) < 1e-5
    (y * G).sum().backward()
    l2a = rel_l2(ga.cpu().numpy(), attn.grad.cpu().numpy())
    l2s = rel_l2(gs.cpu().numpy(), sig.grad.cpu().numpy())
    print(f"gradients through the decode: attn {l2a:.2e} signal {l2s:.2e}")
    assert float(attn.grad.abs().max()) > 0 and float(sig.grad.abs().max()) > 0
    assert l2a <= 1e-5 and l2s <= 1e-5


def test_decoder_shape_and_wrapper_refusals():
    case = ac.AmbisonicCase("c1_sh3")
    r, pose, *_ = _setup(case)
    dec = _decoder(case)
    amb = spatial.ambisonic(3)
    with torch.no_grad():
        with pytest.raises(ValueError, match="K = 16"):
            r(*pose, ray_gain=spatial.ambisonic(2), sh_decoder=dec)
        with pytest.raises(ValueError, match="bins"):
            r(*pose, ray_gain=amb, sh_decoder=dec[:, :, :-1])
        with pytest.raises(ValueError, match="needs ray_gain"):
            r(*pose, sh_decoder=dec)
        with pytest.raises(ValueError, match="needs ray_gain"):
            r.render_ir(*pose, sh_decoder=dec)
        with pytest.raises(NotImplementedError):
            RayShardedRender(r, shard=(0, 2))(*pose, ray_gain=amb, sh_decoder=dec)
        with pytest.raises(NotImplementedError):
            GraphedRender(r).render_ir(*pose, ray_gain=amb, sh_decoder=dec)


def test_head_tracked_walk():
    """auralize_path with per-pose head rotations and a decoder equals the
    per-pose render_ir and convolve_trajectory by hand."""
    from avr_amd.renderer import draw_jitter

    case = ac.AmbisonicCase("c1_sh3")
    r, pose, *_ = _setup(case)
    dec = _decoder(case)
    heads = spatial.head_rotation(torch.tensor([0.0, 0.8]))
    amb = spatial.ambisonic(3, rotation=heads)
    x = torch.from_numpy(rsc.case_rng("walk").standard_normal(700).astype(np.float32)).to(DEV)
    torch.manual_seed(4)
    y = auralize_path(r, pose[0], pose[1], x, 350, ray_gain=amb, sh_decoder=dec)
    torch.manual_seed(4)
    u = draw_jitter(r.n_azi, r.n_ele)
    with torch.no_grad():
        _, ir = r.render_ir(pose[0], pose[1], ray_gain=amb, sh_decoder=dec, u_azi=u)
    want = convolve_trajectory(ir, x, 350)
    assert y.shape == (2, 700 + case.workload.T - 1) and torch.isfinite(y).all() and float(y.abs().max()) > 0
    assert torch.equal(y, want)
    with pytest.raises(ValueError, match="per-pose ray_gain needs 2 poses"):
        auralize_path(r, pose[0], pose[1], x, 350, ray_gain=spatial.ambisonic(3, rotation=torch.eye(3).expand(3, 3, 3)))
