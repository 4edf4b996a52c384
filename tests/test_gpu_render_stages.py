"""GPU: every kernel stage of the render core against its float64 reference
(tests/render_stage_cases.py), called through the C-ABI one entry point at a
time, at the smallest shape that reaches each launch branch.

Every output buffer is pre-filled with NaN and must come back without one:
a stage writes every element it owns, zeros included (dead chunks, empty ray
splits, empty k-slices).  Reduction bounds are derived (u = 2^-24); the DFT
stages are bounded by a float32 yardstick with the kernel's summation shape
(DESIGN.md section 2 holds the measured figures)."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import render_stage_cases as rsc
from oracle import avr_oracle as orc

from avr_amd import AVRRender, _lib, spectrum_to_ir
from avr_amd.renderer import get_tables, render_params

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
U = rsc.U32
CODE = {"float32": 0, "float16": 1, "bfloat16": 2}
LIMIT = _lib.IRFFT_MAX_N
LIMIT_TEXT = f"n > {LIMIT}"


def _report(stage, shape, dtype, l2, mx, e32, bound):
    """One row of DESIGN.md section 2's table (shown with pytest -s)."""
    print(f"STAGE | {stage} | {shape} | {dtype} | {l2:.2e} | {mx} | {e32} | {bound}")


def _st():
    return torch.cuda.current_stream().cuda_stream


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


@functools.lru_cache(maxsize=None)
def _ctx(cfg_items, T, R):
    """(params, device tables, host copies of the device tables)."""
    cfg = dict(cfg_items)
    p = render_params(cfg, T, n_rays=R)
    tb = get_tables(p, DEV)
    torch.cuda.synchronize()
    ph = tb.phase.cpu().numpy()
    host = dict(shift=tb.shift.cpu().numpy().astype(np.int64), pl=tb.pl.cpu().numpy(), phase32=ph,
                phase=ph[..., 0].astype(np.float64) + 1j * ph[..., 1].astype(np.float64),
                d_vals=tb.d_vals.cpu().numpy())
    return p, tb, host


def ctx(cfg, T, R=None):
    return _ctx(tuple(sorted(cfg.items())), T, R if R is not None else cfg["n_azi"] * cfg["n_ele"] + 2)


# ------------------------------------------------------------------ reductions
@functools.lru_cache(maxsize=None)
def _reduce_operands(case):
    p, tb, host = ctx(case.cfg(), case.T, case.R)
    xt, w, delay, gz = rsc.synth_reduce_inputs(case, host["shift"])
    assert 0.2 <= rsc.live_mask(delay, host["shift"], case.T).mean() <= 0.9
    n = xt.numel()
    buf = torch.zeros(n + 8, dtype=xt.dtype, device=DEV)  # 16-byte aligned base
    x_dev = buf[case.offset:case.offset + n].view(xt.shape)
    x_dev.copy_(xt)
    assert (x_dev.data_ptr() % 16 == 0) == (case.offset == 0)
    return dict(p=p, host=host, x64=xt.double().numpy(), x=x_dev, w=w, delay=delay, gz=gz,
                w_dev=torch.from_numpy(w).to(DEV), d_dev=torch.from_numpy(delay).to(DEV),
                gz_dev=torch.from_numpy(gz).to(DEV))


def _reduce_fwd(case, n_split):
    o = _reduce_operands(case)
    part = _nan(n_split, case.B, case.S, case.T)
    _lib.call("avr_ray_reduce_fwd", ctypes.byref(o["p"]), case.B, o["x"].data_ptr(), CODE[case.dtype],
              o["w_dev"].data_ptr(), o["d_dev"].data_ptr(), n_split, part.data_ptr(), _st())
    torch.cuda.synchronize()
    return part.cpu().numpy(), o


def _check_reduce_fwd(case, n_split):
    got, o = _reduce_fwd(case, n_split)
    assert not np.isnan(got).any(), "elements the stage owns were not written"
    ref, mag, n_r = rsc.ref_reduce_fwd(o["x64"], o["w"], o["delay"], o["host"]["shift"], n_split, with_bound=True)
    bound = 2.0 * (n_r[:, None, None, None] + 1) * U * mag
    err = np.abs(got.astype(np.float64) - ref)
    _report("ray_reduce_fwd" + ("" if case.vector else " (scalar)"), f"{case.S}x{case.T} R={case.R} n_split={n_split}",
            case.dtype, rsc.rel_l2(got, ref), f"{float((err / np.maximum(bound, 1e-300)).max()):.2f} of bound", "-",
            "2(n_r+1)u sum|w x|")
    assert np.all(got[mag == 0] == 0)  # no live ray: exactly zero
    assert np.all(err <= bound)
    if (case.R + n_split - 1) // n_split * (n_split - 1) >= case.R:
        assert np.all(got[-1] == 0)  # the empty last split


def _cases(lst):
    return pytest.mark.parametrize("case", lst, ids=[c.id for c in lst])


@_cases(rsc.REDUCE_FWD_VECTOR)
def test_ray_reduce_fwd_vector(case):
    assert case.S * case.T % case.vec == 0
    for n_split in case.n_splits:
        _check_reduce_fwd(case, n_split)


@_cases(rsc.REDUCE_SCALAR)
def test_ray_reduce_fwd_scalar(case):
    assert case.offset or case.S * case.T % case.vec != 0
    for n_split in case.n_splits:
        _check_reduce_fwd(case, n_split)


def _check_reduce_bwd(case):
    o = _reduce_operands(case)
    tdt = rsc.TORCH_DTYPE[case.dtype]
    n = o["x"].numel()
    gbuf = _nan(n + 8, dtype=tdt)
    gx = gbuf[case.offset:case.offset + n].view(o["x"].shape)
    gw = _nan(case.B, case.R, case.S)
    _lib.call("avr_ray_reduce_bwd", ctypes.byref(o["p"]), case.B, o["x"].data_ptr(), CODE[case.dtype],
              o["gz_dev"].data_ptr(), o["w_dev"].data_ptr(), o["d_dev"].data_ptr(), gx.data_ptr(),
              gw.data_ptr(), _st())
    torch.cuda.synchronize()
    assert not torch.isnan(gx).any() and not torch.isnan(gw).any()
    assert torch.isnan(gbuf[:case.offset]).all() and torch.isnan(gbuf[case.offset + n:]).all()  # nothing outside
    shift = o["host"]["shift"]
    _, ref_gw, mag, n_live = rsc.ref_reduce_bwd(o["x64"], o["gz"], o["w"], o["delay"], shift, with_bound=True)
    live = rsc.live_mask(o["delay"], shift, case.T)
    # grad_x: the kernel rounds a single fp32 product (then the storage cast)
    prod = np.where(live, o["w"][..., None] * o["gz"][:, None], np.float32(0)).astype(np.float32)
    want = torch.from_numpy(prod).to(tdt)
    assert np.array_equal(gx.cpu().float().numpy(), want.float().numpy())
    err = np.abs(gw.cpu().numpy().astype(np.float64) - ref_gw)
    bound = 2.0 * (n_live + 8) * U * mag
    _report("ray_reduce_bwd grad_w" + ("" if case.vector else " (scalar)"), f"{case.S}x{case.T} R={case.R}", case.dtype,
            rsc.rel_l2(gw.cpu().numpy(), ref_gw), f"{float((err / np.maximum(bound, 1e-300)).max()):.2f} of bound", "-",
            "2(n_live+8)u sum|gz x|; grad_x exact")
    assert np.all(err <= bound)


@_cases(rsc.REDUCE_BWD_VECTOR)
def test_ray_reduce_bwd_vector(case):
    _check_reduce_bwd(case)


@_cases(rsc.REDUCE_SCALAR)
def test_ray_reduce_bwd_scalar(case):
    _check_reduce_bwd(case)


def test_scalar_path_refuses_five_chunks_per_lane():
    """S*T not a multiple of the vector width and T > 4096: the scalar kernels
    would need 5 chunks per lane; both entry points refuse."""
    case = rsc.SCALAR_LIMIT
    o = _reduce_operands(case)
    part = _nan(1, case.B, case.S, case.T)
    with pytest.raises(RuntimeError, match="T too long"):
        _lib.call("avr_ray_reduce_fwd", ctypes.byref(o["p"]), case.B, o["x"].data_ptr(), 0, o["w_dev"].data_ptr(),
                  o["d_dev"].data_ptr(), 1, part.data_ptr(), _st())
    gx, gw = torch.empty_like(o["x"]), _nan(case.B, case.R, case.S)
    with pytest.raises(RuntimeError, match="T too long"):
        _lib.call("avr_ray_reduce_bwd", ctypes.byref(o["p"]), case.B, o["x"].data_ptr(), 0, o["gz_dev"].data_ptr(),
                  o["w_dev"].data_ptr(), o["d_dev"].data_ptr(), gx.data_ptr(), gw.data_ptr(), _st())
    torch.cuda.synchronize()


# ------------------------------------------------------------------ DFT stages
@functools.lru_cache(maxsize=None)
def _dft_operands(case, n_split):
    p, tb, host = ctx(case.cfg(), case.T)
    F = case.T // 2 + 1
    rng = rsc.case_rng("dft", case.id, n_split)
    part = rng.standard_normal((n_split, case.B, case.S, case.T)).astype(np.float32)
    g = rng.standard_normal((case.B, F, 2)).astype(np.float32)
    ref = rsc.ref_dft_fwd(part, host["pl"], host["shift"], host["phase"])
    return dict(p=p, tb=tb, host=host, part=part, g=g, ref=ref, part_dev=torch.from_numpy(part).to(DEV),
                g_dev=torch.from_numpy(g).to(DEV))


def _dft_fwd(case, n_split, k_split):
    o = _dft_operands(case, n_split)
    p, tb = o["p"], o["tb"]
    B, S, T = case.B, case.S, case.T
    F = T // 2 + 1
    P = math.ceil(S / 32) * k_split
    spart, out = _nan(B, P, F, 2), _nan(B, F, 2)
    _lib.call("avr_dft_phase_fwd", ctypes.byref(p), B, o["part_dev"].data_ptr(), n_split, tb.pl.data_ptr(),
              tb.shift.data_ptr(), tb.phase.data_ptr(), tb.twiddle.data_ptr(), k_split, spart.data_ptr(), _st())
    _lib.call("avr_spectrum_finalize", B, P, F, spart.data_ptr(), out.data_ptr(), _st())
    torch.cuda.synchronize()
    assert not torch.isnan(spart).any(), "a k-slice or s-tile partial was not written"
    assert not torch.isnan(out).any()
    o_ = out.cpu().numpy().astype(np.float64)
    return o_[..., 0] + 1j * o_[..., 1], spart, o


@functools.lru_cache(maxsize=None)
def _e32_fwd(case, n_split, k_split):
    o = _dft_operands(case, n_split)
    F = case.T // 2 + 1
    bins = np.arange(F) if case.T <= 4096 else rsc.subset(F, 64, seed=case.T)
    y = rsc.yardstick_dft_fwd(o["part"], o["host"]["pl"], o["host"]["shift"], o["host"]["phase32"], k_split, bins)
    return rsc.rel_l2(y, o["ref"][:, bins])


def _lib_k_split(case):
    """The k-split the library picks for this shape (avr_render_core_layout)."""
    p, tb, _ = ctx(case.cfg(), case.T)
    return tb.core_layout(p, case.B, _lib.DTYPE_F32)[2]


def _k_list(case):
    ks = [_lib_k_split(case)]
    return ks + [k for k in case.forced_k() if k not in ks]


@_cases(rsc.DFT_FWD_CASES)
def test_dft_phase_fwd(case):
    for n_split in case.n_splits:
        for k_split in _k_list(case):
            got, spart, o = _dft_fwd(case, n_split, k_split)
            e32 = _e32_fwd(case, n_split, k_split)
            b_l2, b_max = rsc.dft_bounds(e32)
            l2, mx = rsc.rel_l2(got, o["ref"]), rsc.rel_max(got, o["ref"])
            _report("dft_phase_fwd + finalize", f"{case.S}x{case.T} n_split={n_split} k_split={k_split}", "float32", l2,
                    f"{mx:.2e}", f"{e32:.2e}", f"{b_l2:.2e}")
            assert l2 <= b_l2 and mx <= b_max
            nkc = math.ceil(case.T / 64)
            kchunk = math.ceil(nkc / k_split) * 64
            for ks in range(k_split):  # a slice that starts past T is empty: exact zeros
                if ks * kchunk >= case.T:
                    assert torch.all(spart.view(case.B, -1, k_split, spart.size(2), 2)[:, :, ks] == 0)


def _dft_bwd(case):
    o = _dft_operands(case, 1)
    p, tb = o["p"], o["tb"]
    gz = _nan(case.B, case.S, case.T)
    _lib.call("avr_dft_phase_bwd", ctypes.byref(p), case.B, o["g_dev"].data_ptr(), tb.pl.data_ptr(),
              tb.shift.data_ptr(), tb.phase.data_ptr(), tb.twiddle.data_ptr(), gz.data_ptr(), _st())
    torch.cuda.synchronize()
    assert not torch.isnan(gz).any()
    return gz.cpu().numpy().astype(np.float64), o


@functools.lru_cache(maxsize=None)
def _bwd_ref_e32(case):
    o = _dft_operands(case, 1)
    T, h = case.T, o["host"]
    g = o["g"]
    ref = rsc.ref_dft_bwd(g[..., 0].astype(np.float64) + 1j * g[..., 1], h["pl"], h["shift"], h["phase"], T)
    samples = np.arange(T) if T <= 4096 else rsc.subset(T, 64, seed=T + 1)
    # the live part of the window, so the yardstick's error is not diluted by zeros
    y = rsc.yardstick_dft_bwd(g, h["pl"], h["shift"], h["phase32"], T, samples)
    return ref, rsc.rel_l2(y, ref[:, :, samples])


@_cases(rsc.DFT_BWD_CASES)
def test_dft_phase_bwd(case):
    got, o = _dft_bwd(case)
    ref, e32 = _bwd_ref_e32(case)
    b_l2, b_max = rsc.dft_bounds(e32)
    l2, mx = rsc.rel_l2(got, ref), rsc.rel_max(got, ref)
    _report("dft_phase_bwd", f"{case.S}x{case.T}", "float32", l2, f"{mx:.2e}", f"{e32:.2e}", f"{b_l2:.2e}")
    assert l2 <= b_l2 and mx <= b_max
    t = np.arange(case.T)
    dead = t[None, :] >= (case.T - 1 - o["host"]["shift"])[:, None]
    assert dead.any() and np.all(got[:, dead] == 0)  # the tail mask: exact zeros


@_cases(rsc.DFT_CASES)
def test_dft_device_adjointness(case):
    """<fwd(z), g> = <z, bwd(g)> on the device results, in float64, within the
    sum of the two stages' bounds (Cauchy-Schwarz on their relative L2 errors)."""
    k = _lib_k_split(case)
    out, _, o = _dft_fwd(case, 1, k)
    gz, _ = _dft_bwd(case)
    g = o["g"].astype(np.float64)
    z = o["part"][0].astype(np.float64)
    lhs = float((out.real * g[..., 0] + out.imag * g[..., 1]).sum())
    rhs = float((z * gz).sum())
    ref_gz, e32b = _bwd_ref_e32(case)
    bf, _ = rsc.dft_bounds(_e32_fwd(case, 1, k))
    bb, _ = rsc.dft_bounds(e32b)
    tol = bf * np.linalg.norm(o["ref"]) * np.linalg.norm(g) + bb * np.linalg.norm(ref_gz) * np.linalg.norm(z)
    print(f"dft adjoint {case.id}: |lhs-rhs| {abs(lhs - rhs):.3e} tol {tol:.3e}")
    assert abs(lhs - rhs) <= tol


# ---------------------------------------------------------------------- tables
@_cases(rsc.DFT_BWD_CASES)
def test_tables(case):
    cfg, T = case.cfg(), case.T
    p, tb, host = ctx(cfg, T)
    F = T // 2 + 1
    a = 2.0 * np.pi * np.arange(T) / T
    np.testing.assert_allclose(tb.twiddle.cpu().numpy(), np.stack([np.cos(a), -np.sin(a)], -1), rtol=0, atol=1.2e-7)
    n = 2 * (F - 1)
    a = 2.0 * np.pi * np.arange(n) / n
    np.testing.assert_allclose(tb.ir_twiddle.cpu().numpy()[:n], np.stack([np.cos(a), np.sin(a)], -1),
                               rtol=0, atol=1.2e-7)
    oc = orc.RenderConfig.from_kwargs(**cfg)
    pl_ref = orc.path_loss_table(oc, T).numpy()
    assert host["pl"].shape == pl_ref.shape
    if not np.array_equal(host["pl"], pl_ref):
        print(f"tables {case.id}: pl differs from the oracle's expression, max rel "
              f"{np.abs(host['pl'] / pl_ref - 1).max():.2e}")
        np.testing.assert_allclose(host["pl"], pl_ref, rtol=1e-6, atol=0)
    frac, sh = orc.receiver_delay(oc, orc.depth_samples(oc))
    ph = orc.phase_rotation(frac, T).numpy()
    err = np.abs(host["phase"] - ph).max()
    _report("tables: phase (pl, shift equal)", f"{case.S}x{case.T}", "float32", rsc.rel_l2(host["phase"], ph), f"{err:.2e} abs",
            "-", "3e-6 abs")
    assert err <= 3e-6
    np.testing.assert_array_equal(host["shift"], sh.numpy().astype(np.int64))


# --------------------------------------------------------------------- weights
def _poses(B):
    rng = rsc.case_rng("pose", B)
    return (rng.uniform(-2, 2, (B, 3)).astype(np.float32), rng.uniform(-2, 2, (B, 3)).astype(np.float32))


@pytest.mark.parametrize("dtype", rsc.WEIGHT_DTYPES)
@pytest.mark.parametrize("S", rsc.WEIGHT_S)
def test_weights_fwd_bwd(S, dtype):
    cfg = rsc.weights_cfg(S)
    B, R, T = rsc.WEIGHT_B, rsc.WEIGHT_R, rsc.WEIGHT_T
    p, tb, host = ctx(cfg, T)
    attn = rsc.synth_attn(S, dtype, cfg["far"])
    if S >= 2:
        tr = rsc.final_transmittance(attn, host["d_vals"])
        assert tr.min() >= 0.05 and tr.max() <= 0.5
    ro, tx = _poses(B)
    r = AVRRender(None, **cfg)
    torch.manual_seed(S)
    *_, geom = r.sample(torch.from_numpy(ro).to(DEV), torch.from_numpy(tx).to(DEV))
    a_dev = attn.to(DEV).contiguous()
    w, dl = _nan(B, R, S), torch.full((B, R, S), -1, dtype=torch.int32, device=DEV)
    _lib.call("avr_weights_fwd", ctypes.byref(p), B, a_dev.data_ptr(), CODE[dtype], geom["rays_o"].data_ptr(),
              geom["position_tx"].data_ptr(), geom["dirs"].data_ptr(), tb.d_vals.data_ptr(), w.data_ptr(),
              dl.data_ptr(), _st())
    rng = rsc.case_rng("gw", S, dtype)
    gw = (rng.standard_normal((B, R, S)) * (S / cfg["far"])).astype(np.float32)
    ga = _nan(B, R, S, dtype=rsc.TORCH_DTYPE[dtype])
    gw_dev = torch.from_numpy(gw).to(DEV)
    _lib.call("avr_weights_bwd", ctypes.byref(p), B, a_dev.data_ptr(), CODE[dtype], tb.d_vals.data_ptr(),
              gw_dev.data_ptr(), ga.data_ptr(), _st())
    torch.cuda.synchronize()
    assert not torch.isnan(w).any() and not torch.isnan(ga).any()
    d = dl.cpu().numpy()
    assert d.min() >= 0 and d.max() <= T - 1
    a64 = attn.double().numpy()
    ref_w, ref_ga = rsc.ref_weights(a64, host["d_vals"], gw)
    y_w, y_ga = rsc.weights_yardstick(attn.float().numpy(), host["d_vals"], gw)
    e32w = np.abs(y_w - ref_w).max()
    e32g = rsc.rel_l2(y_ga, ref_ga)
    err = np.abs(w.cpu().numpy() - ref_w)
    assert np.all(err <= np.maximum(4 * e32w, 2e-7 + 1e-5 * np.abs(ref_w)))
    half_ulp = {"float32": 0.0, "float16": 2.0 ** -11, "bfloat16": 2.0 ** -8}[dtype]
    bound = min(max(4 * e32g, 1e-5), 1e-3) + half_ulp
    l2 = rsc.rel_l2(ga.cpu().double().numpy(), ref_ga)
    _report("weights_fwd", f"S={S}", dtype, rsc.rel_l2(w.cpu().numpy(), ref_w), f"{err.max():.2e} abs", f"{e32w:.2e} abs",
            f"max(4 e32, 2e-7 + 1e-5|w|)")
    _report("weights_bwd", f"S={S}", dtype, l2, "-", f"{e32g:.2e}", f"{bound:.2e}")
    assert l2 <= bound


# ------------------------------------------------------- irfft and its LDS limit
class _Net(torch.nn.Module):
    def __init__(self, attn, signal):
        super().__init__()
        self.attn, self.signal, self.calls = attn, signal, 0

    def forward(self, pts, view, tx, dir_tx=None):
        self.calls += 1
        return self.attn, self.signal


def _ir_setup(T):
    S, R, B = 2, 7, 2
    cfg = rsc.render_cfg("meshrir", S, T)
    rng = rsc.case_rng("ir", T)
    attn = torch.from_numpy(rng.uniform(0, 2, (B, R * S, 1)).astype(np.float32) / cfg["far"]).to(DEV)
    sig = torch.from_numpy(rng.standard_normal((B, R * S, T)).astype(np.float32)).to(DEV)
    ro, tx = _poses(B)
    return cfg, attn, sig, torch.from_numpy(ro).to(DEV), torch.from_numpy(tx).to(DEV)


def test_render_ir_at_the_largest_accepted_length():
    """render_ir (avr_render_core_fwd with ir_out) at the largest even T the
    irfft accepts, against the float64 composition of the stage references on
    the device's own weights, delays and tables."""
    T, S, R, B = LIMIT, 2, 7, 2
    cfg, attn, sig, ro, tx = _ir_setup(T)
    r = AVRRender(_Net(attn, sig), **cfg)
    with torch.no_grad():
        torch.manual_seed(0)
        out, ir = r.render_ir(ro, tx)
        torch.manual_seed(0)
        *_, geom = r.sample(ro, tx)
    p, tb, host = ctx(cfg, T)
    w = torch.empty(B, R, S, device=DEV)
    dl = torch.empty(B, R, S, dtype=torch.int32, device=DEV)
    _lib.call("avr_weights_fwd", ctypes.byref(p), B, attn.data_ptr(), 0, geom["rays_o"].data_ptr(),
              geom["position_tx"].data_ptr(), geom["dirs"].data_ptr(), tb.d_vals.data_ptr(), w.data_ptr(),
              dl.data_ptr(), _st())
    torch.cuda.synchronize()
    delay = dl.cpu().numpy()
    assert 0.2 <= rsc.live_mask(delay, host["shift"], T).mean() <= 0.9
    part = rsc.ref_reduce_fwd(sig.cpu().double().numpy().reshape(B, R, S, T), w.cpu().numpy(), delay,
                              host["shift"], 1)
    spec = rsc.ref_dft_fwd(part, host["pl"], host["shift"], host["phase"])
    o = out.cpu().double().numpy()
    assert ir.shape == (B, T)
    assert rsc.rel_l2(o[..., 0] + 1j * o[..., 1], spec) < 1e-4
    assert rsc.rel_l2(ir.cpu().double().numpy(), rsc.ref_irfft(spec)) < 1e-4


def test_render_ir_past_the_limit_is_refused_before_the_core_runs():
    T = 16384
    cfg, attn, sig, ro, tx = _ir_setup(T)
    r = AVRRender(_Net(attn, sig), **cfg)
    with torch.no_grad():
        out = r(ro, tx)  # the spectrum alone renders at T = 16384
        assert torch.isfinite(out).all()
        with pytest.raises(RuntimeError, match=LIMIT_TEXT):
            r.render_ir(ro, tx)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match=LIMIT_TEXT):
        spectrum_to_ir(out)


def test_irfft_stage_against_float64():
    """avr_irfft / avr_irfft_bwd with non-zero imaginary parts at DC and
    Nyquist, at n = 2, the 64 KiB opt-in threshold and the limit."""
    for F in (2, 65, 2731, 2732, LIMIT // 2 + 1):
        n = 2 * (F - 1)
        rng = rsc.case_rng("irfft", F)
        spec = rng.standard_normal((2, F, 2)).astype(np.float32)
        g = rng.standard_normal((2, n)).astype(np.float32)
        tw = _nan(n, 2)
        _lib.call("avr_ir_twiddle", n, tw.data_ptr(), _st())
        ir, gs = _nan(2, n), _nan(2, F, 2)
        sd, gd = torch.from_numpy(spec).to(DEV), torch.from_numpy(g).to(DEV)
        _lib.call("avr_irfft", 2, F, sd.data_ptr(), tw.data_ptr(), ir.data_ptr(), _st())
        _lib.call("avr_irfft_bwd", 2, F, gd.data_ptr(), tw.data_ptr(), gs.data_ptr(), _st())
        torch.cuda.synchronize()
        assert not torch.isnan(ir).any() and not torch.isnan(gs).any()
        s64 = spec[..., 0].astype(np.float64) + 1j * spec[..., 1]
        gsn = gs.cpu().double().numpy()
        l2f = rsc.rel_l2(ir.cpu().double().numpy(), rsc.ref_irfft(s64))
        l2b = rsc.rel_l2(gsn[..., 0] + 1j * gsn[..., 1], rsc.ref_irfft_bwd(g))
        _report("irfft", f"n={n}", "float32", l2f, "-", "-", "1e-5")
        _report("irfft_bwd", f"n={n}", "float32", l2b, "-", "-", "1e-5")
        assert l2f < 1e-5 and l2b < 1e-5
    for name in ("avr_irfft", "avr_irfft_bwd"):  # the first refused length, before any launch
        with pytest.raises(RuntimeError, match=LIMIT_TEXT):
            _lib.call(name, 1, LIMIT // 2 + 2, sd.data_ptr(), tw.data_ptr(), ir.data_ptr(), _st())
