"""CPU: the stage references of tests/render_stage_cases.py compose to the
oracle, are adjoint to each other in float64, and every listed case meets
its live-fraction / transmittance condition (so no GPU stage test can pass on
an all-masked or all-absorbed input)."""
import numpy as np
import pytest
import torch

import render_stage_cases as rsc
from golden_util import Case
from avr_amd.workloads import RAF, Workload, grad_probe, make_inputs
from oracle import avr_oracle as orc


def _small_workloads():
    # odd T, S not a multiple of 4
    a = Workload("stage_oddT", rsc.render_cfg("meshrir", 6, 1023, n_azi=3, n_ele=2, shift_frac=0.3), 1023, 2)
    # speaker orientation present, S = 10
    rb = dict(RAF, n_azi=4, n_ele=3, n_samples=10)
    b = Workload("stage_raf", rb, 1600, 2, with_dir_tx=True)
    # one of the ragged golden shapes (asymmetric cube, S = 40, T = 2 mod 4), at B = 2
    c = Case("edge_ragged_s3").workload.replace(batch=2)
    return [a, b, c]


@pytest.mark.parametrize("w", _small_workloads(), ids=lambda w: w.name)
def test_stage_references_compose_to_the_oracle(w):
    inp = make_inputs(w, 3)
    B, R, S, T = w.batch, w.n_rays, w.n_samples, w.T
    attn = torch.from_numpy(inp["attn"]).requires_grad_(True)
    sig = torch.from_numpy(inp["signal"]).requires_grad_(True)
    cfg = orc.RenderConfig.from_kwargs(**w.render)
    dtx = None if inp["direction_tx"] is None else torch.from_numpy(inp["direction_tx"])
    rec = {}
    torch.manual_seed(3)
    out = orc.render_spectrum(cfg, orc.StubNetwork(attn, sig), torch.from_numpy(inp["rays_o"]),
                              torch.from_numpy(inp["position_tx"]), dtx, record=rec)
    g = grad_probe(w, 3)
    (out * torch.from_numpy(g)).sum().backward()
    assert float(out.detach().norm()) > 0

    shift = rec["shift"].numpy().astype(np.int64)
    delay = rec["delay"].numpy().astype(np.int64)
    pl = orc.path_loss_table(cfg, T).numpy()
    phase = orc.phase_rotation(rec["frac"], T).numpy()
    x = inp["signal"].reshape(B, R, S, T).astype(np.float64)
    a = inp["attn"].reshape(B, R, S).astype(np.float64)
    d_vals = rec["d_vals"].numpy()

    wt = rsc.ref_weights(a, d_vals)
    assert rsc.rel_l2(wt, rec["weights"].detach().numpy()) < 1e-5
    part = rsc.ref_reduce_fwd(x, wt, delay, shift, 2)
    spec = rsc.ref_dft_fwd(part, pl, shift, phase)
    o = out.detach().numpy()
    assert rsc.rel_l2(spec, o[..., 0] + 1j * o[..., 1]) < 1e-5

    gz = rsc.ref_dft_bwd(g[..., 0] + 1j * g[..., 1], pl, shift, phase, T)
    gx, gw = rsc.ref_reduce_bwd(x, gz, wt, delay, shift)
    _, ga = rsc.ref_weights(a, d_vals, gw)
    assert rsc.rel_l2(gx.reshape(sig.shape), sig.grad.numpy()) < 1e-5
    assert rsc.rel_l2(ga.reshape(attn.shape), attn.grad.numpy()) < 1e-5


@pytest.mark.parametrize("case", [rsc.DFT_CASES[0], rsc.DFT_CASES[2], rsc.DFT_BWD_EXTRA[1]], ids=lambda c: c.id)
def test_dft_references_are_adjoint(case):
    cfg = orc.RenderConfig.from_kwargs(**case.cfg())
    B, S, T = case.B, case.S, case.T
    F = T // 2 + 1
    frac, sh = orc.receiver_delay(cfg, orc.depth_samples(cfg))
    shift = sh.numpy().astype(np.int64)
    pl = orc.path_loss_table(cfg, T).numpy()
    phase = orc.phase_rotation(frac, T).numpy()
    rng = rsc.case_rng("adj", case.id)
    z = rng.standard_normal((1, B, S, T))
    g = rng.standard_normal((B, F)) + 1j * rng.standard_normal((B, F))
    out = rsc.ref_dft_fwd(z, pl, shift, phase)
    gz = rsc.ref_dft_bwd(g, pl, shift, phase, T)
    lhs = float((out.real * g.real + out.imag * g.imag).sum())
    rhs = float((z[0] * gz).sum())
    assert abs(lhs - rhs) <= 1e-12 * np.linalg.norm(out) * np.linalg.norm(g)


def test_reduce_references_are_adjoint():
    case = rsc.ReduceCase(5, 254, "float32")
    shift = rsc.host_shift(case.cfg(), case.T)
    xt, w, delay, gz1 = rsc.synth_reduce_inputs(case, shift)
    x = xt.double().numpy()
    part = rsc.ref_reduce_fwd(x, w, delay, shift, 1)
    gx, _ = rsc.ref_reduce_bwd(x, gz1, w, delay, shift)
    lhs = float((part[0] * gz1).sum())
    rhs = float((x * gx).sum())
    assert abs(lhs - rhs) <= 1e-12 * np.linalg.norm(part) * np.linalg.norm(gz1)
    # irfft pair
    rng = rsc.case_rng("irfft")
    s = rng.standard_normal((2, 129)) + 1j * rng.standard_normal((2, 129))
    gi = rng.standard_normal((2, 256))
    gs = rsc.ref_irfft_bwd(gi)
    lhs = float((rsc.ref_irfft(s) * gi).sum())
    rhs = float((s.real * gs.real + s.imag * gs.imag).sum())
    assert abs(lhs - rhs) <= 1e-12 * np.linalg.norm(s) * np.linalg.norm(gi)


_REDUCE_IDS = sorted({c.id: c for c in rsc.ALL_REDUCE}.items())


@pytest.mark.parametrize("case", [c for _, c in _REDUCE_IDS], ids=[i for i, _ in _REDUCE_IDS])
def test_reduce_cases_live_fraction_and_delay_edges(case):
    shift = rsc.host_shift(case.cfg(), case.T)
    T = case.T
    assert shift.max() <= 1.5 * T  # check_config
    delay = rsc.synth_delays(case, shift)
    assert delay.dtype == np.int32 and delay.min() >= 0 and delay.max() <= T - 1
    frac = rsc.live_mask(delay, shift, T).mean()
    assert 0.2 <= frac <= 0.9, frac
    for s in range(case.S):
        col = set(delay[:, :, s].reshape(-1).tolist())
        lim = T - 1 - int(shift[s])
        assert {0, T - 1, lim - 1, lim, min(lim + 1, T - 1)} <= col, (s, lim)
        ph = (s * T) % case.vec
        assert any({e - 1, e, e + 1} <= col for e in range(case.vec - ph, T - 1, case.vec)), s
        assert any(d >= lim for d in col)  # an empty row


@pytest.mark.parametrize("case", rsc.DFT_BWD_CASES, ids=lambda c: c.id)
def test_dft_cases_live_fraction(case):
    shift = rsc.host_shift(case.cfg(), case.T)
    assert shift.max() <= 1.5 * case.T
    assert 0.2 <= rsc.live_fraction_dft(case) <= 0.9


@pytest.mark.parametrize("dtype", rsc.WEIGHT_DTYPES)
@pytest.mark.parametrize("S", [s for s in rsc.WEIGHT_S if s >= 2])
def test_weight_cases_transmittance(S, dtype):
    cfg = rsc.weights_cfg(S)
    d_vals = orc.depth_samples(orc.RenderConfig.from_kwargs(**cfg)).numpy()
    tr = rsc.final_transmittance(rsc.synth_attn(S, dtype, cfg["far"]), d_vals)
    assert tr.min() >= 0.05 and tr.max() <= 0.5, (tr.min(), tr.max())
