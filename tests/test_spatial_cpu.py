"""CPU: receiver patterns (avr_amd.spatial) against the reference's values, the
multi-channel stage references against the golden renders, and the oracle on
gain-scaled signals against the same goldens bit for bit."""
import numpy as np
import pytest
import torch

import render_stage_cases as rsc
import spatial_cases as sc
from avr_amd import spatial
from oracle import avr_oracle as orc

RENDER = sc.render_case_names()


def _dirs(n_azi=73, n_ele=14, seed=5):
    torch.manual_seed(seed)
    return orc.sphere_directions(n_azi, n_ele)[0]


def test_goldens_present():
    assert set(RENDER) == {"c1_foa", "c1_pair", "c1_pair_fp16", "raf_c5"}
    assert len(sc.load_patterns()) == 12


def test_wide_cardioid_matches_the_reference_bit_for_bit():
    seen = set()
    for row, phi, want in sc.load_patterns():
        got = spatial.wide_cardioid_beam_pattern(row["facing"], torch.from_numpy(phi), base_level=row["base_level"])
        assert got.dtype == torch.float32 and np.array_equal(got.numpy(), want), row
        assert float(got.max()) == 1.0
        seen.add((row["base_level"], len(phi), row["facing"]))
    assert len(seen) == 12
    # base_level 0 is falsy: it counts as 1.0
    phi = torch.from_numpy(sc.load_patterns()[0][1])
    assert torch.equal(spatial.wide_cardioid_beam_pattern(2.1, phi, 0), spatial.wide_cardioid_beam_pattern(2.1, phi, 1.0))


def test_foa_rows():
    d = _dirs()
    g = spatial.foa(d)
    assert g.shape == (4, d.size(0)) and g.dtype == torch.float32
    assert torch.all(g[0] == 1.0)
    n2 = (g[1:].double() ** 2).sum(0)
    assert float((n2 - 1).abs().max()) <= 4 * 2.0 ** -23
    # ACN order W, Y, Z, X: the poles are the last two rays (0, 0, +-1)
    assert g[:, -2].tolist() == [1.0, 0.0, 1.0, 0.0] and g[:, -1].tolist() == [1.0, 0.0, -1.0, 0.0]


def test_first_order_family():
    d = _dirs()
    axis = (0.3, -0.2, 0.9)
    assert torch.all(spatial.first_order(d, axis, 1) == 1.0)
    a = torch.tensor(axis) / torch.tensor(axis).norm()
    cosang = (d * a).sum(-1)
    np.testing.assert_allclose(spatial.first_order(d, axis, 0.0).numpy(), cosang.numpy(), atol=1e-6)
    card = spatial.first_order(d, axis, 0.5)
    assert float(card.min()) >= -1e-6 and float(card.max()) <= 1 + 1e-6


def test_azimuth_and_cardioid_pair():
    d = _dirs(8, 3)
    az = spatial.azimuth(d)
    np.testing.assert_allclose(az.numpy(), np.arctan2(d[:, 1].numpy(), d[:, 0].numpy()), atol=1e-6)
    pair = spatial.cardioid_pair(90, 110)(d)
    assert pair.shape == (2, d.size(0))
    # left capsule looks towards azimuth 145 deg, right towards 35 deg
    for row, deg in zip(pair, (145.0, 35.0)):
        a = np.radians(deg)
        want = 0.5 + 0.5 * (d[:, 0] * np.cos(a) + d[:, 1] * np.sin(a))
        np.testing.assert_allclose(row.numpy(), want.numpy(), atol=1e-6)


@pytest.fixture(scope="module", params=RENDER)
def rendered(request):
    case = sc.SpatialCase(request.param)
    out, rec, cfg = sc.oracle_render(case)
    return case, out, rec, cfg


def test_oracle_on_scaled_signals_equals_the_golden(rendered):
    case, out, rec, _ = rendered
    assert float(np.linalg.norm(case["out"])) > 0
    assert np.array_equal(out.numpy(), case["out"])
    assert np.array_equal(rec["delay"].numpy().astype(np.int16), case["delay"])
    ir = torch.stack([orc.spectrum_to_ir(out[:, c]) for c in range(case.C)], 1)
    assert np.array_equal(ir.numpy(), case["ir"])


def test_mc_stage_references_compose_to_the_golden(rendered):
    """ref_reduce_mc_fwd/bwd with the existing DFT and weight references
    reproduce the golden spectrum and gradients: this proves the references
    the GPU tests use, not the kernels.  Bars: test_render_stages_cpu.py's."""
    case, _, rec, cfg = rendered
    w, inp = case.workload, case.inputs()
    B, R, S, T, C = w.batch, w.n_rays, w.n_samples, w.T, case.C
    shift = rec["shift"].numpy().astype(np.int64)
    delay = rec["delay"].numpy().astype(np.int64)
    pl = orc.path_loss_table(cfg, T).numpy()
    phase = orc.phase_rotation(rec["frac"], T).numpy()
    x = inp["signal"].reshape(B, R, S, T).astype(np.float64)
    a = inp["attn"].reshape(B, R, S).astype(np.float64)
    d_vals = rec["d_vals"].numpy()
    gain = case["gain"]
    wt = rsc.ref_weights(a, d_vals)
    part, _, _ = sc.ref_reduce_mc_fwd(x, wt, delay, shift, gain, 2)
    spec = rsc.ref_dft_fwd(part.reshape(2, B * C, S, T), pl, shift, phase).reshape(B, C, -1)
    o = case["out"]
    for c in range(C):
        assert rsc.rel_l2(spec[:, c], o[:, c, :, 0] + 1j * o[:, c, :, 1]) < 1e-5

    G = case.grad_probe().reshape(B * C, -1, 2)
    gz = rsc.ref_dft_bwd(G[..., 0] + 1j * G[..., 1], pl, shift, phase, T).reshape(B, C, S, T)
    gx, gw, *_ = sc.ref_reduce_mc_bwd(x, gz, wt, delay, shift, gain)
    _, ga = rsc.ref_weights(a, d_vals, gw)
    assert rsc.rel_l2(ga.reshape(case["grad_attn"].shape), case["grad_attn"]) < 1e-5
    half = w.signal_dtype == "float16"  # the reference stores an fp16 signal's gradient in fp16
    flat = gx.reshape(-1)
    if case.has("grad_signal"):
        assert rsc.rel_l2(flat, case["grad_signal"].reshape(-1)) < (1e-3 if half else 1e-5)
    else:
        assert rsc.rel_l2(flat[case["grad_signal_idx"]], case["grad_signal_at"]) < (1e-3 if half else 1e-5)
    assert abs(float(flat.sum()) - float(case["grad_signal_sum"])) <= 1e-3 * np.sqrt(
        float(case["grad_signal_sumsq"]) * flat.size)


def test_mc_references_are_adjoint():
    case = sc.MC_BWD[-1]
    shift = rsc.host_shift(case.cfg(), case.T)
    xt, w, delay, _ = rsc.synth_reduce_inputs(case, shift)
    x = xt.double().numpy()
    for per_pose in (False, True):
        gain = sc.synth_gain(case, 3, per_pose)
        gz = sc.synth_gz(case, 3)
        part, _, _ = sc.ref_reduce_mc_fwd(x, w, delay, shift, gain, 1)
        gx, gw, *_ = sc.ref_reduce_mc_bwd(x, gz, w, delay, shift, gain)
        lhs = float((part[0] * gz).sum())
        assert abs(lhs - float((gx * x).sum())) <= 1e-12 * np.linalg.norm(part) * np.linalg.norm(gz)
        assert abs(lhs - float((gw * w).sum())) <= 1e-12 * np.linalg.norm(part) * np.linalg.norm(gz)
        assert (gain == 0).any() and np.abs(gain).max() <= 1
