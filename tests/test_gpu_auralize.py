"""GPU: avr_amd.auralize against the fixtures written from the reference's
whitenoise_bandpass_doa.py (tools/gen_auralize_golden.py).  Every test prints
its figures before it asserts.

Bars (set by the issue, from CPU figures): time-domain convolution
max|y - y_ref| <= 1e-5 max|y_ref| (the reference's own fp32 result sits 1.4e-7
from float64 at Nh = 4094, a strictly sequential fp32 chain 1.5e-6; one
dropped white tap costs >= 1e-3); the spectrum-input case 2e-5 (the fp32 irfft
adds its own error); the band-pass 1e-9 of the output's largest value in fp64
(tests/test_auralize_cpu.py: a same-recurrence float64 restatement sits
<= 2e-15 from scipy).

Measured on MI355X (fractions of the reference's largest output): convolution
meshrir (spectrum input) 1.29e-6, ragged 4.6e-7, short_x 2.9e-7, one_nh1 and
one_nh2 0, groups 5.5e-7, long_ir 1.75e-6; band-pass bp_meshrir 6.5e-16,
bp_block 1.95e-15, bp_n28 1.8e-15, single sections 0 (the same figures as the
float64 restatement on the CPU); every exact test exact.
"""
import numpy as np
import pytest
import torch

import auralize_cases as ac

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def aur():
    from avr_amd import auralize

    return auralize


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.fixture(scope="module")
def conv_out(dev, aur):
    """Every convolution case computed once, shared by the tests below."""
    out = {}
    for name, *_ , kind in ac.CONV_CASES:
        h, x = ac.conv_inputs(name)
        f = aur.synth_observation if kind == "spec" else aur.convolve_source
        out[name] = f(_t(h, dev), _t(x, dev))
    torch.cuda.synchronize()
    return out


# ------------------------------------------------ convolution vs fixtures

@pytest.mark.parametrize("name", [c[0] for c in ac.CONV_CASES])
def test_convolution_matches_reference(name, conv_out):
    _, C, Nh, L, S, _, kind = ac.CONV[name]
    z = ac.load(f"conv_{name}")
    y = conv_out[name]
    assert y.dtype == torch.float32
    assert tuple(y.shape) == ((C, L + Nh - 1) if S == 1 else (S, C, L + Nh - 1))
    y = y.cpu().numpy()
    amax = float(z["y_absmax"])
    err = np.abs(y[..., z["rows"], :] - z["y_rows"]).max()
    if len(z["cols"]):
        err = max(err, np.abs(y[..., :, z["cols"]] - z["y_cols"]).max())
    bar = 2e-5 if kind == "spec" else 1e-5
    print(f"conv {name}: max err {err / amax:.2e} of max|y_ref| (bar {bar:.0e})")
    assert np.isfinite(y).all()
    assert err <= bar * amax


# ------------------------------------------------ exact, no tolerance

@pytest.mark.parametrize("Nh", [255, 1022])
def test_unit_impulses_are_exact(Nh, dev, aur):
    taps = [0, 1, 31, 32, 63, 64, Nh - 1]
    L = 701
    h = torch.zeros(len(taps), Nh)
    for c, k in enumerate(taps):
        h[c, k] = 1.0
    x = torch.from_numpy(np.random.default_rng(5).standard_normal(L).astype(np.float32))
    y = aur.convolve_source(h.to(dev), x.to(dev)).cpu()
    want = torch.zeros(len(taps), L + Nh - 1)
    for c, k in enumerate(taps):
        want[c, k:k + L] = x
    bad = int((y != want).sum())
    print(f"impulses Nh={Nh}: {bad} elements differ")
    assert bad == 0


def test_rows_do_not_depend_on_the_batch(dev, aur, conv_out):
    h, x = ac.conv_inputs("groups")
    hd, xd = _t(h, dev), _t(x[0], dev)
    full = aur.convolve_source(hd, xd)
    assert torch.equal(full, conv_out["groups"][0])
    for c in (0, 7, 31, 32, 39):
        alone = aur.convolve_source(hd[c:c + 1], xd)
        same = torch.equal(alone[0], full[c])
        print(f"row {c} alone == in the batch of 40: {same}")
        assert same
    for n in (16, 17):  # both sides of the switch between the 16-row and the 32-row kernel
        same = torch.equal(aur.convolve_source(hd[:n], xd), full[:n])
        print(f"rows 0..{n - 1} as a batch of {n} == in the batch of 40: {same}")
        assert same
    for lo in (0, 32):
        eight = aur.convolve_source(hd[lo:lo + 8], xd)
        same = torch.equal(eight, full[lo:lo + 8])
        print(f"rows {lo}..{lo + 7} as a batch of 8 == in the batch of 40: {same}")
        assert same


def test_runs_repeat_bitwise(dev, aur, conv_out):
    for name in ("groups", "long_ir"):
        h, x = ac.conv_inputs(name)
        again = aur.convolve_source(_t(h, dev), _t(x, dev))
        same = torch.equal(again, conv_out[name])
        print(f"{name}: second run bitwise equal: {same}")
        assert same


def test_sources_form_equals_single_calls(dev, aur, conv_out):
    h, x = ac.conv_inputs("groups")
    hd = _t(h, dev)
    for s in range(x.shape[0]):
        one = aur.convolve_source(hd, _t(x[s], dev))
        same = torch.equal(one, conv_out["groups"][s])
        print(f"source {s}: [L] call == row {s} of the [S, L] call: {same}")
        assert same


def test_large_offsets_are_64_bit(dev, aur):
    """288 channels x 1.9e6 samples: the output passes 2^31 bytes.  The last
    channel (a unit impulse at tap 3) must land in the last row."""
    C, Nh, L = 288, 4, 1_900_000
    h = torch.zeros(C, Nh)
    h[:, 0] = 1.0
    h[C - 1] = torch.tensor([0.0, 0.0, 0.0, 1.0])
    x = torch.from_numpy(np.random.default_rng(6).standard_normal(L).astype(np.float32)).to(dev)
    y = aur.convolve_source(h.to(dev), x)
    assert y.numel() * 4 > 2 ** 31
    ok = bool(torch.equal(y[C - 1, 3:], x)) and bool((y[C - 1, :3] == 0).all())
    ok0 = bool(torch.equal(y[0, :L], x)) and bool(torch.equal(y[C - 2, :L], x))
    print(f"last row exact: {ok}; first and next-to-last rows exact: {ok0}")
    assert ok and ok0


# ------------------------------------------------ band-pass vs fixtures

@pytest.fixture(scope="module")
def meshrir_y():
    return np.ascontiguousarray(ac.load("conv_meshrir")["y_rows"])


@pytest.mark.parametrize("name", [c[0] for c in ac.BP_CASES + ac.SINGLE_CASES])
def test_zero_phase_matches_scipy(name, dev, aur, meshrir_y):
    z = ac.load(name)
    y = ac.bp_input(name, meshrir_y if name == "bp_meshrir" else None)
    yd = _t(y, dev)
    worst = 0.0
    for i, (sos, want, amax) in enumerate(zip(z["sos"], z["out_cols"], z["out_absmax"])):
        out = aur.zero_phase_sos(yd, sos if i % 2 else torch.from_numpy(sos).to(dev))  # host and device tables
        assert out.dtype == torch.float64 and out.shape == yd.shape
        got = out.cpu().numpy()
        assert np.isfinite(got).all()
        worst = max(worst, np.abs(got[:, z["cols"]] - want).max() / amax)
        # the columns the fixture does not keep: the CPU-pinned restatement
        if name == "bp_block":
            full = ac.restate_sosfiltfilt(sos, y)
            worst = max(worst, np.abs(got - full).max() / amax)
        out32 = aur.zero_phase_sos(yd, sos, out_dtype=torch.float32)
        assert out32.dtype == torch.float32
        assert torch.equal(out32, out.float()), "fp32 output is not the fp64 output rounded"
    print(f"zero-phase {name}: max err {worst:.2e} of max|ref| (bar 1e-9)")
    assert worst <= 1e-9


def test_zero_phase_leading_dims_and_length_check(dev, aur):
    z = ac.load("bp_n28")
    sos = z["sos"][0]
    y = _t(ac.bp_input("bp_n28"), dev)
    with pytest.raises(ValueError, match="padlen"):
        aur.zero_phase_sos(y[:, :27], sos)
    flat = aur.zero_phase_sos(y, sos)
    nested = aur.zero_phase_sos(y.reshape(3, 1, 28), sos)
    assert nested.shape == (3, 1, 28) and torch.equal(nested.reshape(3, 28), flat)
    assert torch.equal(aur.zero_phase_sos(y[1], sos), flat[1])


# ------------------------------------------------ the chain

def test_auralize_dump_runs_the_chain(dev, aur, conv_out, tmp_path):
    from avr_amd.data import write_val_dump

    spec, x = ac.conv_inputs("meshrir")
    rx = np.arange(24, dtype=np.float32).reshape(8, 3)
    tx = np.ones((8, 3), np.float32)
    path = write_val_dump(str(tmp_path / "val_iter000001.npz"), spec[::-1].copy(), spec, rx, tx, ac.FS)
    xd = _t(x, dev)
    sos = ac.load("bp_meshrir")["sos"][0]
    d = aur.auralize_dump(path, xd)
    assert torch.equal(d["pred"], conv_out["meshrir"])
    assert torch.equal(d["ori"], conv_out["meshrir"].flip(0))
    assert d["position_rx"].device.type == "cuda" and torch.equal(d["position_rx"].cpu(), torch.from_numpy(rx))
    assert torch.equal(d["position_tx"].cpu(), torch.from_numpy(tx))
    b = aur.auralize_dump(path, xd, sos=sos)
    assert b["pred"].dtype == torch.float64
    assert torch.equal(b["pred"], aur.zero_phase_sos(conv_out["meshrir"], sos))
    L, H = aur.seg_hop_samples(ac.FS, 64.0, 0.5)
    fr = aur.sliding_frames(b["pred"], L, H)
    assert fr.shape == (8, (5021 - L) // H + 1, L) and fr.data_ptr() == b["pred"].data_ptr()
    assert torch.equal(fr[3, 2], b["pred"][3, 2 * H:2 * H + L])
    w = aur.white_noise(0.01, ac.FS, 3, dev)
    assert w.device.type == "cuda" and w.shape == (160,)
