"""CPU: `avr_amd.spatial`'s higher-order ambisonics, the spherical-head
transfer functions and the decoder fits, against float64 statements written
independently of the code under test (tests/ambisonic_cases.py), and the
golden render of the 16 order-3 channels against the oracle."""
import math

import numpy as np
import pytest
import torch

import ambisonic_cases as ac
import spatial_cases as sc
from avr_amd import spatial
from oracle import avr_oracle as orc


def _dirs(n, seed=0):
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n, 3))
    return torch.from_numpy((d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32))


def _render_dirs(n_azi=12, n_ele=8):
    torch.manual_seed(5)
    return orc.sphere_directions(n_azi, n_ele)[0].double()


# --------------------------------------------------------------- ambisonic
def test_first_four_rows_are_foa_bit_for_bit():
    d = _dirs(257) * 1.7  # not normalised: both normalise
    for order in (1, 2, 3):
        assert torch.equal(spatial.ambisonic(order)(d)[:4], spatial.foa(d))
    assert torch.equal(spatial.ambisonic(0)(d), spatial.foa(d)[:1])
    assert [spatial.ambisonic(o)(d).shape[0] for o in range(4)] == [1, 4, 9, 16]
    with pytest.raises(ValueError):
        spatial.ambisonic(4)


def test_rows_match_the_legendre_recurrence():
    """About 8 fp32 operations on terms whose magnitudes sum to at most 4:
    4e-6 absolute."""
    d = _dirs(1000, 1)
    d = torch.cat([d, torch.tensor([[0, 0, 1.0], [0, 0, -1.0], [1.0, 0, 0], [0, -1.0, 0]])])
    got = spatial.ambisonic(3)(d).double().numpy()
    ref = ac.sh_reference(d.double().numpy(), 3)
    err = np.abs(got - ref).max(axis=1)
    print("max |err| per row:", np.array2string(err, precision=2))
    assert err.max() <= 4e-6
    got64 = spatial.ambisonic(3)(d.double()).numpy()
    assert np.abs(got64 - ac.sh_reference(d.double().numpy(), 3)).max() <= 1e-14


def test_gram_matrix_on_the_gauss_legendre_grid():
    dirs, w = ac.gauss_legendre_grid(16, 32)
    Y = spatial.ambisonic(3)(torch.from_numpy(dirs).float()).double().numpy()
    gram = (Y * w) @ Y.T
    want = np.diag([1.0 / (2 * n + 1) for n in range(4) for _ in range(2 * n + 1)])
    print("max |gram - diag(1/(2n+1))|:", float(np.abs(gram - want).max()))
    assert np.abs(gram - want).max() <= 1e-5


# ---------------------------------------------------------------- rotation
def test_rotation_is_the_gain_of_rotated_directions():
    d = _dirs(64, 2)
    Rm = spatial.head_rotation(0.7, -0.3, 1.9).float()
    assert torch.allclose(Rm @ Rm.T, torch.eye(3), atol=1e-6) and abs(float(torch.det(Rm)) - 1) < 1e-6
    assert torch.equal(spatial.ambisonic(3, rotation=Rm)(d), spatial.ambisonic(3)(d @ Rm))


def test_quarter_yaw_moves_a_source_at_left_to_front():
    Rm = spatial.head_rotation(math.pi / 2)
    left = torch.tensor([[0.0, 1.0, 0.0]], dtype=torch.float64)
    front = torch.tensor([[1.0, 0.0, 0.0]], dtype=torch.float64)
    got = spatial.ambisonic(3, rotation=Rm)(left)
    assert torch.allclose(got, spatial.ambisonic(3)(front), atol=1e-15)
    assert got[3, 0] == pytest.approx(1.0) and abs(float(got[1, 0])) < 1e-15  # X = 1, Y = 0


def test_per_pose_rotations_and_slicing():
    d = _dirs(32, 3)
    heads = spatial.head_rotation(torch.linspace(0, 2.0, 5), 0.1, torch.tensor([0.0, 0.2, 0.4, 0.6, 0.8])).float()
    assert heads.shape == (5, 3, 3)
    amb = spatial.ambisonic(3, rotation=heads)
    assert amb.per_pose and len(amb) == 5 and not spatial.ambisonic(3).per_pose
    g = amb(d)
    assert g.shape == (5, 16, 32)
    for i in range(5):
        assert torch.allclose(g[i], spatial.ambisonic(3, rotation=heads[i])(d), atol=1e-6)
    cut = amb[1:3]
    assert cut.per_pose and len(cut) == 2 and torch.equal(cut(d), g[1:3])
    assert amb[4].per_pose and torch.equal(amb[4](d), g[4:5])
    with pytest.raises(TypeError):
        len(spatial.ambisonic(3, rotation=heads[0]))


# ----------------------------------------------------------------- decoder
def test_ls_recovers_a_band_limited_decoder():
    """On the renderer's own directions for n_azi = 12, n_ele = 8 (cond(Y)
    about 3.5; the 32-ray grid's is 39)."""
    dirs = _render_dirs()
    Y = spatial.ambisonic(3)(dirs).numpy().T
    cond = np.linalg.cond(Y)
    print("cond(Y):", cond)
    assert cond < 10
    rng = np.random.default_rng(4)
    F = 65
    D0 = rng.standard_normal((2, 16, F)) + 1j * rng.standard_normal((2, 16, F))
    H = np.einsum("jk,ekf->jef", Y, D0)
    D = spatial.sh_decoder(H, dirs, 3, method="ls")
    assert D.shape == (2, 16, F) and D.dtype == torch.complex64
    # the solve to 1e-9 (dtype= keeps its float64 result); the default
    # complex64 output is that result rounded once
    D64 = spatial.sh_decoder(H, dirs, 3, method="ls", dtype=torch.complex128)
    rel = np.linalg.norm(D64.numpy() - D0) / np.linalg.norm(D0)
    print("relative error of the recovered decoder:", rel)
    assert rel <= 1e-9
    assert torch.equal(D, D64.to(torch.complex64))
    # impulse responses with n= are transformed first
    hrir = rng.standard_normal((dirs.shape[0], 2, 20))
    a = spatial.sh_decoder(hrir, dirs, 3, method="ls", n=128)
    b = spatial.sh_decoder(np.fft.rfft(hrir, n=128, axis=-1), dirs, 3, method="ls")
    assert torch.equal(a, b)
    with pytest.raises(ValueError):
        spatial.sh_decoder(hrir, dirs, 3, method="ls")
    with pytest.raises(ValueError):
        spatial.sh_decoder(H, dirs, 3, method="magls")  # no fs


@pytest.mark.parametrize("fs,T", ac.RATES)
def test_magls_keeps_the_magnitude_above_the_cutoff(fs, T):
    grid = ac.fibonacci_sphere(512)
    H = spatial.spherical_head_hrtf(grid, fs, T).numpy()
    Y = ac.sh_reference(grid, 3).T
    freqs = fs * np.arange(T // 2 + 1) / T
    hi, lo = freqs >= 2000.0, freqs < 1000.0
    err = {}
    for method in ("ls", "magls"):
        D = spatial.sh_decoder(H, grid, 3, method=method, fs=fs).numpy().astype(np.complex128)
        fit = np.einsum("jk,ekf->jef", Y, D)
        err[method] = (np.linalg.norm((np.abs(fit) - np.abs(H))[..., hi]) / np.linalg.norm(np.abs(H)[..., hi]),
                       np.linalg.norm((fit - H)[..., lo]) / np.linalg.norm(H[..., lo]))
        err[method + "_D"] = D
    print(f"fs={fs} T={T}: magnitude error >= 2 kHz ls {err['ls'][0]:.3f} magls {err['magls'][0]:.3f}; "
          f"complex error < 1 kHz ls {err['ls'][1]:.3f} magls {err['magls'][1]:.3f}")
    assert err["magls"][0] <= 0.1 and err["magls"][0] <= 0.25 * err["ls"][0]
    below = freqs < 1500.0
    assert np.array_equal(err["ls_D"][..., below], err["magls_D"][..., below])


# -------------------------------------------------------------------- head
def test_spherical_head_symmetry_dc_and_arrival():
    d = _dirs(50, 6).double()
    fs, n = 48000.0, 256
    H = spatial.spherical_head_hrtf(d, fs, n)
    assert H.shape == (50, 2, n // 2 + 1) and H.dtype == torch.complex128
    mirror = d * torch.tensor([1.0, -1.0, 1.0], dtype=torch.float64)
    Hm = spatial.spherical_head_hrtf(mirror, fs, n)
    assert torch.equal(H[:, 0], Hm[:, 1]) and torch.equal(H[:, 1], Hm[:, 0])
    assert torch.allclose(H[..., 0].abs(), torch.ones(50, 2, dtype=torch.float64), atol=1e-15)
    # a source at +y (left): the left ear leads by the Woodworth path a/c (1 + pi/2)
    left = spatial.spherical_head_hrtf(torch.tensor([[0.0, 1.0, 0.0]]), fs, n)[0]
    ir = torch.fft.irfft(left, n=n)
    onset = [int(torch.nonzero(ir[e].abs() > 0.3 * ir[e].abs().max())[0]) for e in range(2)]
    itd = 0.0875 / 343.0 * (1 + math.pi / 2) * fs
    print("onsets (samples):", onset, "expected lag", itd)
    assert onset[0] < onset[1] and abs((onset[1] - onset[0]) - itd) <= 2


# ------------------------------------------------------------------ golden
def test_decode_statement_matches_einsum():
    rng = np.random.default_rng(9)
    dec = rng.standard_normal((2, 16, 7)) + 1j * rng.standard_normal((2, 16, 7))
    amb = rng.standard_normal((3, 16, 7)) + 1j * rng.standard_normal((3, 16, 7))
    ref, mag = ac.ref_decode(dec, amb)
    want = torch.einsum("ekf,bkf->bef", torch.from_numpy(dec), torch.from_numpy(amb)).numpy()
    assert np.abs(ref - want).max() <= 1e-13 * mag.max()
    g = rng.standard_normal((3, 2, 7)) + 1j * rng.standard_normal((3, 2, 7))
    adj, _ = ac.ref_decode_adjoint(dec, g)
    # <decode(amb), g> = <amb, adjoint(g)> (real inner product of complex vectors)
    assert abs(np.vdot(g, ref).real - np.vdot(adj, amb).real) <= 1e-12 * np.abs(ref).sum()


def test_oracle_reproduces_the_sh3_golden():
    """As tests/test_spatial_cpu.py for its goldens: the oracle behind the
    gain-scaled stub network gives the fixture's 16 channels bit for bit."""
    case = ac.AmbisonicCase("c1_sh3")
    assert case.C == 16 and case["gain"].shape == (16, case.workload.n_rays)
    out, rec, _ = sc.oracle_render(case)
    assert torch.equal(out, torch.from_numpy(case["out"]))
    assert torch.equal(rec["dirs"], torch.from_numpy(case["dirs"]))
    np.testing.assert_array_equal(rec["delay"].numpy().astype(np.int16), case["delay"])
    # the fixture's gains are ambisonic(3) on the reference's own jittered directions
    assert torch.equal(spatial.ambisonic(3)(torch.from_numpy(case["dirs"])), torch.from_numpy(case["gain"]))
    ir = torch.stack([orc.spectrum_to_ir(out[:, c]) for c in range(case.C)], 1)
    assert torch.equal(ir, torch.from_numpy(case["ir"]))
