"""CPU: the host side of avr_amd.auralize against the fixtures written from
the reference's whitenoise_bandpass_doa.py (tools/gen_auralize_golden.py),
the float64 restatement of sosfiltfilt the GPU tests lean on, and argument
refusals that need no device.

Measured when the fixtures were written (numpy 2.2.6, scipy 1.15.3), printed
again by each test:

* restate_sosfiltfilt vs scipy: at most 1.95e-15 of the output's largest
  value over the four reference bands (6.5e-16 on 8 x 5021, 1.95e-15 on
  40 x 300, 1.8e-15 at n = 28) and 0 on the single sections (bar here: 1e-12).
  That is the distance a same-recurrence fp64 implementation sits from scipy,
  and it supports the GPU test's 1e-9 bar with five decades to spare.
* sosfilt_zi vs scipy.signal.sosfilt_zi: at most 2.9e-16 of the table's
  largest entry (bar 1e-14).
"""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import auralize_cases as ac
from avr_amd import _lib, auralize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BP_ALL = [c[0] for c in ac.BP_CASES + ac.SINGLE_CASES]


@pytest.fixture(scope="module")
def meshrir_y():
    z = ac.load("conv_meshrir")
    return np.ascontiguousarray(z["y_rows"])


def _bp_input(name, meshrir_y):
    return ac.bp_input(name, meshrir_y if name == "bp_meshrir" else None)


# ------------------------------------------------------------- fixtures

def test_fixture_sizes():
    total = 0
    for f in os.listdir(ac.GOLDEN):
        sz = os.path.getsize(os.path.join(ac.GOLDEN, f))
        assert sz <= 256 * 1024, (f, sz)
        total += sz
    print(f"fixtures: {total / 1024:.0f} KB")
    assert total <= 1024 * 1024


@pytest.mark.parametrize("name", [c[0] for c in ac.CONV_CASES])
def test_conv_inputs_regenerate(name):
    z = ac.load(f"conv_{name}")
    h, x = ac.conv_inputs(name)
    assert np.array_equal(z["digest"], ac.digest(h, x))
    rows, cols = ac.conv_keep(name)
    assert np.array_equal(z["rows"], rows) and np.array_equal(z["cols"], cols)


@pytest.mark.parametrize("name", ["ragged", "short_x", "one_nh1", "one_nh2", "groups"])
def test_conv_fixture_is_a_convolution(name):
    """The stored rows against a float64 convolution: the reference's own fp32 error."""
    z = ac.load(f"conv_{name}")
    h, x = ac.conv_inputs(name)
    xs = x[None] if x.ndim == 1 else x
    ref = np.stack([[np.convolve(xi.astype(np.float64), h[c].astype(np.float64)) for c in z["rows"]] for xi in xs])
    got = z["y_rows"].reshape(ref.shape)
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"{name}: reference fp32 vs float64 {err:.2e}")
    assert err < 1e-6


# ----------------------------------------------------------- white noise

def test_white_noise_matches_reference():
    z = ac.load("white_noise")
    for (sec, fs, seed), dig, n in zip(json.loads(str(z["meta"]))["cases"], z["digest"], z["length"]):
        x = auralize.white_noise(sec, fs, seed, "cpu")
        assert x.dtype == torch.float32 and x.numel() == n
        assert np.array_equal(ac.digest(x.numpy())[:18], dig)


# --------------------------------------------------------------- framing

def test_seg_hop_samples_over_the_reference_grid():
    grid = ac.load("frames")["grid"]
    assert grid.shape == (21, 4)
    for seg_ms, ov, L, H in grid:
        assert auralize.seg_hop_samples(ac.FS, float(seg_ms), float(ov)) == (int(L), int(H))


def test_sliding_frames_is_the_reference_list_as_a_view():
    z = ac.load("frames")
    y = torch.arange(2 * 1000, dtype=torch.float32).reshape(2, 1000)
    L, H = 256, 192
    fr = auralize.sliding_frames(y, L, H)
    ref = [y[..., i:i + L] for i in range(0, 1000 - L + 1, H)]  # whitenoise_bandpass_doa.py:117
    assert fr.shape == (2, len(ref), L)
    assert np.array_equal(fr[0, :, 0].numpy(), z["starts"])
    for i, r in enumerate(ref):
        assert torch.equal(fr[:, i], r)
    assert fr.untyped_storage().data_ptr() == y.untyped_storage().data_ptr()
    y[1, 192] = -5.0
    assert fr[1, 1, 0] == -5.0 and fr[1, 0, 192] == -5.0
    short = auralize.sliding_frames(y[:, :100], L, H)
    assert short.shape == (2, 0, L) and int(z["n_short"]) == 0
    assert auralize.sliding_frames(y[:, :L], L, H).shape == (2, 1, L)


# ------------------------------------------------------ zi, padlen, restate

@pytest.mark.parametrize("name", BP_ALL)
def test_sosfilt_zi_matches_scipy(name):
    z = ac.load(name)
    worst = 0.0
    for sos, zi in zip(z["sos"], z["zi"]):
        got = auralize.sosfilt_zi(sos)
        assert got.dtype == np.float64 and got.shape == zi.shape
        assert np.array_equal(got, ac.restate_zi(sos))
        worst = max(worst, (np.abs(got - zi) / np.abs(zi).max()).max())
    print(f"{name}: sosfilt_zi vs scipy {worst:.2e}")
    assert worst <= 1e-14
    assert np.array_equal(auralize.sosfilt_zi(torch.from_numpy(z["sos"][0])), auralize.sosfilt_zi(z["sos"][0]))


def test_padlen_rule():
    for name in BP_ALL:
        z = ac.load(name)
        want = json.loads(str(z["meta"]))["padlen"]
        for sos in z["sos"]:
            assert auralize.sos_padlen(sos) == want == ac.restate_padlen(sos)
    assert auralize.sos_padlen(ac.load("bp_block")["sos"][0]) == 27
    assert auralize.sos_padlen(ac.load("single_o2")["sos"][0]) == 9
    assert auralize.sos_padlen(ac.load("single_o1")["sos"][0]) == 6  # b2 = a2 = 0
    sos = np.array([[1, 0, 0, 1, 0.5, 0.1], [1, 0.2, 0, 1, 0.3, 0.0]])  # min(#b2, #a2) = 1
    assert auralize.sos_padlen(sos) == 3 * (5 - 1)
    with pytest.raises(ValueError):
        auralize.sos_padlen(np.ones((2, 5)))
    with pytest.raises(ValueError):
        auralize.sosfilt_zi(np.array([[1, 0, 0, 2.0, 0, 0]]))  # a0 != 1, as scipy's sosfilt refuses


@pytest.mark.parametrize("name", BP_ALL)
def test_restatement_is_pinned_to_scipy(name, meshrir_y):
    z = ac.load(name)
    y = _bp_input(name, meshrir_y)
    assert np.array_equal(z["digest"], ac.digest(y))
    worst = 0.0
    for sos, want, amax in zip(z["sos"], z["out_cols"], z["out_absmax"]):
        got = ac.restate_sosfiltfilt(sos, y)[:, z["cols"]]
        worst = max(worst, np.abs(got - want).max() / amax)
    print(f"{name}: restatement vs scipy {worst:.2e}")
    assert worst <= 1e-12


def test_restatement_refuses_n_at_padlen():
    sos = ac.load("bp_n28")["sos"][0]
    with pytest.raises(ValueError, match="padlen"):
        ac.restate_sosfiltfilt(sos, np.zeros((1, 27), np.float32))


# --------------------------------------------------- refusals without a device

def test_cpu_tensors_raise():
    h, x = torch.zeros(2, 8), torch.zeros(16)
    with pytest.raises(RuntimeError, match="HIP tensor"):
        auralize.convolve_source(h, x)
    with pytest.raises(RuntimeError, match="HIP tensor"):
        auralize.synth_observation(torch.zeros(2, 5, dtype=torch.complex64), x)
    with pytest.raises(RuntimeError, match="HIP tensor"):
        auralize.zero_phase_sos(torch.zeros(2, 64), ac.load("bp_n28")["sos"][0])
    with pytest.raises(RuntimeError, match="HIP tensor"):
        auralize.auralize_dump({"pred_sig": np.zeros((8, 5), np.complex64)}, x)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "avr_amd", "csrc"), "-j8"], check=True)
    return _lib.load()


def test_c_entry_points_refuse_bad_arguments(lib):
    one = ctypes.c_void_p(8)  # never dereferenced: every refusal comes before any device call
    for args in [(0, 1, 1, 1, one, one, one), (1, 0, 1, 1, one, one, one), (1, 1, 0, 1, one, one, one),
                 (1, 1, 1, 0, one, one, one), (1, 1, 1, -4, one, one, one), (1, 1, 1, 1, None, one, one),
                 (1, 1, 1, 1, one, None, one), (1, 1, 1, 1, one, one, None)]:
        assert lib.avr_conv_source(*args, None) == 1001, args
        assert b"avr_conv_source" in lib.avr_last_error()
    nb = ctypes.c_int64(-1)
    assert lib.avr_sosfiltfilt_workspace(3, 28, 4, 27, ctypes.byref(nb)) == 0
    assert nb.value == 3 * (28 + 54) * 8
    for args in [(0, 28, 4, 27), (3, 27, 4, 27), (3, 28, 0, 27), (3, 28, 9, 27), (3, 28, 4, -1), (-1, 28, 4, 27)]:
        assert lib.avr_sosfiltfilt_workspace(*args, ctypes.byref(nb)) == 1001, args
    assert lib.avr_sosfiltfilt_workspace(3, 28, 4, 27, None) == 1001
    ok = (3, 28, 4, 27, one, one, one, 0, one, 3, one, nb.value)
    for i, bad in [(0, 0), (1, 27), (2, 0), (4, None), (5, None), (6, None), (7, 1), (8, None), (9, 2),
                   (10, None), (11, 8)]:
        args = list(ok)
        args[i] = bad
        assert lib.avr_sosfiltfilt(*args, None) == 1001, (i, bad)
        assert b"avr_sosfiltfilt" in lib.avr_last_error()


def test_call_path_imports_no_scipy():
    """Importing the package and resolving everything convolve_source and
    zero_phase_sos touch on the host (tables, zi, padlen) loads no scipy."""
    code = (
        "import sys, numpy as np\n"
        "import avr_amd\n"
        "from avr_amd import auralize\n"
        "sos = np.array([[0.2, 0.4, 0.2, 1.0, -0.3, 0.1]])\n"
        "auralize.sosfilt_zi(sos); auralize.sos_padlen(sos)\n"
        "for f in (auralize.convolve_source, auralize.zero_phase_sos):\n"
        "    try:\n"
        "        f(avr_amd.auralize.torch.zeros(2, 64), sos)\n"
        "    except RuntimeError:\n"
        "        pass\n"
        "assert not [m for m in sys.modules if m == 'scipy' or m.startswith('scipy.')], 'scipy imported'\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    src = open(os.path.join(ROOT, "avr_amd", "auralize.py")).read()
    assert src.count("import scipy") + src.count("from scipy") == 1  # butter_bandpass_sos alone


def test_butter_bandpass_sos_is_scipys():
    signal = pytest.importorskip("scipy.signal")
    for (lo, hi), want in zip(ac.BANDS, ac.load("bp_block")["sos"]):
        got = auralize.butter_bandpass_sos(lo, hi, ac.FS, 4)
        assert np.allclose(got, want, rtol=1e-12, atol=0.0)
        assert np.array_equal(got, signal.butter(4, [lo, hi], btype="band", fs=ac.FS, output="sos"))
