"""CPU: the host side of the time-varying convolution: the
float64 restatement the GPU tests lean on, `trajectory_weights`, the
condition on the sequential fp32 form that keeps the GPU bar tight, and the
argument refusals of `avr_conv_trajectory`, which need no device.

Every test prints its figures before it asserts.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import trajectory_cases as tc
from avr_amd import _lib, auralize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------- the restatement

@pytest.mark.parametrize("name", tc.NAMES)
def test_overlap_add_equals_the_per_sample_form(name):
    ir, x = tc.inputs(name)
    *_, hop, fade = tc.CASES[name]
    y64, _ = tc.reference(name)
    P, C, Nh, L = ir.shape + x.shape
    assert y64.shape == (C, L + Nh - 1)
    d = tc.direct64(ir, x, hop, fade)
    err = np.abs(d - y64).max() / np.abs(y64).max()
    print(f"{name}: overlap-add vs per-sample loop {err:.2e}")
    assert err <= 1e-12


@pytest.mark.parametrize("name", tc.NAMES)
def test_sequential_fp32_is_close_to_float64(name):
    """e32 <= 1e-5 keeps the GPU bar max(8 e32, 1e-6) three decades under the
    1e-2 a wrong point or weight costs."""
    _, e32 = tc.reference(name)
    print(f"{name}: e32 = {e32:.2e}")
    assert e32 <= 1e-5


def test_a_wrong_point_is_far_outside_the_bar():
    """What the bar must not hide: every sample played through the neighbouring point's IR."""
    name = "full_fade_group"
    ir, x = tc.inputs(name)
    *_, hop, fade = tc.CASES[name]
    y64, e32 = tc.reference(name)
    wrong = tc.restate64(np.roll(ir, 1, axis=0), x, hop, fade)
    err = np.abs(wrong - y64).max() / np.abs(y64).max()
    print(f"{name}: points rolled by one {err:.2e} against the bar {max(8 * e32, 1e-6):.2e}")
    assert err >= 1e-2


# ------------------------------------------------------------------ weights

WEIGHT_SHAPES = [(P, L, hop, fade) for P, _, _, L, hop, fade in tc.CASES.values()] + [
    (1, 7, 1, 1), (3, 10, 1, 1), (3, 10, 1, 0), (2, 9, 4, 4), (5, 64, 16, 7), (7, 30, 100, 100)]


@pytest.mark.parametrize("P,L,hop,fade", WEIGHT_SHAPES)
def test_trajectory_weights(P, L, hop, fade):
    w = auralize.trajectory_weights(P, L, hop, fade)
    assert isinstance(w, np.ndarray) and w.dtype == np.float32 and w.shape == (P, L)
    assert np.array_equal(w, tc.weights(P, L, hop, fade))
    assert (w >= 0).all()
    assert ((w != 0).sum(axis=0) <= 2).all()
    col = w.astype(np.float64).sum(axis=0)
    print(f"P={P} L={L} hop={hop} fade={fade}: max |column sum - 1| = {np.abs(col - 1).max():.2e}")
    assert (np.abs(col - 1) <= 2.0 ** -24).all()
    if fade == 0:
        assert np.isin(w, (0.0, 1.0)).all()
    hold = (P - 1) * hop
    if hold < L:
        assert (w[P - 1, hold:] == 1).all() and (w[:P - 1, hold:] == 0).all()
    # the definition, sample by sample
    for m in range(L):
        q = min(m // hop, P - 1)
        j = m - ((q + 1) * hop - fade)
        want = np.zeros(P, np.float32)
        if q + 1 < P and j >= 0:
            u = np.float32(2 * j + 1) / np.float32(2 * fade)
            want[q + 1], want[q] = u, np.float32(1) - u
        else:
            want[q] = 1
        assert np.array_equal(w[:, m], want), m


def test_trajectory_weights_refuses_bad_arguments():
    for args in [(0, 5, 1, 0), (1, 0, 1, 0), (1, 5, 0, 0), (1, 5, 2, 3), (1, 5, 2, -1), (2, 5, 1 << 23, 1 << 23)]:
        with pytest.raises(ValueError):
            auralize.trajectory_weights(*args)


# --------------------------------------------------- refusals without a device

def test_cpu_tensors_raise():
    ir, x = torch.zeros(2, 3, 8), torch.zeros(16)
    with pytest.raises(RuntimeError, match="HIP tensor"):
        auralize.convolve_trajectory(ir, x, 4)
    with pytest.raises(RuntimeError, match="HIP tensor"):
        auralize.synth_trajectory(torch.zeros(2, 3, 5, dtype=torch.complex64), x, 4)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "avr_amd", "csrc"), "-j8"], check=True)
    return _lib.load()


def test_c_entry_point_refuses_bad_arguments(lib):
    one = ctypes.c_void_p(8)  # never dereferenced: every refusal comes before any device call
    ok = [2, 3, 8, 100, 10, 4, one, one, one]  # P, C, Nh, L, hop, fade, h, x, y
    bad = [(0, 0), (0, -1), (1, 0), (1, -3), (2, 0), (2, -8), (3, 0), (3, -100), (4, 0), (4, -10),
           (5, -1), (5, 11), (6, None), (7, None), (8, None),
           (1, 65535 * 32 + 1),       # channel tiles beyond the grid
           (3, (1 << 40) * 512 + 1)]  # output blocks beyond the grid
    for i, v in bad:
        args = list(ok)
        args[i] = v
        assert lib.avr_conv_trajectory(*args, None) == 1001, (i, v)
        assert b"avr_conv_trajectory" in lib.avr_last_error(), (i, v)
    big = list(ok)
    big[4], big[5] = 1 << 24, 1 << 23  # fade <= hop but fade >= 2^23
    assert lib.avr_conv_trajectory(*big, None) == 1001
    assert b"avr_conv_trajectory" in lib.avr_last_error()


def test_binding_matches_the_header():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "avr_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+avr_conv_trajectory\s*\(([^)]*)\)\s*;", text)
    assert m, "avr_conv_trajectory is not declared in include/avr_hip.h"
    ctype = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}
    want = []
    for arg in m.group(1).split(","):
        arg = " ".join(arg.split())
        want.append(ctypes.c_void_p if "*" in arg else ctype[arg.replace("const ", "").split(" ")[0]])
    names = [" ".join(a.split()).replace("*", " ").split()[-1] for a in m.group(1).split(",")]
    assert names == ["P", "C", "Nh", "L", "hop", "fade", "h", "x", "y", "stream"]
    res, args = _lib._SIGS["avr_conv_trajectory"]
    assert res is ctypes.c_int and args == want
