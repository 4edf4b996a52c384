"""CPU: the validation metrics' C-ABI refuses bad arguments before any device
call, and the committed fixtures (tests/golden/metrics, from the reference's
utils/metric.py) parse and regenerate from their seeds."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

from avr_amd import _lib
import avr_amd.metrics as metrics
from metrics_cases import CASES, GOLDEN, WINDOW, digest, irs, load, restate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = 1001


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "avr_amd", "csrc"), "-j8"], check=True)
    return _lib.load()


def _metrics(lib, B=2, n=1022, fs=24000.0, s50=1200, window=32, null=None, ws_bytes=1 << 30):
    """avr_metrics with placeholder (never dereferenced) pointers: every call
    here must be refused while the arguments are checked."""
    ptrs = [ctypes.c_void_p(0x1000)] * 10
    if null is not None:
        ptrs[null] = None
    return lib.avr_metrics(B, n, fs, s50, window, *ptrs, ws_bytes, None)


def test_workspace_size_and_shape_checks(lib):
    out = ctypes.c_int64(0)
    assert lib.avr_metrics_workspace(2, 1022, ctypes.byref(out)) == 0
    K = 1022 // 2 + 1
    assert out.value >= 2 * 2 * K * 8 + 2 * 2 * 1022 * 4  # half spectra and envelopes
    assert out.value % 16 == 0
    big = ctypes.c_int64(0)
    assert lib.avr_metrics_workspace(4, 4094, ctypes.byref(big)) == 0 and big.value > out.value
    assert lib.avr_metrics_workspace(2, 1022, None) == E_ARG
    assert b"null" in lib.avr_last_error()
    for n, word in ((1021, b"even"), (256, b"256 < n"), (254, b"256 < n"), (12290, b"12288")):
        assert lib.avr_metrics_workspace(2, n, ctypes.byref(out)) == E_ARG, n
        assert word in lib.avr_last_error(), (n, lib.avr_last_error())
    assert lib.avr_metrics_workspace(0, 1022, ctypes.byref(out)) == E_ARG
    assert lib.avr_metrics_workspace(257, 1022, ctypes.byref(out)) == E_ARG


def test_metrics_refuses_bad_arguments_without_gpu(lib):
    for i in range(10):
        assert _metrics(lib, null=i) == E_ARG, i
        assert b"null pointer" in lib.avr_last_error()
    assert _metrics(lib, n=1021) == E_ARG and b"even" in lib.avr_last_error()
    assert _metrics(lib, n=256) == E_ARG and b"256 < n" in lib.avr_last_error()
    assert _metrics(lib, n=12290) == E_ARG and b"12288" in lib.avr_last_error()
    assert _metrics(lib, window=1023) == E_ARG and b"window" in lib.avr_last_error()
    assert _metrics(lib, window=0) == E_ARG and b"window" in lib.avr_last_error()
    assert _metrics(lib, fs=0.0) == E_ARG and b"fs" in lib.avr_last_error()
    assert _metrics(lib, fs=float("nan")) == E_ARG and b"fs" in lib.avr_last_error()
    assert _metrics(lib, s50=-1) == E_ARG and b"s50" in lib.avr_last_error()
    assert _metrics(lib, B=0) == E_ARG
    assert _metrics(lib, ws_bytes=64) == E_ARG and b"workspace too small" in lib.avr_last_error()


def test_python_entry_points_need_hip_tensors():
    import torch

    x = torch.zeros(2, 1022)
    for fn in (metrics.metric_cal, metrics.metric_rows):
        with pytest.raises(RuntimeError, match="HIP tensor"):
            fn(x, x)
    assert len(metrics.ROW_COLS) == 9
    with pytest.raises(RuntimeError, match="no batch"):
        metrics.MetricAccumulator().result()


def test_call_path_imports_neither_scipy_nor_numpy():
    import ast

    tree = ast.parse(open(os.path.join(ROOT, "avr_amd", "metrics.py")).read())
    mods = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            mods |= {a.name.split(".")[0] for a in node.names}
        elif isinstance(node, ast.ImportFrom) and node.level == 0:
            mods.add(node.module.split(".")[0])
    assert mods == {"__future__", "ctypes", "torch"}, mods


def test_every_fixture_parses():
    files = sorted(f for f in os.listdir(GOLDEN) if f.endswith(".npz"))
    assert files == sorted(f"metrics_{c[0]}.npz" for c in CASES)
    for name, B, n, fs, seed, noise, delay in CASES:
        z = load(name)
        meta = json.loads(str(z["meta"]))
        assert (meta["name"], meta["B"], meta["n"], meta["fs"], meta["seed"]) == (name, B, n, fs, seed)
        assert meta["noise"] == noise and meta["delay"] == delay and meta["window"] == WINDOW
        assert meta["ref_cpu_ms"] > 0
        assert z["metrics"].shape == (6,) and z["metrics"].dtype == np.float64
        assert z["ori_energy"].shape == (B, n) and z["pred_energy"].shape == (B, n)
        assert z["t60_rows"].shape == (2, B) and z["edt_rows"].shape == (2, B)
        # C50 is NaN exactly where the IR ends before the 50 ms split
        assert bool(np.isnan(z["metrics"][5])) == (n <= int(0.05 * fs))
        assert np.isfinite(z["metrics"][:5]).all()
        assert np.all(z["ori_energy"][:, 0] == 0.0)
        assert os.path.getsize(os.path.join(GOLDEN, f"metrics_{name}.npz")) < 1 << 20


def test_fixture_inputs_regenerate_from_their_seeds():
    for name, B, n, fs, seed, noise, delay in CASES:
        ori, pred = irs(B, n, seed, noise, delay)
        assert ori.dtype == np.float32 and ori.shape == (B, n)
        assert np.all(ori[:, :delay] == 0.0) and np.all(pred[:, :delay] == 0.0)
        np.testing.assert_allclose(digest(ori, pred), load(name)["digest"], rtol=1e-4, atol=1e-7)


def test_restatement_is_pinned_to_the_reference_fixtures():
    """metrics_cases.restate (float64, numpy alone) against the reference's
    stored values: 1e-6 relative (the reference transforms in fp32; its own
    fp32-input and fp64-input results differ by <= 5e-7) and 1e-3 dB on the
    curves above -60 dB: the reference's curve is a sequential fp32 sum of up
    to 4094 terms, whose rounding alone can reach n 2^-24 relative, i.e.
    4094 * 6e-8 * 10 / ln 10 = 1.06e-3 dB, the bar the GPU curves are held to."""
    for name, B, n, fs, seed, noise, delay in CASES:
        z = load(name)
        ori, pred = irs(B, n, seed, noise, delay)
        angle, amp, env, oe, pe = restate(ori, pred, fs, WINDOW)
        for got, ref in zip((angle, amp, env), z["metrics"][:3]):
            assert abs(got - ref) <= 1e-6 * abs(ref), (name, got, ref)
        for got, ref in ((oe, z["ori_energy"]), (pe, z["pred_energy"])):
            assert np.abs(got - ref)[ref > -60.0].max() <= 1e-3, name
