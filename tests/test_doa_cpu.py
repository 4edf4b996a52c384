"""CPU: the DoA fixtures (tools/gen_doa_golden.py, written from the
reference's plot_eval.py / whitenoise_bandpass_doa.py), the float64
restatements in tests/doa_cases.py that the GPU tests compare against, and the
argument checks of avr_amd.doa and its C entry points.  No GPU."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import doa_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    with np.load(os.path.join(dc.GOLDEN, f"{name}.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def frames64():
    """The fp64 restatement of every scene and algorithm, computed once."""
    out = {}
    for name, L, nfft, hop, win, fr, G, nf, kind, seed in dc.SCENES:
        y, theta, H = dc.scene(name)
        for algo in dc.ALGOS:
            out[name, algo] = (y, theta, H) + dc.restate_frames(y, L, H, nfft, hop, win, algo, freq_range=fr)
    return out


def test_fixture_sizes_and_inputs_regenerate():
    files = sorted(os.listdir(dc.GOLDEN))
    assert files == sorted([f"das_{c[0]}.npz" for c in dc.DAS_CASES] + ["circ_stats.npz", "timing.npz"])
    for f in files:
        assert os.path.getsize(os.path.join(dc.GOLDEN, f)) <= 256 * 1024, f
    for name, N, T, fs, kind, pdt in dc.DAS_CASES:
        fx = _load(f"das_{name}")
        d = dc.das_inputs(name, int(fx["seed"]))
        assert d["pred_sig"].shape == (N, T // 2 + 1) and d["pred_sig"].dtype == np.complex64
        assert d["position_rx"].dtype == np.dtype(pdt)
        assert np.array_equal(dc.digest(d["pred_sig"], d["ori_sig"], d["position_rx"], d["position_tx"]),
                              fx["digest"]), name
        assert json.loads(str(fx["meta"]))["seed"] == int(fx["seed"])
    cs = _load("circ_stats")
    for i, nm in enumerate(cs["names"]):
        a = dc.circ_angles(str(nm))
        assert np.array_equal(cs["digest"][i], [len(a), sum(a), sum(v * v for v in a)])


@pytest.mark.parametrize("name", [c[0] for c in dc.DAS_CASES])
def test_das_restatement_reproduces_the_reference(name):
    """argmax values exactly; soft-argmax within twice the stored e_ref (e_ref
    IS the largest such distance, so this also pins the fixture to the
    restatement it was checked with); true_deg to 1e-9."""
    _, N, T, fs, kind, pdt = dc.DAS[name]
    fx = _load(f"das_{name}")
    res, power = dc.restate_das(dc.das_inputs(name, int(fx["seed"])), fs=fs)
    G = N // dc.MICS
    assert power.shape == (G, 2, 360)
    assert dc.peak_margin(power).min() >= 1e-4
    for k in dc.DAS_KEYS:
        got, want = np.array(res[dc.DAS_METHODS[1]][k]), fx[f"m1_{k}"]
        print(name, "argmax", k, got, want)
        assert got.shape == (G,)
        if k == "true_deg" or k.endswith("true_error"):
            assert np.abs(got - want).max() <= 1e-9
        else:
            assert np.array_equal(got, want), k
    bar = 2 * float(fx["e_ref"])
    for k in ("pred_deg", "gt_deg"):
        dist = np.abs(np.array(res[dc.DAS_METHODS[0]][k]) - fx[f"m0_{k}"]).max()
        print(name, "soft", k, "distance", dist, "bar", bar)
        assert dist <= bar
    if kind == "burst":  # a sharp peak: soft equals arg
        assert np.array_equal(fx["m0_pred_deg"], fx["m1_pred_deg"])
    else:                # a flat power: the soft-argmax is fractional
        assert np.any(fx["m0_pred_deg"] != np.round(fx["m0_pred_deg"]))


def test_circular_statistics_restatement_equals_the_reference():
    cs = _load("circ_stats")
    assert [str(n) for n in cs["names"]] == [c[0] for c in dc.CIRC_CASES]
    for i, nm in enumerate(cs["names"]):
        got = np.array(dc.restate_circ_stats(dc.circ_angles(str(nm))))
        want = cs["stats"][i]
        print(nm, got, want)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        assert np.allclose(got, want, rtol=0, atol=1e-12, equal_nan=True)
    assert np.isnan(cs["stats"][0]).all() and cs["n"][0] == 0
    wrap = cs["stats"][[str(n) for n in cs["names"]].index("wrap")]
    assert wrap[0] < 20 or wrap[0] > 340           # the mean lies at the wrap, not near 180
    assert cs["stats"][-1][1] > 0.7                # the uniform list: R near 0


@pytest.mark.parametrize("name", [s[0] for s in dc.SCENES])
def test_frames_restatement_on_the_scenes(name, frames64):
    """Dry scenes: theta recovered within 1 degree (circular) by all three
    algorithms; the J = 0 setting is invalid; and the margin rule the GPU test
    relies on holds for the restatement alone: at most 5 % of a scene's frames
    have an fp64 peak that stands less than 4 bars above a 1-degree neighbour
    (bar = max(8 e32, 1e-6), e32 the complex64 evaluation's distance from fp64
    on the spectrum divided by its maximum)."""
    _, L, nfft, hop, win, fr, G, nf, kind, seed = dc.SCENE[name]
    for algo in dc.ALGOS:
        y, theta, H, est, valid, spec = frames64[name, algo]
        assert (y.shape[2] - L) % H != 0 and est.shape == (G, nf)
        if name == "too_short":
            assert not valid.any() and (est == -1).all() and (spec == 0).all()
            continue
        assert valid.all()
        e32, v32, s32 = dc.restate_frames(y, L, H, nfft, hop, win, algo, freq_range=fr, dtype=np.float32)
        err = np.abs(spec / spec.max(-1, keepdims=True) - s32 / s32.max(-1, keepdims=True)).max()
        bar = max(8 * err, 1e-6)
        outside = (dc.frames_margin(spec) <= 4 * bar).mean()
        terr = dc.circ_dist(est, theta[:, None]).max()
        print(name, algo, "e32 %.2e outside %.3f truth error %.2f deg" % (err, outside, terr))
        assert outside <= 0.05
        assert np.array_equal(est, e32)
        if kind == "dry":
            assert terr <= 1.0


def test_bins_and_snapshot_counts():
    assert dc.doa_bins(256, 16000, (700.0, 3100.0)) == (11, 39)
    assert dc.doa_bins(512, 16000, (500.0, 4000.0)) == (16, 112)
    assert dc.doa_bins(256, 16000, (0.0, 1e9)) == (0, 129)
    from avr_amd.doa import doa_bins

    for nfft, fr in ((256, (700.0, 3100.0)), (1024, (500.0, 4000.0)), (256, (-5.0, 1e9)), (512, (7900.0, 8100.0))):
        assert doa_bins(nfft, 16000, fr) == dc.doa_bins(nfft, 16000, fr)


def test_cpu_tensors_raise():
    import avr_amd
    from avr_amd import doa

    assert avr_amd.das_doa is doa.das_doa and avr_amd.doa_frames is doa.doa_frames
    assert avr_amd.frame_stats is doa.frame_stats and avr_amd.das_doa_dump is doa.das_doa_dump
    spec = torch.zeros(8, 257, dtype=torch.complex64)
    pos = torch.zeros(8, 3)
    with pytest.raises(RuntimeError, match="HIP tensor"):
        doa.das_doa(spec, spec, pos, pos)
    with pytest.raises(RuntimeError, match="HIP tensor"):
        doa.doa_frames(torch.zeros(1, 8, 4000), 1600, 400, 512, 256)
    with pytest.raises(RuntimeError, match="HIP tensor"):
        doa.frame_stats(torch.zeros(1, 4, dtype=torch.int32), torch.ones(1, 4, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="HIP device"):
        doa.das_doa_dump(dc.das_inputs("g1", 1000), device="cpu")


def test_c_entry_points_refuse_bad_arguments_without_a_gpu():
    from avr_amd import _lib

    lib = _lib.load()
    nb = ctypes.c_int64(-1)
    assert lib.avr_doa_das_workspace(18, 512, 360, ctypes.byref(nb)) == 0
    tiles = (257 + 15) // 16
    assert nb.value == 2 * 18 * 8 * 257 * 16 + 2 * 18 * tiles * 360 * 8
    for args in ((0, 512, 360), (1, 511, 360), (1, 4096, 360), (1, 512, 0), (1, 512, 2000)):
        assert lib.avr_doa_das_workspace(*args, ctypes.byref(nb)) == 1001, args
        assert b"avr_doa_das" in lib.avr_last_error()
    assert lib.avr_doa_das_workspace(1, 512, 360, None) == 1001
    p = ctypes.c_void_p(16)  # never dereferenced: every call below is refused before any device call
    assert lib.avr_doa_das(1, 512, 512, 360, None, p, p, p, p, 100.0, p, p, 0, p, p, 1 << 30, None) == 1001
    assert lib.avr_doa_das(1, 512, 512, 360, p, p, p, p, p, 100.0, p, p, 1, p, p, 1 << 30, None) == 1001
    assert lib.avr_doa_das(1, 512, 512, 360, p, p, p, p, p, 100.0, p, p, 0, p, p, 16, None) == 1001
    assert b"workspace too small" in lib.avr_last_error()

    def frames(G=1, n=4000, L=1600, H=400, nf=7, nfft=512, hop=256, k_lo=16, K=112, algo=2, floor=1e-4,
               y=p, dt=0):
        return lib.avr_doa_frames(G, n, L, H, nf, nfft, hop, k_lo, K, algo, floor, y, dt, p, p, p, p, p, None, None)

    for kw in (dict(G=0), dict(nf=8), dict(L=5000), dict(nfft=4096), dict(nfft=1), dict(hop=0), dict(K=0),
               dict(k_lo=200), dict(algo=3), dict(floor=0.0), dict(y=None), dict(dt=1), dict(H=0)):
        assert frames(**kw) == 1001, kw
        assert b"avr_doa_frames" in lib.avr_last_error()
    assert lib.avr_doa_frame_stats(0, 4, p, p, p, p, p, None) == 1001
    assert lib.avr_doa_frame_stats(1, 4, None, p, p, p, p, None) == 1001
    assert lib.avr_doa_frame_stats(1, 4, p, p, None, p, p, None) == 1001
    assert lib.avr_doa_frame_stats(1, 4, p, p, p, None, p, None) == 1001


def test_call_path_imports_no_scipy():
    code = ("import sys; import avr_amd; from avr_amd import doa; "
            "doa._das_tables; doa.doa_bins(512, 16000, (500.0, 4000.0)); "
            "assert not any(m == 'scipy' or m.startswith('scipy.') for m in sys.modules), 'scipy imported'")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT,
                   env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")))
