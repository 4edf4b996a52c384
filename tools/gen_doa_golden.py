"""Golden vectors for the DoA evaluation from the REAL reference
`plot_eval.py` (run_delay_and_sum_on_npz) and `whitenoise_bandpass_doa.py`
(circ_stats_deg), on the build machine only (/root/reference is absent on the
GPU box).

pyroomacoustics, librosa, matplotlib and tensorboard are not installed; their
imports are satisfied by empty placeholder modules, and none of the functions
called here touches them.  The frame estimators (pyroomacoustics' MUSIC /
NormMUSIC / SRP) therefore have no reference fixture: their contract is the
definition restated in tests/doa_cases.py.

Fixtures hold data only: seeds, shapes, digests of the inputs (tests
regenerate the inputs from the seeds) and the reference's returned lists as
arrays.  For every NormDAS case the float64 restatement (doa_cases.restate_das)
is evaluated too: a seed is kept only if every group's fp64 power peak stands
at least 1e-4 above both neighbours, and `e_ref`, the largest distance in
degrees between the reference's own fp32 soft-argmax and the fp64 one, is
stored.  Files regenerate bit-identically except `timing.npz`.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_doa_golden.py [--no-timing]
"""
from __future__ import annotations

import io
import json
import os
import pickle
import sys
import tempfile
import time
import types
import zipfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.dont_write_bytecode = True
REF = "/root/reference"

sys.path.insert(0, os.path.join(REPO, "tests"))
import doa_cases as dc  # noqa: E402


def _reference():
    for name in ("pyroomacoustics", "librosa", "matplotlib", "matplotlib.pyplot", "tensorboard",
                 "tensorboard.backend", "tensorboard.backend.event_processing",
                 "tensorboard.backend.event_processing.event_accumulator", "pandas", "yaml"):
        if name not in sys.modules:
            try:
                __import__(name)
            except ImportError:
                sys.modules[name] = types.ModuleType(name)  # never touched
    sys.path.insert(0, REF)
    import plot_eval  # noqa: E402  (the reference's files)
    import whitenoise_bandpass_doa as wn  # noqa: E402

    return plot_eval, wn


def save(name, **arrays):
    """np.savez_compressed with a fixed timestamp and member order."""
    path = os.path.join(dc.GOLDEN, f"{name}.npz")
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())
    kb = os.path.getsize(path) / 1024
    assert kb <= 256, (name, kb)
    print(f"{name}: {kb:.1f} KB")


def main():
    import torch

    plot_eval, wn = _reference()
    os.makedirs(dc.GOLDEN, exist_ok=True)
    versions = dict(numpy=np.__version__, torch=torch.__version__.split("+")[0])

    # ---- NormDAS: run_delay_and_sum_on_npz on synthetic dumps
    with tempfile.TemporaryDirectory() as tmp:
        for ci, (name, N, T, fs, kind, pdt) in enumerate(dc.DAS_CASES):
            for seed in range(1000 * (ci + 1), 1000 * (ci + 1) + 200):
                d = dc.das_inputs(name, seed)
                res64, power = dc.restate_das(d, fs=fs)
                if dc.peak_margin(power).min() >= 1e-4:
                    break
            else:
                raise RuntimeError(f"{name}: no seed with a 1e-4 peak margin")
            npz = os.path.join(tmp, f"{name}.npz")
            np.savez(npz, **d)
            pkl = os.path.join(tmp, f"{name}.pkl")
            ret = plot_eval.run_delay_and_sum_on_npz(npz, fs=fs, save_path=pkl)
            with open(pkl, "rb") as f:
                res = pickle.load(f)
            assert res == ret
            arrays = {}
            for mi, m in enumerate(dc.DAS_METHODS):
                for k in dc.DAS_KEYS:
                    arrays[f"m{mi}_{k}"] = np.array([float(v) for v in res[m][k]], np.float64)
            soft = dc.DAS_METHODS[0]
            e_ref = max(np.abs(np.array(res[soft][k], np.float64) - np.array(res64[soft][k])).max()
                        for k in ("pred_deg", "gt_deg"))
            G = N // dc.MICS
            assert all(len(v) == G for v in arrays.values())
            print(f"  {name}: seed {seed}, G {G}, margin {dc.peak_margin(power).min():.2e}, e_ref {e_ref:.3e} deg")
            save(f"das_{name}",
                 meta=json.dumps(dict(name=name, N=N, T=T, fs=fs, kind=kind, positions=pdt, seed=seed, **versions,
                                      source="plot_eval.py run_delay_and_sum_on_npz (reference)")),
                 seed=np.int64(seed), e_ref=np.float64(e_ref), margin=np.float64(dc.peak_margin(power).min()),
                 digest=dc.digest(d["pred_sig"], d["ori_sig"], d["position_rx"], d["position_tx"]), **arrays)

    # ---- circular statistics: circ_stats_deg
    names, stats, lens = [], [], []
    for name, n, seed, kind in dc.CIRC_CASES:
        a = dc.circ_angles(name)
        names.append(name)
        lens.append(len(a))
        # doa_sample_from_frames:162-164: an empty list never reaches circ_stats_deg
        stats.append(wn.circ_stats_deg(a) if len(a) else (np.nan, np.nan, np.nan))
    save("circ_stats", meta=json.dumps(dict(**versions, source="whitenoise_bandpass_doa.py circ_stats_deg (reference)")),
         names=np.array(names), n=np.array(lens), stats=np.array(stats, np.float64),
         digest=np.array([[len(a), sum(a), sum(v * v for v in a)] for a in map(dc.circ_angles, names)], np.float64))

    if "--no-timing" in sys.argv:
        return
    # ---- context for tools/bench_doa.py: the fp64 numpy restatement of ONE
    # group of the benchmark's shape (8 s at 16 kHz, L 1600, H 400, nfft 512,
    # hop 256, NormMUSIC), and the reference's NormDAS on 18 groups, T = 1600
    rng = np.random.default_rng(0)
    y = rng.standard_normal((1, 8, 8 * dc.FS)).astype(np.float32)
    t0 = time.perf_counter()
    est, valid, _ = dc.restate_frames(y, 1600, 400, 512, 256, "hann", "NormMUSIC")
    t_frames = (time.perf_counter() - t0) * 1e3
    with tempfile.TemporaryDirectory() as tmp:
        spec = np.fft.rfft(rng.standard_normal((144, 1600)), axis=-1).astype(np.complex64)
        pos = rng.standard_normal((144, 3)).astype(np.float32)
        npz = os.path.join(tmp, "b.npz")
        np.savez(npz, pred_sig=spec, ori_sig=spec[::-1].copy(), position_rx=pos, position_tx=pos[::-1].copy())
        t0 = time.perf_counter()
        plot_eval.run_delay_and_sum_on_npz(npz)
        t_das = (time.perf_counter() - t0) * 1e3
    names = ["restate_frames_1group_8s_L1600_H400_nfft512_NormMUSIC", "reference_das_G18_T1600"]
    save("timing", meta=json.dumps(dict(cpus=os.cpu_count(), **versions, frames=int(est.shape[1]),
                                        note="CPU milliseconds; this file is a measurement and does not "
                                             "regenerate bit-identically")),
         names=np.array(names), ms=np.array([t_frames, t_das]))
    print(f"  {names[0]}: {t_frames:.1f} ms ({est.shape[1]} frames)\n  {names[1]}: {t_das:.1f} ms")


if __name__ == "__main__":
    main()
