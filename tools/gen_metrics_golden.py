"""Golden vectors for the validation metrics from the REAL reference
`utils/metric.py` (build container only; /root/reference is absent on the
GPU box).

auraloss (the reference's MR-STFT dependency) is not installed.  Its import
is satisfied by a placeholder module whose `MultiResolutionSTFTLoss` returns
NaN: the multi_stft metric is never stored (it stays "parity unpinned" like
the criterion's term).  The six other metrics -- Angle,
Amplitude, Envelope, T60, EDT, C50 -- and both energy curves run the
reference's own numpy / scipy code, on fp32 arrays as the runner passes them.

Fixtures hold data only: seeds, shapes, fs, the expected metrics, per-row
T60 / EDT, the energy curves and a digest of the inputs (tests regenerate
the inputs from the seeds).  `meta` also records the reference's CPU
milliseconds per call on the machine that wrote the fixture.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_metrics_golden.py
"""
from __future__ import annotations

import json
import os
import sys
import time
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.dont_write_bytecode = True
REF = "/root/reference"

sys.path.insert(0, os.path.join(REPO, "tests"))
from metrics_cases import CASES, GOLDEN, WINDOW, digest, irs  # noqa: E402

METRICS = ("angle", "amplitude", "envelope", "t60", "edt", "c50")


def _reference_metric():
    class _NoMRSTFT(torch.nn.Module):
        """auraloss is absent: the term it computes is never stored."""

        def __init__(self, *a, **k):
            super().__init__()

        def forward(self, x, y):
            return torch.tensor(float("nan"))

    aura = types.ModuleType("auraloss")
    aura.freq = types.SimpleNamespace(MultiResolutionSTFTLoss=_NoMRSTFT)
    sys.modules["auraloss"] = aura
    sys.path.insert(0, REF)
    from utils import metric  # noqa: E402  (the reference's file)

    return metric


def main():
    metric = _reference_metric()
    os.makedirs(GOLDEN, exist_ok=True)
    for name, B, n, fs, seed, noise, delay in CASES:
        ori, pred = irs(B, n, seed, noise, delay)
        with np.errstate(all="ignore"):
            out = metric.metric_cal(ori, pred, fs=fs, window=WINDOW)  # raises if the reference refuses the case
            times = []
            for _ in range(9):
                t0 = time.perf_counter()
                metric.metric_cal(ori, pred, fs=fs, window=WINDOW)
                times.append((time.perf_counter() - t0) * 1e3)
            ms = sorted(times)[len(times) // 2]  # median of nine calls
        ori_energy, pred_energy = out[7], out[8]
        t60_o, edt_o = metric.t60_EDT_cal(ori_energy, fs=fs)
        t60_p, edt_p = metric.t60_EDT_cal(pred_energy, fs=fs)
        z = {
            "meta": json.dumps(dict(name=name, B=B, n=n, fs=fs, seed=seed, noise=noise, delay=delay,
                                    window=WINDOW, metrics=list(METRICS), ref_cpu_ms=round(ms, 3),
                                    numpy=np.__version__,
                                    source="utils/metric.py (reference), multi_stft not stored")),
            "metrics": np.array([float(x) for x in out[:6]], np.float64),
            "t60_rows": np.stack([t60_o, t60_p]).astype(np.float64),
            "edt_rows": np.stack([edt_o, edt_p]).astype(np.float64),
            "ori_energy": ori_energy.astype(np.float32),
            "pred_energy": pred_energy.astype(np.float32),
            "digest": digest(ori, pred),
        }
        np.savez_compressed(os.path.join(GOLDEN, f"metrics_{name}.npz"), **z)
        print(f"metrics_{name}: {np.array2string(z['metrics'], precision=6)} ref {ms:.1f} ms "
              f"input dtype {ori.dtype}")


if __name__ == "__main__":
    main()
