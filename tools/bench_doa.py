"""Times the DoA evaluation on an MI355X with HIP events around whole calls
(recorded, not gated): `das_doa` at G = 18 groups and T = 1600, and
`doa_frames` at G = 18, 8 s at 16 kHz, L = 1600, H = 400, nfft = 512,
hop = 256 for the three algorithms (NormMUSIC is the reference's default),
plus `frame_stats` on its result.

Each call is warmed up, then timed as one event pair around `reps` calls
(median of 5 such windows).  For context, tests/golden/doa/timing.npz holds
the CPU milliseconds of the float64 numpy restatement for ONE group of the
same `doa_frames` shape and of the reference's own NormDAS function on 18
groups, on the machine that wrote the fixtures.

    python tools/bench_doa.py --out profiles/doa_gpu.json
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

FS = 16000


def _time(fn, reps, rounds=5):
    fn()
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / reps)
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "doa_gpu.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_doa: no HIP device (nothing is measured on the CPU)")
    from avr_amd import doa

    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    res = dict(device=torch.cuda.get_device_name(0), fs=FS, das=[], frames=[])

    G, T = 18, 1600
    spec = lambda: torch.from_numpy(np.fft.rfft(rng.standard_normal((G * 8, T)), axis=-1).astype(np.complex64)).to(dev)
    pred, ori = spec(), spec()
    rx = torch.from_numpy(rng.standard_normal((G * 8, 3)).astype(np.float32)).to(dev)
    tx = torch.from_numpy(rng.standard_normal((G * 8, 3)).astype(np.float32)).to(dev)
    med, lo, hi = _time(lambda: doa.das_doa(pred, ori, rx, tx), 20)
    row = dict(call="das_doa", G=G, T=T, n_fft=512, ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4))
    res["das"].append(row)
    print(json.dumps(row), flush=True)

    L, H, nfft, hop = 1600, 400, 512, 256
    y = torch.from_numpy(rng.standard_normal((G, 8, 8 * FS)).astype(np.float32)).to(dev)
    n_frames = (8 * FS - L) // H + 1
    J, K = (L - nfft) // hop + 1, doa.doa_bins(nfft, FS, (500.0, 4000.0))[1]
    for algo in ("NormMUSIC", "MUSIC", "SRP"):
        med, lo, hi = _time(lambda: doa.doa_frames(y, L, H, nfft, hop, win="hann", algo=algo), 5)
        row = dict(call="doa_frames", algo=algo, G=G, seconds=8, L=L, H=H, nfft=nfft, hop=hop, n_frames=n_frames,
                   snapshots=J, bins=K, ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4),
                   us_per_frame=round(med * 1e3 / (G * n_frames), 3),
                   dft_gflops=round(2.0 * 2 * G * n_frames * J * 8 * nfft * K / med / 1e6, 1))
        res["frames"].append(row)
        print(json.dumps(row), flush=True)
    est, valid = doa.doa_frames(y, L, H, nfft, hop)
    med, lo, hi = _time(lambda: doa.frame_stats(est, valid), 20)
    row = dict(call="frame_stats", G=G, n_frames=n_frames, ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4))
    res["frames"].append(row)
    print(json.dumps(row), flush=True)

    tpath = os.path.join(REPO, "tests", "golden", "doa", "timing.npz")
    if os.path.exists(tpath):
        with np.load(tpath) as z:
            res["cpu_ms"] = {str(k): round(float(v), 2) for k, v in zip(z["names"], z["ms"])}
            res["cpu_note"] = json.loads(str(z["meta"]))["note"] + "; restate_frames_* is ONE group"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
