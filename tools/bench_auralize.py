"""Times the auralization kernels on an MI355X with HIP events (recorded, not
gated): `convolve_source` at the reference's 144 channels (18 groups x 8
microphones) for Nh in {1022, 1600, 4094} and sources of 8 s and 100 s at
16 kHz, one 8-microphone group for comparison, and `zero_phase_sos` at
144 x 8 s.

Each shape is warmed up, then timed as one event pair around `reps` calls
(median of `rounds` such windows).  FLOP are counted from the shapes:
`useful` = 2 C Nh L (what np.convolve does), `issued` = what the MFMA tiles
execute (32-row tiles, or one 16-row tile for C <= 16; 64-tap stages,
512-sample blocks, padding included).
The fp32 matrix peak is 157 TF/s.  The reference's CPU milliseconds for ONE
channel of the same lengths come from tests/golden/auralize/timing.npz (its
own functions on the machine that wrote the fixtures); they are per channel
and per core and are not multiplied out here.

    python tools/bench_auralize.py --out profiles/auralize_gpu.json

`--trajectory` times `convolve_trajectory` instead (C = 8 and 144, the same
three Nh, 8 s, a path point every 100 ms, fade = hop and hop / 4) with
`convolve_source` at the same C, Nh and L, measured in the same run, as the
yardstick; the issued count follows the kernel's own (stage, point, wave)
passes.

    python tools/bench_auralize.py --trajectory   # profiles/auralize_trajectory_gpu.json
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

PEAK_TF = 157.0
FS = 16000


def _time(fn, reps, rounds):
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


def issued_flop(C, Nh, L):
    N = L + Nh - 1
    total = 0
    for blk in range((N + 511) // 512):
        nb = blk * 512
        k_begin = max(0, (nb - (L - 1)) // 64 * 64)
        k_end = min(Nh, nb + 512)
        stages = max(0, (k_end - k_begin + 63) // 64)
        total += stages * 64 * 512 * 2
    rows = 16 if C <= 16 else 32  # the 16-row tile serves C <= 16
    return total * rows * ((C + rows - 1) // rows)


def issued_flop_trajectory(P, C, Nh, L, hop, fade):
    """What conv_trajectory_kernel's MFMAs execute: per output block and
    64-tap stage, one pass per path point whose samples meet the stage's
    window of x, in each wave (128 outputs) whose own window meets them."""
    N = L + Nh - 1
    first = lambda p: p * hop - fade if p > 0 else 0          # noqa: E731
    end = lambda p: (p + 1) * hop if p + 1 < P else L          # noqa: E731
    if hop - fade >= L:
        P = 1
    passes = 0
    for blk in range((N + 511) // 512):
        nb = blk * 512
        k_begin = max(0, (nb - (L - 1)) // 64 * 64)
        k_end = min(Nh, nb + 512)
        for k0 in range(k_begin, k_end, 64):
            lo, hi = max(nb - k0 - 63, 0), min(nb - k0 + 511, L - 1)
            for p in range(min(lo // hop, P - 1), min((hi + fade) // hop, P - 1) + 1):
                for wave in range(4):
                    wlo = nb + 128 * wave - k0 - 63
                    passes += first(p) <= wlo + 190 and end(p) > wlo
    rows = 16 if C <= 16 else 32
    return passes * 64 * 128 * 2 * rows * ((C + rows - 1) // rows)


def trajectory(args):
    """`convolve_trajectory` against `convolve_source` (the static kernel, the
    yardstick) at the same C, Nh and L in the same run: 8 s at 16 kHz, a path
    point every 100 ms, crossfades over the whole hop and over a quarter."""
    from avr_amd import auralize

    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    L, hop = 8 * FS, 1600
    P = (L + hop - 1) // hop
    res = dict(device=torch.cuda.get_device_name(0), peak_tf=PEAK_TF, fs=FS, seconds=8, hop=hop, points=P, rows=[])
    x = torch.from_numpy(rng.standard_normal(L).astype(np.float32)).to(dev)
    for C in (8, 144):
        for Nh in (1022, 1600, 4094):
            h = torch.from_numpy(rng.standard_normal((P, C, Nh)).astype(np.float32)).to(dev)
            h0 = h[0].contiguous()
            static, *_ = _time(lambda: auralize.convolve_source(h0, x), 10, 5)
            static_issued = float(issued_flop(C, Nh, L))
            for fade in (hop, hop // 4):
                med, lo, hi = _time(lambda: auralize.convolve_trajectory(h, x, hop, fade), 10, 5)
                issued = float(issued_flop_trajectory(P, C, Nh, L, hop, fade))
                row = dict(C=C, Nh=Nh, L=L, hop=hop, fade=fade, ms=round(med, 4), ms_min=round(lo, 4),
                           ms_max=round(hi, 4), issued_tflops=round(issued / med / 1e9, 2),
                           issued_of_peak=round(issued / med / 1e9 / PEAK_TF, 4),
                           static_ms=round(static, 4), static_issued_tflops=round(static_issued / static / 1e9, 2),
                           ratio_to_static=round(med / static, 3), issued_ratio=round(issued / static_issued, 3),
                           expected_ratio=round(1 + fade / hop, 3))
                res["rows"].append(row)
                print(json.dumps(row), flush=True)
            del h, h0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: profiles/auralize_gpu.json, or "
                    "profiles/auralize_trajectory_gpu.json with --trajectory")
    ap.add_argument("--quick", action="store_true", help="8 s sources only")
    ap.add_argument("--trajectory", action="store_true",
                    help="time convolve_trajectory against convolve_source instead (DESIGN.md §22)")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(REPO, "profiles",
                                "auralize_trajectory_gpu.json" if args.trajectory else "auralize_gpu.json")
    if not torch.cuda.is_available():
        raise SystemExit("bench_auralize: no HIP device (nothing is measured on the CPU)")
    if args.trajectory:
        return trajectory(args)
    from avr_amd import auralize

    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    res = dict(device=torch.cuda.get_device_name(0), peak_tf=PEAK_TF, fs=FS, conv=[], zero_phase=[])
    shapes = [(144, nh, secs) for secs in ((8,) if args.quick else (8, 100)) for nh in (1022, 1600, 4094)]
    # one group (16-row tile), C = 17 (one 32-row tile: what one group cost on it), full tiles
    shapes += [(8, 4094, 8), (16, 4094, 8), (17, 4094, 8), (32, 4094, 8), (160, 4094, 8)]
    for C, Nh, secs in shapes:
        L = secs * FS
        h = torch.from_numpy(rng.standard_normal((C, Nh)).astype(np.float32)).to(dev)
        x = torch.from_numpy(rng.standard_normal(L).astype(np.float32)).to(dev)
        reps = 10 if secs == 8 else 3
        med, lo, hi = _time(lambda: auralize.convolve_source(h, x), reps, 5)
        useful, issued = 2.0 * C * Nh * L, float(issued_flop(C, Nh, L))
        row = dict(C=C, Nh=Nh, L=L, seconds=secs, ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4),
                   useful_tflops=round(useful / med / 1e9, 2), useful_of_peak=round(useful / med / 1e9 / PEAK_TF, 4),
                   issued_tflops=round(issued / med / 1e9, 2), issued_of_peak=round(issued / med / 1e9 / PEAK_TF, 4),
                   out_gbytes_per_s=round(4.0 * C * (L + Nh - 1) / med / 1e6, 1))
        res["conv"].append(row)
        print(json.dumps(row), flush=True)
        del h, x
    # the reference's 500-6000 Hz order-4 band-pass, from the fixture (no scipy needed here)
    with np.load(os.path.join(REPO, "tests", "golden", "auralize", "bp_block.npz")) as z:
        sos = z["sos"][0]
    y = torch.from_numpy(rng.standard_normal((144, 8 * FS)).astype(np.float32)).to(dev)
    for dt in (torch.float64, torch.float32):
        med, lo, hi = _time(lambda: auralize.zero_phase_sos(y, sos, out_dtype=dt), 3, 5)
        row = dict(rows=144, n=8 * FS, sections=4, out=str(dt).split(".")[1], ms=round(med, 3),
                   ms_min=round(lo, 3), ms_max=round(hi, 3),
                   ns_per_sample_per_pass=round(med * 1e6 / (2 * (8 * FS + 54)), 2))
        res["zero_phase"].append(row)
        print(json.dumps(row), flush=True)
    tpath = os.path.join(REPO, "tests", "golden", "auralize", "timing.npz")
    if os.path.exists(tpath):
        with np.load(tpath) as z:
            res["reference_cpu_ms"] = {str(k): round(float(v), 2) for k, v in zip(z["names"], z["ms"])}
            res["reference_cpu_note"] = json.loads(str(z["meta"]))["note"] + "; np_convolve_* are ONE channel"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
