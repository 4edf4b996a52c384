"""Time the multi-channel ray reduction against the single-channel one.

Config 2 (R = 1024, S = 256, T = 1022, one pose) with an fp32 and an fp16
signal: `avr_ray_reduce_fwd` (t_1, the kernel every render runs) and
`avr_ray_reduce_mc_fwd` at C = 2, 4, 8 in the same process, and the same for
the backward pair.  Weights and delays come from `avr_weights_fwd` on seeded
poses, so the live windows are those of a render.  HIP events around each
launch, the variants interleaved round-robin, the median over `--reps`
launches after `--warmup` rounds.

    python tools/bench_spatial.py [--reps 25] [--out profiles/spatial_reduce.json]

Prints one JSON document and a markdown table of t_mc(C)/t_1 and
t_mc(C)/(C t_1).
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from avr_amd import AVRRender, _lib  # noqa: E402
from avr_amd.renderer import _weights, get_tables, reduce_mc_splits, reduce_splits  # noqa: E402
from avr_amd.workloads import WORKLOADS  # noqa: E402

CHANNELS = (2, 4, 8)


def variants(w, dtype, dev):
    """name -> zero-argument launcher, for one signal dtype."""
    B, R, S, T = w.batch, w.n_rays, w.n_samples, w.T
    gen = torch.Generator(device=dev).manual_seed(0)
    r = AVRRender(None, **w.render)
    ro = torch.rand(B, 3, device=dev, generator=gen) * 4 - 2
    tx = torch.rand(B, 3, device=dev, generator=gen) * 4 - 2
    torch.manual_seed(0)
    *_, geom = r.sample(ro, tx)
    p = r._params(T, R)
    pref = ctypes.byref(p)
    tables = get_tables(p, dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    attn = torch.rand(B, R * S, device=dev, generator=gen) * 2
    wt, delay = _weights(p, attn, geom["rays_o"], geom["position_tx"], geom["dirs"], tables, st)
    sig = (torch.randn(B, R, S, T, device=dev, generator=gen) * 0.1).to(dtype)
    code = {torch.float32: 0, torch.float16: 1}[dtype]
    grad = torch.empty_like(sig)
    gw = torch.empty(B, R, S, device=dev)
    cmax = max(CHANNELS)
    gain = torch.rand(cmax, R, device=dev, generator=gen) * 2 - 1
    gz = torch.randn(B * cmax, S, T, device=dev, generator=gen)
    n1 = reduce_splits(p, B, code)
    part1 = torch.empty(n1, B, S, T, device=dev)
    out = {
        "fwd_1": lambda: _lib.call("avr_ray_reduce_fwd", pref, B, sig.data_ptr(), code, wt.data_ptr(), delay.data_ptr(),
                                   n1, part1.data_ptr(), st),
        "bwd_1": lambda: _lib.call("avr_ray_reduce_bwd", pref, B, sig.data_ptr(), code, gz.data_ptr(), wt.data_ptr(),
                                   delay.data_ptr(), grad.data_ptr(), gw.data_ptr(), st),
    }
    info = {"n_split_1": n1}
    for C in CHANNELS:
        n, _ = reduce_mc_splits(p, B, C, code)
        part = torch.empty(n, B * C, S, T, device=dev)
        g = gain[:C].contiguous()
        info[f"n_split_mc{C}"] = n
        out[f"fwd_mc{C}"] = (lambda C=C, n=n, part=part, g=g: _lib.call(
            "avr_ray_reduce_mc_fwd", pref, B, C, sig.data_ptr(), code, wt.data_ptr(), delay.data_ptr(), g.data_ptr(),
            0, n, part.data_ptr(), st))
        out[f"bwd_mc{C}"] = (lambda C=C, g=g: _lib.call(
            "avr_ray_reduce_mc_bwd", pref, B, C, sig.data_ptr(), code, gz.data_ptr(), wt.data_ptr(), delay.data_ptr(),
            g.data_ptr(), 0, grad.data_ptr(), gw.data_ptr(), st))
    info["signal_bytes"] = sig.numel() * sig.element_size()
    return out, info


def measure(fns, reps, warmup):
    times = {k: [] for k in fns}
    for i in range(warmup + reps):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= warmup:
                times[k].append(e0.elapsed_time(e1) * 1e3)
    return {k: statistics.median(v) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    dev = torch.device("cuda", 0)
    w = WORKLOADS["c2_meshrir_1024x256x512"]
    doc = {"workload": w.name, "reps": args.reps, "unit": "us", "results": {}}
    rows = []
    for dtype in (torch.float32, torch.float16):
        fns, info = variants(w, dtype, dev)
        med = measure(fns, args.reps, args.warmup)
        name = str(dtype).split(".")[1]
        doc["results"][name] = dict(info, median_us=med)
        for d in ("fwd", "bwd"):
            t1 = med[f"{d}_1"]
            for C in CHANNELS:
                t = med[f"{d}_mc{C}"]
                rows.append((name, d, C, t1, t, t / t1, t / (C * t1)))
        del fns
        torch.cuda.empty_cache()
    doc["accept_fwd_mc4_lt_4x"] = {k: v["median_us"]["fwd_mc4"] < 4 * v["median_us"]["fwd_1"]
                                   for k, v in doc["results"].items()}
    print(json.dumps(doc))
    print("| signal | pass | C | t_1 us | t_mc(C) us | t_mc/t_1 | t_mc/(C t_1) |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        print("| %s | %s | %d | %.1f | %.1f | %.2f | %.2f |" % r)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
