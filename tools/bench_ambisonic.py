"""Time the one-pass MFMA ray reduction against the vector kernels.

Config 2 (R = 1024, S = 256, T = 1022, one pose) with an fp32 and an fp16
signal: `avr_ray_reduce_mc16_fwd` and `avr_ray_reduce_mc_fwd` at C = 5, 8, 9
and 16 at the same n_split, and `avr_ray_reduce_fwd` (t_1, the kernel every
render runs) beside them, all interleaved round-robin in one process.
Operands as tools/bench_spatial.py: weights and delays from `avr_weights_fwd`
on seeded poses, so the live windows are those of a render.  HIP events
around each launch; median, min and max over `--reps` launches after
`--warmup` rounds.  The two kernels' outputs are compared bit for bit.  One
more line times a whole binaural `render_ir` (`ambisonic(3)` and a decoder)
against the mono `render_ir`.

    python tools/bench_ambisonic.py [--reps 25] [--out profiles/ambisonic_reduce.json]

Prints one JSON document and a markdown table.
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

from avr_amd import AVRRender, _lib, spatial  # noqa: E402
from avr_amd.renderer import _weights, get_tables, reduce_mc_splits, reduce_splits  # noqa: E402
from avr_amd.workloads import WORKLOADS  # noqa: E402

CHANNELS = (5, 8, 9, 16)


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
    gain = spatial.ambisonic(3)(geom["dirs"]).contiguous()
    n1 = reduce_splits(p, B, code)
    part1 = torch.empty(n1, B, S, T, device=dev)
    out = {"fwd_1": lambda: _lib.call("avr_ray_reduce_fwd", pref, B, sig.data_ptr(), code, wt.data_ptr(),
                                      delay.data_ptr(), n1, part1.data_ptr(), st)}
    info = {"n_split_1": n1, "bitwise_equal": {}}
    for C in CHANNELS:
        n, _ = reduce_mc_splits(p, B, C, code)
        g = gain[:C].contiguous()
        parts = {}
        info[f"n_split_mc{C}"] = n
        for name, entry in (("vec", "avr_ray_reduce_mc_fwd"), ("mfma", "avr_ray_reduce_mc16_fwd")):
            part = parts[name] = torch.empty(n, B * C, S, T, device=dev)
            out[f"{name}_mc{C}"] = (lambda entry=entry, C=C, n=n, part=part, g=g: _lib.call(
                entry, pref, B, C, sig.data_ptr(), code, wt.data_ptr(), delay.data_ptr(), g.data_ptr(), 0, n,
                part.data_ptr(), st))
            out[f"{name}_mc{C}"]()
        torch.cuda.synchronize()
        info["bitwise_equal"][str(C)] = bool(torch.equal(parts["vec"], parts["mfma"]))
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
    return {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in times.items()}


def whole_render(w, dev, reps, warmup):
    """render_ir of a stub network's fp16 output: mono against binaural."""
    B, R, S, T = w.batch, w.n_rays, w.n_samples, w.T
    gen = torch.Generator(device=dev).manual_seed(1)
    attn = torch.rand(B, R * S, device=dev, generator=gen) * 2
    sig = (torch.randn(B, R * S, T, device=dev, generator=gen) * 0.1).half()

    class Stub(torch.nn.Module):
        def forward(self, pts, view, tx, dir_tx=None):
            return attn, sig

    r = AVRRender(Stub(), **w.render)
    ro = torch.rand(B, 3, device=dev, generator=gen) * 4 - 2
    tx = torch.rand(B, 3, device=dev, generator=gen) * 4 - 2
    grid = torch.randn(256, 3, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    dec = spatial.sh_decoder(spatial.spherical_head_hrtf(grid, w.render["fs"], T), grid, 3, fs=w.render["fs"]).to(dev)
    amb = spatial.ambisonic(3)
    with torch.no_grad():
        return measure({"render_ir_mono": lambda: r.render_ir(ro, tx),
                        "render_ir_binaural": lambda: r.render_ir(ro, tx, ray_gain=amb, sh_decoder=dec)}, reps, warmup)


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
        t = measure(fns, args.reps, args.warmup)
        name = str(dtype).split(".")[1]
        doc["results"][name] = dict(info, us=t)
        for C in CHANNELS:
            v, m = t[f"vec_mc{C}"], t[f"mfma_mc{C}"]
            rows.append((name, C, t["fwd_1"]["median"], v["median"], v["min"], v["max"], m["median"], m["min"],
                         m["max"], m["median"] / v["median"], m["median"] / t["fwd_1"]["median"]))
        del fns
        torch.cuda.empty_cache()
    # the smallest measured C from which on the MFMA kernel is faster at both
    # dtypes by more than the spread of the runs (its slowest launch under the
    # vector kernels' fastest)
    wins = [C for C in CHANNELS if all(doc["results"][d]["us"][f"mfma_mc{C}"]["max"] <
                                       doc["results"][d]["us"][f"vec_mc{C}"]["min"] for d in doc["results"])]
    doc["c_min"] = next((C for C in CHANNELS if all(c in wins for c in CHANNELS if c >= C)), None)
    doc["whole_render_us"] = whole_render(w, dev, args.reps, args.warmup)
    print(json.dumps(doc))
    print("| signal | C | t_1 us | vector us (min-max) | MFMA us (min-max) | MFMA/vector | MFMA/t_1 |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        print("| %s | %d | %.1f | %.1f (%.1f-%.1f) | %.1f (%.1f-%.1f) | %.2f | %.2f |" % r)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
