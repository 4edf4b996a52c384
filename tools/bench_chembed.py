"""GPU time of the channel-embedding bias + ReLU kernels (csrc/chembed.hip)
beside the torch-op composition they replace (`KernelOptions(chembed=False)`:
gather, add, relu, cast, and autograd's backward of those), HIP events, at the
reference's own shape: real_exp_ch_emb_add_das (batch 8, 64 x 32 + 2 rays, 64
samples: N = 1,049,600 rows, 8 groups, 8 channels), widths 512 (signal
network) and 128 (sigma encoder), fp16 and bf16.  Recorded, not gated: the
comparison base is the composition, and no number is fixed in advance.

Achieved bytes/s are against the live bytes: forward reads y and writes out
(4 B per 16-bit element), backward reads gy and out and writes g (6 B).

Each step is a child process under its own `timeout`; the first non-zero
status ends the run.

    python tools/bench_chembed.py [--out profiles/chembed_gpu.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, G, C = 1_049_600, 8, 8
STEPS = [(W, dt) for W in (512, 128) for dt in ("float16", "bfloat16")]
LIMIT_S = 180


def _time(fn, calls, windows):
    import torch

    for _ in range(5):  # code objects, the allocator's blocks
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / calls)
    return dict(ms_median=statistics.median(ms), ms_min=min(ms), ms_max=max(ms))


def child(W, dtype_name, calls, windows):
    import torch

    from avr_amd.chembed import bias_relu_bwd, bias_relu_fwd, bias_relu_torch

    dev = torch.device("cuda", 0)
    dtype = getattr(torch, dtype_name)
    rpg = N // G
    g = torch.Generator(device=dev).manual_seed(0)
    y = torch.randn(N, W, device=dev, generator=g).to(dtype)
    gy = torch.randn(N, W, device=dev, generator=g).to(dtype)
    table = torch.randn(C, W, device=dev, generator=g) / W ** 0.5
    idx = torch.randint(0, C, (G,), device=dev, generator=g)
    out = bias_relu_fwd(y, table, idx, rpg)
    yr, tr = y.clone().requires_grad_(True), table.clone().requires_grad_(True)

    def comp_fwd():
        with torch.no_grad():
            return torch.relu(y + table[idx].repeat_interleave(rpg, 0)).to(dtype)

    def comp_fwd_bwd():
        yr.grad = tr.grad = None
        bias_relu_torch(yr, tr, idx, rpg).backward(gy)

    res = dict(
        kernel_fwd=_time(lambda: bias_relu_fwd(y, table, idx, rpg, out=out), calls, windows),
        kernel_bwd=_time(lambda: bias_relu_bwd(gy, out, idx, rpg, C), calls, windows),
        composition_fwd=_time(comp_fwd, calls, windows),
        composition_fwd_bwd=_time(comp_fwd_bwd, calls, windows),
    )
    elems, size = N * W, y.element_size()
    res["kernel_fwd"]["live_bytes"] = 2 * size * elems
    res["kernel_bwd"]["live_bytes"] = 3 * size * elems
    for k in ("kernel_fwd", "kernel_bwd"):
        res[k]["bytes_per_s"] = res[k]["live_bytes"] / (res[k]["ms_median"] * 1e-3)
    res["composition_bwd_ms_by_difference"] = (res["composition_fwd_bwd"]["ms_median"]
                                               - res["composition_fwd"]["ms_median"])
    props = torch.cuda.get_device_properties(dev)  # what the step actually ran on
    print(json.dumps(dict(device=f"{props.name} ({props.gcnArchName}, {props.multi_processor_count} CUs)",
                          N=N, W=W, G=G, C=C, dtype=dtype_name, calls=calls, **res,
                          what="events around back-to-back calls: host issue and output allocation included")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chembed_gpu.json"))
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--child", nargs=2, metavar=("W", "DTYPE"))
    a = ap.parse_args()
    if a.child:
        child(int(a.child[0]), a.child[1], a.calls, a.windows)
        return
    lines = []
    for W, dt in STEPS:
        r = subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__),
                            "--child", str(W), dt, "--calls", str(a.calls), "--windows", str(a.windows)],
                           capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stderr)
            raise SystemExit(f"bench_chembed: step (W={W}, {dt}) ended with status {r.returncode}")
        line = json.loads(r.stdout.strip().splitlines()[-1])
        lines.append(line)
        print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        devices = sorted({line["device"] for line in lines})  # as the child processes reported it
        json.dump(dict(tool="tools/bench_chembed.py", device=", ".join(devices), results=lines), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
