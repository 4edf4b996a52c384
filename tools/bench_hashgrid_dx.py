"""Kernel time of the hash grid's input gradient beside the forward.

Times `avr_hashgrid_bwd_input` (both passes) and `avr_hashgrid_fwd` at the
same shape in one process with device events: config 3's per-sample grid by
default (N = 4 x 650 x 32 points, 20 levels, 2^18 entries), fp32 and fp16
tables.  Both gather the same 8 entries per point and level, so the ratio is
the number of interest.  Each figure is the median of `--reps` windows of
`--iters` back-to-back launches (forward and gradient windows alternate), with
the windows' min and max as the spread.  Ray-ordered points as the renderer
lays them out.  One JSON line per dtype, appended to `--out`.

    python tools/bench_hashgrid_dx.py [--out profiles/hashgrid_dx.jsonl]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from avr_amd import _lib  # noqa: E402
from avr_amd.encoding import HashGridEncoding, _code  # noqa: E402


def ray_points(B, R, S, seed):
    """[B*R*S, 3] in [0, 1]: R rays from each of B listeners, S samples each."""
    rng = np.random.default_rng(seed)
    o = rng.uniform(0.3, 0.7, size=(B, 1, 1, 3))
    d = rng.standard_normal(size=(B, R, 1, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    t = np.linspace(0, 0.25, S).reshape(1, 1, S, 1)
    return np.clip(o + d * t, 0, 1).reshape(-1, 3).astype(np.float32)


def window_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--rays", type=int, default=650)
    ap.add_argument("--samples", type=int, default=32)
    ap.add_argument("--levels", type=int, default=20)
    ap.add_argument("--log2", type=int, default=18)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hashgrid_dx.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_hashgrid_dx needs a GPU: kernel times are not measured anywhere else")
    dev = torch.device("cuda", 0)
    N = a.batch * a.rays * a.samples
    x = torch.from_numpy(ray_points(a.batch, a.rays, a.samples, 0)).to(dev)
    cfg = dict(otype="HashGrid", n_levels=a.levels, n_features_per_level=2, log2_hashmap_size=a.log2,
               base_resolution=16)
    st = torch.cuda.current_stream(dev).cuda_stream
    for dtype in (torch.float32, torch.float16):
        enc = HashGridEncoding(3, cfg, dtype=dtype, seed=1).to(dev)
        with torch.no_grad():
            enc.params.uniform_(-1, 1)
        table = enc.table(False)
        out = torch.empty(N, enc.n_output_dims, dtype=dtype, device=dev)
        g = torch.randn(N, enc.n_output_dims, device=dev).to(dtype)
        gx = torch.empty(N, 3, device=dev)
        nb = ctypes.c_int64()
        _lib.call("avr_hashgrid_bwd_input_workspace", N, enc.n_levels, ctypes.byref(nb))
        ws = torch.empty(nb.value, dtype=torch.uint8, device=dev)
        meta = enc.level_meta()

        def fwd():
            _lib.call("avr_hashgrid_fwd", N, enc.n_levels, x.data_ptr(), table.data_ptr(), _code(table.dtype), *meta,
                      out.data_ptr(), _code(out.dtype), st)

        def dx():
            _lib.call("avr_hashgrid_bwd_input", N, enc.n_levels, x.data_ptr(), table.data_ptr(), _code(table.dtype),
                      g.data_ptr(), _code(g.dtype), *meta, gx.data_ptr(), ws.data_ptr(), nb.value, st)

        for _ in range(a.warmup):
            fwd()
            dx()
        torch.cuda.synchronize()
        tf, td = [], []
        for _ in range(a.reps):
            tf.append(window_ms(fwd, a.iters))
            td.append(window_ms(dx, a.iters))
        stat = lambda v: dict(median_us=1e3 * float(np.median(v)), min_us=1e3 * min(v), max_us=1e3 * max(v))  # noqa: E731
        # bytes the algorithm needs: 8 gathered pairs per point and level, x,
        # the gradient row, the partials written and read once, grad_x
        esz = 2 if dtype == torch.float16 else 4
        gather = N * a.levels * 8 * 2 * esz
        dx_bytes = gather + N * (12 + a.levels * 2 * esz + 12) + 2 * N * a.levels * 12
        res = dict(tool="bench_hashgrid_dx", device=torch.cuda.get_device_name(dev), N=N, levels=a.levels, log2=a.log2,
                   dtype=str(dtype).split(".")[-1], iters=a.iters, reps=a.reps, fwd=stat(tf), dx=stat(td),
                   dx_over_fwd=float(np.median(td) / np.median(tf)), gather_bytes=gather, dx_bytes=dx_bytes,
                   dx_gbps=dx_bytes / (1e6 * float(np.median(td))))
        line = json.dumps(res)
        print(line)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
