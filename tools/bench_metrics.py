"""GPU time of avr_amd.metrics.metric_cal (seven metrics and both energy
curves, csrc/metrics.hip) per call, HIP events, beside the reference's CPU
milliseconds for utils/metric.py:metric_cal recorded in the fixtures' meta
(tests/golden/metrics, taken on the machine that wrote them: a host CPU against
one MI355X, different machines).  Recorded, not gated.

Each shape is timed in a child process of its own under its own time limit.

    python tools/bench_metrics.py [--out profiles/metrics_gpu.json]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

# B, n, fs, and the fixture whose meta holds the reference's time at that n
SHAPES = [(4, 1022, 24000, "meshrir_1022"), (4, 1600, 16000, "raf_1600"), (1, 4094, 16000, "simu_4094")]
LIMIT_S = 120


def child(B, n, fs, calls, windows):
    import torch

    from avr_amd.metrics import metric_cal
    from metrics_cases import irs

    dev = torch.device("cuda", 0)
    ori, pred = irs(B, n, 0)
    o, p = torch.from_numpy(ori).to(dev), torch.from_numpy(pred).to(dev)
    for _ in range(20):  # tables, code objects, the allocator's blocks
        metric_cal(o, p, fs=fs)
    torch.cuda.synchronize()
    ms = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            metric_cal(o, p, fs=fs)
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / calls)
    print(json.dumps(dict(B=B, n=n, fs=fs, calls=calls, gpu_ms_median=statistics.median(ms),
                          gpu_ms_min=min(ms), gpu_ms_max=max(ms),
                          what="events around back-to-back metric_cal calls: host issue included")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics_gpu.json"))
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--child", nargs=3, type=int, metavar=("B", "N", "FS"))
    a = ap.parse_args()
    if a.child:
        child(*a.child, a.calls, a.windows)
        return
    from metrics_cases import load

    lines = []
    for B, n, fs, case in SHAPES:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(B), str(n), str(fs),
                            "--calls", str(a.calls), "--windows", str(a.windows)],
                           capture_output=True, text=True, timeout=LIMIT_S)
        if r.returncode != 0:
            sys.stderr.write(r.stderr)
            raise SystemExit(f"bench_metrics: shape ({B}, {n}) ended with status {r.returncode}")
        line = json.loads(r.stdout.strip().splitlines()[-1])
        meta = json.loads(str(load(case)["meta"]))
        line.update(ref_case=case, ref_B=meta["B"], ref_cpu_ms=meta["ref_cpu_ms"],
                    ref_what="utils/metric.py metric_cal on the fixture's machine (CPU), multi_stft stubbed out")
        lines.append(line)
        print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(tool="tools/bench_metrics.py", device="MI355X", results=lines), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
