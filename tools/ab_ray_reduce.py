"""A/B of the four ray-reduction entry points between two builds of the library.

    SRC="render_fwd.hip render_bwd.hip" bash tools/build_ab.sh ray_parent <parent rev>
    python tools/ab_ray_reduce.py bits [--a tools/_lib/libab_ray_parent.so] [--b avr_amd/libavr_hip.so]
    python tools/ab_ray_reduce.py time [--reps 25] [--out profiles/ray_stream_ab.json]
    python tools/ab_ray_reduce.py static --old old/fwd.s old/bwd.s --new new/fwd.s new/bwd.s

bits: every case of ALL_REDUCE (avr_ray_reduce_fwd / _bwd) and of MC_FWD /
MC_BWD over CHANNELS (the _mc_ pair), on the inputs the tests synthesise.
`part` and `grad_signal` must be byte-equal between A and B; exits non-zero
otherwise.  grad_w is summed by LDS atomics in wave-arrival order, so it is
not repeatable bit for bit: the tool prints max |B - A| beside max |A - A'| of
two runs of A (relative to the largest |grad_w|) and also exits non-zero where
|B - A| exceeds max |A - A'| by more than the GPU tests' own grad_w bound,
2 (n_live + 8 [+ C]) u sum |gz x|, at any element.

time: the four entry points (C = 4 for the _mc_ pair) at config 2 fp32,
config 3 fp16 and config 5 fp16, A and B interleaved round-robin in one
process, HIP events around each launch; median and the 10th-90th percentile
spread per kernel and library.

static (no GPU): VGPRs and scratch bytes of every ray_reduce* kernel of the new
build beside the old one, as the markdown table of profiles/ray_stream_static.md,
from device assembly listings (`hipcc <the Makefile's FLAGS> --cuda-device-only
-S render_fwd.hip -o fwd.s`).  Kernels are matched by (family, dtype, form,
chunks per lane, G or CB, launch bound, accumulating).  Exits non-zero if a
kernel has more scratch, fewer waves per SIMD by its VGPR count, or static LDS,
or if the headline kernel <float, vector, 1 chunk, 512> has more than 52 VGPRs.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import re
import statistics
import subprocess
import sys

import functools

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import render_stage_cases as rsc  # noqa: E402
import spatial_cases as sc  # noqa: E402
from avr_amd import AVRRender, _lib  # noqa: E402
from avr_amd.renderer import _weights, get_tables, reduce_mc_splits, reduce_splits, render_params  # noqa: E402
from avr_amd.workloads import WORKLOADS  # noqa: E402

DEV = torch.device("cuda", 0)
CODE = {"float32": 0, "float16": 1, "bfloat16": 2}
ENTRIES = ("avr_ray_reduce_fwd", "avr_ray_reduce_bwd", "avr_ray_reduce_mc_fwd", "avr_ray_reduce_mc_bwd")


def load(path):
    lib = ctypes.CDLL(os.path.abspath(path))
    for n in ENTRIES:
        fn = getattr(lib, n)
        fn.restype, fn.argtypes = _lib._SIGS[n]
    return lib


def st():
    return torch.cuda.current_stream().cuda_stream


def nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def same(a, b):
    """Byte equality (NaN patterns included)."""
    a, b = a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)
    return bool(torch.equal(a, b))


@functools.lru_cache(maxsize=None)
def operands(case):
    p = render_params(case.cfg(), case.T, n_rays=case.R)
    shift = rsc.host_shift(case.cfg(), case.T)
    xt, w, delay, gz = rsc.synth_reduce_inputs(case, shift)
    n = xt.numel()
    buf = torch.zeros(n + 8, dtype=xt.dtype, device=DEV)
    x = buf[case.offset:case.offset + n].view(xt.shape)
    x.copy_(xt)
    return dict(p=p, x=x, n=n, w=torch.from_numpy(w).to(DEV), d=torch.from_numpy(delay).to(DEV),
                gz=torch.from_numpy(gz).to(DEV), host=(xt.double().numpy(), gz, w, delay, shift))


class Tally:
    def __init__(self):
        self.fail, self.n, self.gw_ab, self.gw_aa = [], 0, 0.0, 0.0

    def check(self, what, ok):
        self.n += 1
        if not ok:
            self.fail.append(what)
            print("DIFFERS:", what, flush=True)

    def grad_w(self, what, a, a2, b, bound):
        """bound: the GPU tests' grad_w bound against float64, per element."""
        scale = float(a.abs().max()) or 1.0
        d_ab, d_aa = (b - a).abs().cpu().double().numpy(), float((a2 - a).abs().max())
        ab, aa = float(d_ab.max()) / scale, d_aa / scale
        self.gw_ab, self.gw_aa = max(self.gw_ab, ab), max(self.gw_aa, aa)
        print(f"grad_w {what}: max|B-A| {ab:.2e}  max|A-A'| {aa:.2e} (relative)", flush=True)
        self.check(what + " grad_w within max|A-A'| + test bound", bool(np.all(d_ab <= d_aa + bound)))


def bits(A, B, tally):
    for case in list({c.id: c for c in rsc.ALL_REDUCE}.values()):
        o = operands(case)
        pref, code = ctypes.byref(o["p"]), CODE[case.dtype]
        for n_split in case.n_splits:
            outs = []
            for lib in (A, B):
                part = nan(n_split, case.B, case.S, case.T)
                rc = lib.avr_ray_reduce_fwd(pref, case.B, o["x"].data_ptr(), code, o["w"].data_ptr(), o["d"].data_ptr(),
                                            n_split, part.data_ptr(), st())
                torch.cuda.synchronize()
                outs.append((rc, part))
            tally.check(f"fwd {case.id} n_split={n_split}", outs[0][0] == outs[1][0] and same(outs[0][1], outs[1][1]))
        outs = []
        for lib in (A, A, B):
            gbuf = nan(o["n"] + 8, dtype=o["x"].dtype)
            gx = gbuf[case.offset:case.offset + o["n"]].view(o["x"].shape)
            gw = nan(case.B, case.R, case.S)
            rc = lib.avr_ray_reduce_bwd(pref, case.B, o["x"].data_ptr(), code, o["gz"].data_ptr(), o["w"].data_ptr(),
                                        o["d"].data_ptr(), gx.data_ptr(), gw.data_ptr(), st())
            torch.cuda.synchronize()
            outs.append((rc, gbuf, gw))
        tally.check(f"bwd {case.id} grad_signal", outs[0][0] == outs[2][0] and same(outs[0][1], outs[2][1]))
        if outs[0][0] == 0:
            _, _, mag, n_live = rsc.ref_reduce_bwd(*o["host"], with_bound=True)
            tally.grad_w(f"bwd {case.id}", outs[0][2], outs[1][2], outs[2][2], 2.0 * (n_live + 8) * rsc.U32 * mag)
    for C in sc.CHANNELS:
        for case in sc.MC_FWD:
            o = operands(case)
            pref, code = ctypes.byref(o["p"]), CODE[case.dtype]
            for per_pose in (False, True):
                g = torch.from_numpy(sc.synth_gain(case, C, per_pose)).to(DEV)
                stride = C * case.R if per_pose else 0
                for n_split in case.n_splits:
                    outs = []
                    for lib in (A, B):
                        part = nan(n_split, case.B, C, case.S, case.T)
                        rc = lib.avr_ray_reduce_mc_fwd(pref, case.B, C, o["x"].data_ptr(), code, o["w"].data_ptr(),
                                                       o["d"].data_ptr(), g.data_ptr(), stride, n_split,
                                                       part.data_ptr(), st())
                        torch.cuda.synchronize()
                        outs.append((rc, part))
                    tally.check(f"mc_fwd {case.id} C={C} per_pose={per_pose} n_split={n_split}",
                                outs[0][0] == 0 and outs[1][0] == 0 and same(outs[0][1], outs[1][1]))
        for case in sc.MC_BWD:
            o = operands(case)
            pref, code = ctypes.byref(o["p"]), CODE[case.dtype]
            gz_host = sc.synth_gz(case, C)
            gz = torch.from_numpy(gz_host).to(DEV)
            for per_pose in (False, True):
                gain = sc.synth_gain(case, C, per_pose)
                g = torch.from_numpy(gain).to(DEV)
                outs = []
                for lib in (A, A, B):
                    gbuf = nan(o["n"] + 8, dtype=o["x"].dtype)
                    gx = gbuf[case.offset:case.offset + o["n"]].view(o["x"].shape)
                    gw = nan(case.B, case.R, case.S)
                    rc = lib.avr_ray_reduce_mc_bwd(pref, case.B, C, o["x"].data_ptr(), code, gz.data_ptr(),
                                                   o["w"].data_ptr(), o["d"].data_ptr(), g.data_ptr(),
                                                   C * case.R if per_pose else 0, gx.data_ptr(), gw.data_ptr(), st())
                    torch.cuda.synchronize()
                    outs.append((rc, gbuf, gw))
                what = f"mc_bwd {case.id} C={C} per_pose={per_pose}"
                tally.check(what + " grad_signal",
                            outs[0][0] == 0 and outs[2][0] == 0 and same(outs[0][1], outs[2][1]))
                x64, _, w, delay, shift = o["host"]
                *_, mag_w, n_live = sc.ref_reduce_mc_bwd(x64, gz_host, w, delay, shift, gain)
                tally.grad_w(what, outs[0][2], outs[1][2], outs[2][2], 2.0 * (n_live + 8 + C) * rsc.U32 * mag_w)


# ---------------------------------------------------------------- static table
DT = {"float": "f32", "__half": "f16", "__hip_bfloat16": "bf16"}


def asm_kernels(path):
    """{mangled name: (vgprs, scratch bytes, static LDS bytes)} from the amdhsa metadata."""
    out, cur = {}, {}
    for line in open(path, errors="replace"):
        m = re.match(r"\s+(?:- )?\.(name|vgpr_count|private_segment_fixed_size|group_segment_fixed_size):\s+(\S+)", line)
        if not m:
            continue
        k, v = m.groups()
        if k == "name" and v.startswith("_Z"):
            cur["name"] = v
        elif k != "name":
            cur[k] = int(v)
        if len(cur) == 4:
            out[cur["name"]] = (cur["vgpr_count"], cur["private_segment_fixed_size"], cur["group_segment_fixed_size"])
            cur = {}
    return out


def asm_key(demangled):
    m = re.search(r"(ray_reduce\w*_kernel)<(.*?)>\(", demangled)
    if not m:
        return None
    fam = m.group(1)
    a = [x.strip() for x in m.group(2).split(",")]
    a = [re.sub(r"^\((?:bool|int)\)", "", x) for x in a]
    dt, vec, cpt, rest = DT[a[0]], a[1] in ("true", "1"), int(a[2]), a[3:]
    if fam == "ray_reduce_fwd_kernel":      # old <.., U, G, MAXT>, new <.., MAXT>
        g, maxt, acc = 1, int(rest[-1]), False
    elif fam == "ray_reduce_mc_fwd_kernel":  # old <.., U, CB, MAXT>, new <.., CB, MAXT>
        g, maxt, acc = int(rest[-2]), int(rest[-1]), False
    elif fam == "ray_reduce_bwd_kernel":     # old <.., G, MAXT, NTS>, new <.., G, MAXT>
        g, maxt, acc = int(rest[0]), int(rest[1]), False
    else:                                    # <.., CB, MAXT, ACCUM>
        g, maxt, acc = int(rest[0]), int(rest[1]), rest[2] in ("true", "1")
    return fam.replace("ray_reduce_", "").replace("_kernel", ""), dt, vec, cpt, g, maxt, acc


def asm_load(paths):
    ks = {}
    for p in paths:
        ks.update(asm_kernels(p))
    names = list(ks)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return {asm_key(d): ks[n] for n, d in zip(names, dem) if asm_key(d)}


def waves(vgprs):
    """Waves per SIMD by VGPRs alone (512 per lane, allocated in eights)."""
    return min(8, 512 // max(8, -(-vgprs // 8) * 8))

def static_table(old_paths, new_paths):
    old, new = asm_load(old_paths), asm_load(new_paths)
    bad = []
    print("| kernel | dtype | form | cpt | G/CB | bound | add | VGPRs parent → new | scratch B parent → new |")
    print("|---|---|---|---|---|---|---|---|---|")
    for k in sorted(new):
        n, o = new[k], old.get(k)
        if o is None:
            bad.append(f"{k}: not in the old build")
            continue
        fam, dt, vec, cpt, g, maxt, acc = k
        print(f"| {fam} | {dt} | {'vec' if vec else 'elem'} | {cpt} | {g} | {maxt} | {'+' if acc else ''} | "
              f"{o[0]} → {n[0]} | {o[1]} → {n[1]} |")
        if n[1] > o[1]:
            bad.append(f"{k}: scratch {o[1]} -> {n[1]}")
        if waves(n[0]) < waves(o[0]):
            bad.append(f"{k}: waves per SIMD {waves(o[0])} -> {waves(n[0])} (VGPRs {o[0]} -> {n[0]})")
        if n[2] or o[2]:
            bad.append(f"{k}: static LDS {o[2]} -> {n[2]}")
    head = ("fwd", "f32", True, 1, 1, 512, False)
    if new[head][0] > 52:
        bad.append(f"headline kernel: {new[head][0]} VGPRs")
    fams = sorted({k[0] for k in old})
    print("\nkernels in the code object, parent → new: " +
          ", ".join(f"{f} {sum(k[0] == f for k in old)} → {sum(k[0] == f for k in new)}" for f in fams))
    for b in bad:
        print("MISSED:", b)
    return 1 if bad else 0


def time_variants(lib, w, dtype):
    B, R, S, T = w.batch, w.n_rays, w.n_samples, w.T
    gen = torch.Generator(device=DEV).manual_seed(0)
    r = AVRRender(None, **w.render)
    ro = torch.rand(B, 3, device=DEV, generator=gen) * 4 - 2
    tx = torch.rand(B, 3, device=DEV, generator=gen) * 4 - 2
    torch.manual_seed(0)
    *_, geom = r.sample(ro, tx)
    p = r._params(T, R)
    pref = ctypes.byref(p)
    tables = get_tables(p, DEV)
    attn = torch.rand(B, R * S, device=DEV, generator=gen) * 2
    wt, delay = _weights(p, attn, geom["rays_o"], geom["position_tx"], geom["dirs"], tables, st())
    sig = torch.empty(B, R, S, T, device=DEV, dtype=dtype).normal_(0.0, 0.1, generator=gen)
    code = {torch.float32: 0, torch.float16: 1}[dtype]
    grad = torch.empty_like(sig)
    gw = torch.empty(B, R, S, device=DEV)
    C = 4
    gain = torch.rand(C, R, device=DEV, generator=gen) * 2 - 1
    gz = torch.randn(B * C, S, T, device=DEV, generator=gen)
    n1 = reduce_splits(p, B, code)
    n4, _ = reduce_mc_splits(p, B, C, code)
    part = torch.empty(max(n1, n4 * C), B, S, T, device=DEV)
    keep = (p, wt, delay, sig, grad, gw, gain, gz, part)

    def fns(lib):
        return {
            "fwd_1": lambda: lib.avr_ray_reduce_fwd(pref, B, sig.data_ptr(), code, wt.data_ptr(), delay.data_ptr(), n1,
                                                    part.data_ptr(), st()),
            "bwd_1": lambda: lib.avr_ray_reduce_bwd(pref, B, sig.data_ptr(), code, gz.data_ptr(), wt.data_ptr(),
                                                    delay.data_ptr(), grad.data_ptr(), gw.data_ptr(), st()),
            "fwd_mc4": lambda: lib.avr_ray_reduce_mc_fwd(pref, B, C, sig.data_ptr(), code, wt.data_ptr(),
                                                         delay.data_ptr(), gain.data_ptr(), 0, n4, part.data_ptr(), st()),
            "bwd_mc4": lambda: lib.avr_ray_reduce_mc_bwd(pref, B, C, sig.data_ptr(), code, gz.data_ptr(), wt.data_ptr(),
                                                         delay.data_ptr(), gain.data_ptr(), 0, grad.data_ptr(),
                                                         gw.data_ptr(), st()),
        }
    return {f"{k}/{name}": f for name, l in lib.items() for k, f in fns(l).items()}, keep


def measure(fns, reps, warmup):
    times = {k: [] for k in fns}
    for i in range(warmup + reps):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = fn()
            e1.record()
            e1.synchronize()
            assert rc == 0, k
            if i >= warmup:
                times[k].append(e0.elapsed_time(e1) * 1e3)
    out = {}
    for k, v in times.items():
        v = sorted(v)
        out[k] = {"median_us": statistics.median(v), "p10_us": v[len(v) // 10], "p90_us": v[-1 - len(v) // 10]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("bits", "time", "static"))
    ap.add_argument("--old", nargs="+", help="static: the parent's listings")
    ap.add_argument("--new", nargs="+", help="static: the new listings")
    ap.add_argument("--a", default=os.path.join(REPO, "tools", "_lib", "libab_ray_parent.so"))
    ap.add_argument("--b", default=os.path.join(REPO, "avr_amd", "libavr_hip.so"))
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.mode == "static":
        sys.exit(static_table(args.old, args.new))
    A, B = load(args.a), load(args.b)
    if args.mode == "bits":
        t = Tally()
        bits(A, B, t)
        print(json.dumps({"compared": t.n, "differ": len(t.fail), "grad_w_max_rel_B_vs_A": t.gw_ab,
                          "grad_w_max_rel_A_vs_A": t.gw_aa, "failed": t.fail[:20]}))
        sys.exit(1 if t.fail else 0)
    doc = {"a": os.path.basename(args.a), "b": os.path.basename(args.b), "reps": args.reps, "unit": "us", "results": {}}
    for name, dtype in (("c2_meshrir_1024x256x512", torch.float32), ("c3_raf_furnished_b4", torch.float16),
                        ("c5_simu_4096x512x2048", torch.float16)):
        fns, keep = time_variants({"a": A, "b": B}, WORKLOADS[name], dtype)
        doc["results"][f"{name}/{str(dtype).split('.')[1]}"] = measure(fns, args.reps, args.warmup)
        print(name, json.dumps(doc["results"][f"{name}/{str(dtype).split('.')[1]}"]), flush=True)
        del fns, keep
        torch.cuda.empty_cache()
    print(json.dumps(doc))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
