"""Golden vectors for the auralization chain from the REAL reference
`whitenoise_bandpass_doa.py` (build container only; /root/reference is absent
on the GPU box).

pyroomacoustics (the reference's DoA dependency) is not installed.  Its import
is satisfied by a placeholder module; only `white_noise`, `synth_observation`,
`butter_bandpass_sos`, `apply_zero_phase_bp`, `seg_hop_samples` and
`sliding_frames` are called, and none of them touches the placeholder.

Fixtures hold data only: seeds, shapes, the sos and zi tables, expected
outputs (for large outputs the rows and columns `auralize_cases` names), a
digest of the inputs (tests regenerate the inputs from the seeds).  Arrays are
written with fixed zip timestamps, so every file regenerates bit-identically
except `timing.npz`, which records measurements: the reference's CPU
milliseconds on the machine that wrote it.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_auralize_golden.py [--no-timing]
"""
from __future__ import annotations

import io
import json
import os
import sys
import time
import types
import zipfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.dont_write_bytecode = True
REF = "/root/reference"

sys.path.insert(0, os.path.join(REPO, "tests"))
import auralize_cases as ac  # noqa: E402


def _reference():
    sys.modules["pyroomacoustics"] = types.ModuleType("pyroomacoustics")  # never touched
    sys.path.insert(0, REF)
    import whitenoise_bandpass_doa as ref  # noqa: E402  (the reference's file)

    return ref


def save(name, **arrays):
    """np.savez_compressed with a fixed timestamp and member order."""
    path = os.path.join(ac.GOLDEN, f"{name}.npz")
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


def _median_ms(fn, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return sorted(t)[len(t) // 2]


def main():
    import scipy
    from scipy import signal

    ref = _reference()
    os.makedirs(ac.GOLDEN, exist_ok=True)
    versions = dict(numpy=np.__version__, scipy=scipy.__version__)
    timing = {}

    # ---- convolution: synth_observation (spectra) / its np.convolve line (time-domain h)
    meshrir_y = None
    for name, C, Nh, L, S, seed, kind in ac.CONV_CASES:
        h, x = ac.conv_inputs(name)
        xs = x[None] if x.ndim == 1 else x
        if kind == "spec":
            fn = lambda xi: ref.synth_observation(h, xi)
        else:
            # synth_observation's body after its irfft (whitenoise_bandpass_doa.py:100-101)
            fn = lambda xi: np.stack([np.convolve(xi, h_i, mode="full") for h_i in h], 0).astype(np.float32)
        y = np.stack([fn(xi) for xi in xs], 0)
        timing[f"conv_{name}"] = _median_ms(lambda: fn(xs[0]), 3)
        y = y[0] if S == 1 else y
        assert y.dtype == np.float32 and y.shape[-2:] == (C, L + Nh - 1)
        if name == "meshrir":
            meshrir_y = y
        rows, cols = ac.conv_keep(name)
        save(f"conv_{name}",
             meta=json.dumps(dict(name=name, C=C, Nh=Nh, L=L, S=S, seed=seed, kind=kind, **versions,
                                  source="whitenoise_bandpass_doa.py synth_observation (reference)")),
             rows=rows, cols=cols, y_rows=y[..., rows, :], y_cols=y[..., :, cols],
             y_absmax=np.float64(np.abs(y).max()), digest=ac.digest(h, x))

    # ---- white_noise
    wn = [(0.5, 16000, 0), (0.01, 16000, 3), (1.0, 8000, 7)]
    save("white_noise", meta=json.dumps(dict(cases=wn, **versions)),
         digest=np.stack([ac.digest(ref.white_noise(*c))[:18] for c in wn]),
         length=np.array([len(ref.white_noise(*c)) for c in wn]))

    # ---- band-pass: the four reference bands, order 4
    sos4 = np.stack([ref.butter_bandpass_sos(lo, hi, ac.FS, 4) for lo, hi in ac.BANDS])
    zi4 = np.stack([signal.sosfilt_zi(s) for s in sos4])
    for name, rows, n, dt, seed in ac.BP_CASES:
        y = ac.bp_input(name, meshrir_y)
        cols = ac.bp_cols(n)
        outs = [ref.apply_zero_phase_bp(y, s) for s in sos4]
        assert all(o.dtype == np.float64 for o in outs)
        timing[name] = _median_ms(lambda: ref.apply_zero_phase_bp(y, sos4[0]), 3)
        save(name, meta=json.dumps(dict(name=name, rows=rows, n=n, dtype=dt, seed=seed, fs=ac.FS, order=4,
                                        bands=ac.BANDS, padlen=27, **versions,
                                        source="whitenoise_bandpass_doa.py apply_zero_phase_bp (reference)")),
             sos=sos4, zi=zi4, cols=cols, out_cols=np.stack([o[:, cols] for o in outs]),
             out_absmax=np.array([np.abs(o).max() for o in outs]), digest=ac.digest(y))
    # single sections (scipy's sosfiltfilt, the function apply_zero_phase_bp calls)
    singles = {"single_o2": signal.butter(2, 0.2, output="sos"), "single_o1": signal.butter(1, 0.2, output="sos")}
    for name, rows, n, dt, seed in ac.SINGLE_CASES:
        sos = singles[name]
        y = ac.bp_input(name)
        out = ref.apply_zero_phase_bp(y, sos)
        save(name, meta=json.dumps(dict(name=name, rows=rows, n=n, dtype=dt, seed=seed,
                                        padlen=int(ac.restate_padlen(sos)), **versions)),
             sos=sos[None], zi=signal.sosfilt_zi(sos)[None], cols=np.arange(n), out_cols=out[None],
             out_absmax=np.array([np.abs(out).max()]), digest=ac.digest(y))

    # ---- framing: the reference's whole grid (7 segment lengths x 3 overlaps)
    # whitenoise_config/white_noise_bandpass_config.yml: segments_ms, overlap_factors
    segs = [50, 75, 100, 150, 200, 300, 400]
    ovs = [0.75, 0.6667, 0.5]
    grid = np.array([[s, o, *ref.seg_hop_samples(ac.FS, s, o)] for s in segs for o in ovs])
    yy = np.arange(2 * 1000, dtype=np.float32).reshape(2, 1000)
    starts = np.array([f[0, 0] for f in ref.sliding_frames(yy, 256, 192)])
    save("frames", meta=json.dumps(dict(fs=ac.FS, n=1000, L=256, H=192, **versions)), grid=grid,
         starts=starts, n_short=np.int64(len(ref.sliding_frames(yy[:, :100], 256, 192))))

    if "--no-timing" in sys.argv:
        return
    # ---- the reference's CPU time for ONE channel at the benchmark's lengths
    rng = np.random.default_rng(0)
    for Nh, secs in ((1022, 8), (1600, 8), (4094, 8), (4094, 100)):
        xi = rng.standard_normal(secs * ac.FS).astype(np.float32)
        hi = rng.standard_normal(Nh).astype(np.float32)
        timing[f"np_convolve_1ch_Nh{Nh}_L{secs}s"] = _median_ms(lambda: np.convolve(xi, hi, mode="full"),
                                                                3 if secs == 8 else 1)
    yb = rng.standard_normal((144, 8 * ac.FS)).astype(np.float32)
    timing["sosfiltfilt_144x8s"] = _median_ms(lambda: ref.apply_zero_phase_bp(yb, sos4[0]), 3)
    save("timing", meta=json.dumps(dict(cpus=os.cpu_count(), **versions,
                                        note="reference CPU milliseconds; this file is a measurement and "
                                             "does not regenerate bit-identically")),
         names=np.array(sorted(timing)), ms=np.array([timing[k] for k in sorted(timing)]))
    for k in sorted(timing):
        print(f"  {k}: {timing[k]:.2f} ms")


if __name__ == "__main__":
    main()
