"""Cases and host restatements for the time-varying convolution
(`avr_amd.auralize.convolve_trajectory`), shared by
tests/test_trajectory_cpu.py and tests/test_gpu_trajectory.py.

The definition, restated here without the code under test:

    q = min(m // hop, P-1),  j = m - ((q+1) hop - fade)
    q+1 < P and j >= 0:  u = fp32(2j+1) / fp32(2 fade),  w[q+1, m] = u,  w[q, m] = fp32(1 - u)
    otherwise:           w[q, m] = 1
    xw[p, m] = fp32(w[p, m] x[m])
    y[c, n]  = sum_p sum_k ir[p, c, k] xw[p, n - k]
"""
import functools

import numpy as np

# name: (P, C, Nh, L, hop, fade)
CASES = {
    "one_point": (1, 1, 1, 5, 3, 0),                  # single point, single tap
    "tiny_hop": (4, 3, 70, 200, 5, 3),                # many points inside one stage window
    "full_fade_group": (5, 8, 130, 700, 160, 160),    # 16-row tile, interpolation everywhere, two output blocks
    "wide17": (3, 17, 257, 900, 300, 64),             # 32-row tile, Nh not a stage multiple
    "wide40": (3, 40, 65, 1300, 600, 600),            # two channel tiles, three output blocks
    "rect": (6, 2, 64, 100, 40, 0),                   # hard switches
    "short_x": (4, 8, 300, 50, 100, 20),              # L < hop: point 0 only; L < Nh
    "hold_tail": (2, 8, 96, 1500, 200, 200),          # last point holds over two blocks
    "seam_at_block": (3, 1, 64, 1100, 512, 1),        # seam on an output-block edge, u = 1/2
    "meshrir": (4, 8, 1022, 4000, 1000, 400),         # MeshRIR IR length
}
NAMES = list(CASES)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(ir [P, C, Nh], x [L]) of a case, float32: standard normal IRs under
    exp(-k / (Nh / 6)), a standard normal source."""
    P, C, Nh, L, _, _ = CASES[name]
    rng = np.random.default_rng(2200 + NAMES.index(name))
    env = np.exp(-np.arange(Nh) / (Nh / 6.0))
    ir = (rng.standard_normal((P, C, Nh)) * env).astype(np.float32)
    x = rng.standard_normal(L).astype(np.float32)
    ir.setflags(write=False)
    x.setflags(write=False)
    return ir, x


def weights(P, L, hop, fade):
    """w [P, L] float32 of the definition."""
    m = np.arange(L, dtype=np.int64)
    q = np.minimum(m // hop, P - 1)
    j = m - ((q + 1) * hop - fade)
    fading = (q + 1 < P) & (j >= 0)
    u = (2 * np.where(fading, j, 0) + 1).astype(np.float32) / np.float32(max(2 * fade, 1))
    w = np.zeros((P, L), np.float32)
    w[q, m] = np.where(fading, np.float32(1) - u, np.float32(1))
    w[np.minimum(q + 1, P - 1)[fading], m[fading]] = u[fading]
    return w


def windowed(x, P, hop, fade):
    """xw [P, L] float32: one rounding per product."""
    return weights(P, len(x), hop, fade) * x[None, :]


def _support(row):
    nz = np.flatnonzero(row)
    return (0, 0) if nz.size == 0 else (int(nz[0]), int(nz[-1]) + 1)


def restate64(ir, x, hop, fade):
    """y [C, L+Nh-1] float64, the overlap-add form sum_p np.convolve(xw[p], ir[p, c])."""
    P, C, Nh = ir.shape
    xw = windowed(x, P, hop, fade).astype(np.float64)
    y = np.zeros((C, len(x) + Nh - 1))
    for p in range(P):
        s, e = _support(xw[p])
        if e > s:
            for c in range(C):
                y[c, s:e + Nh - 1] += np.convolve(xw[p, s:e], ir[p, c].astype(np.float64))
    return y


def direct64(ir, x, hop, fade):
    """The same y by a loop over source samples: sample m adds
    xw[p, m] ir[p, :, :] at delay m for the (at most two) points in force."""
    P, C, Nh = ir.shape
    xw = windowed(x, P, hop, fade).astype(np.float64)
    h = ir.astype(np.float64)
    y = np.zeros((C, len(x) + Nh - 1))
    for m in range(len(x)):
        for p in np.flatnonzero(xw[:, m]):
            y[:, m:m + Nh] += xw[p, m] * h[p]
    return y


def seq32(ir, x, hop, fade):
    """The definition in float32: for every output the later point first,
    taps ascending, every multiply and every add rounded to fp32."""
    P, C, Nh = ir.shape
    xw = windowed(x, P, hop, fade)
    assert xw.dtype == np.float32
    y = np.zeros((C, len(x) + Nh - 1), np.float32)
    for p in range(P - 1, -1, -1):
        s, e = _support(xw[p])
        for k in range(Nh if e > s else 0):
            y[:, s + k:e + k] += ir[p, :, k, None] * xw[p, None, s:e]
    return y


@functools.lru_cache(maxsize=None)
def reference(name):
    """(y64, e32) of a case: the float64 restatement and the distance of the
    sequential fp32 form from it, as a fraction of max|y64|."""
    ir, x = inputs(name)
    *_, hop, fade = CASES[name]
    y64 = restate64(ir, x, hop, fade)
    e32 = float(np.abs(seq32(ir, x, hop, fade) - y64).max() / np.abs(y64).max())
    y64.setflags(write=False)
    return y64, e32
