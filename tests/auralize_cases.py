"""Auralization test cases shared by the GPU tests, the CPU tests and
tools/gen_auralize_golden.py (which writes tests/golden/auralize/ from the
reference's whitenoise_bandpass_doa.py): inputs regenerated from seeds, the
index sets the fixtures keep of large outputs, and a float64 numpy
restatement of scipy.signal.sosfiltfilt."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "auralize")
FS = 16000

# name, C, Nh, L, S, seed, input kind.  White, non-decaying h: every tap weighs in.
CONV_CASES = [
    ("meshrir", 8, 1022, 4000, 1, 11, "spec"),  # F = 512 spectra through synth_observation
    ("ragged", 3, 255, 701, 1, 12, "time"),     # odd sizes everywhere
    ("short_x", 8, 1022, 100, 1, 13, "time"),   # L < Nh
    ("one_nh1", 1, 1, 1, 1, 14, "time"),        # degenerate sizes
    ("one_nh2", 1, 2, 1, 1, 15, "time"),
    ("groups", 40, 250, 1500, 3, 16, "time"),   # C not a multiple of 32, several sources
    ("long_ir", 8, 4094, 2500, 1, 17, "time"),  # the longest accumulation chain
]
CONV = {c[0]: c for c in CONV_CASES}

# the reference's four bands (whitenoise_config/*.yml), order 4 at fs = 16000
BANDS = [(500.0, 6000.0), (600.0, 6000.0), (1000.0, 4000.0), (1500.0, 6000.0)]
# name, rows, n, input dtype, seed ("meshrir": the meshrir fixture's own output)
BP_CASES = [
    ("bp_meshrir", 8, 5021, "float32", None),
    ("bp_block", 40, 300, "float32", 21),
    ("bp_n28", 3, 28, "float32", 22),  # the shortest legal length at padlen 27
]
# single sections: butter(2, 0.2) and a first-order section (b2 = a2 = 0: padlen 6)
SINGLE_CASES = [("single_o2", 4, 50, "float64", 23), ("single_o1", 4, 50, "float64", 24)]


def conv_inputs(name):
    """(h_or_spec, x): h fp32 [C, Nh] (or spec complex64 [C, F] for a "spec"
    case) and x fp32 [L] (or [S, L] when S > 1)."""
    _, C, Nh, L, S, seed, kind = CONV[name]
    rng = np.random.default_rng(seed)
    if kind == "spec":
        F = Nh // 2 + 1
        spec = (rng.standard_normal((C, F)) + 1j * rng.standard_normal((C, F))).astype(np.complex64)
        spec[:, 0] = spec[:, 0].real
        spec[:, -1] = spec[:, -1].real
        h = spec
    else:
        h = rng.standard_normal((C, Nh)).astype(np.float32)
    x = rng.standard_normal((S, L)).astype(np.float32)
    return h, (x[0] if S == 1 else x)


def conv_keep(name):
    """(rows, cols) of the expected output a fixture keeps: every row in full
    for the small cases; for `groups` four full rows (both sides of the 32-row
    tile edge) plus every 8th column of all rows."""
    _, C, Nh, L, S, _, _ = CONV[name]
    N = L + Nh - 1
    if name == "groups":
        return np.array([0, 31, 32, 39]), np.arange(0, N, 8)
    return np.arange(C), np.zeros(0, np.int64)


def bp_input(name, meshrir_y=None):
    for nm, rows, n, dt, seed in BP_CASES + SINGLE_CASES:
        if nm == name:
            if seed is None:
                assert meshrir_y.shape == (rows, n) and meshrir_y.dtype == np.float32
                return meshrir_y
            return np.random.default_rng(seed).standard_normal((rows, n)).astype(dt)
    raise KeyError(name)


def bp_cols(n):
    """Columns of a band-pass result a fixture keeps: both edges (where a
    wrong zi, pad or direction shows first) and a comb over the middle."""
    if n <= 64:
        return np.arange(n)
    edge, step = (128, 32) if n > 1000 else (40, 5)
    return np.unique(np.concatenate([np.arange(edge), np.arange(n - edge, n), np.arange(0, n, step)]))


def digest(*arrays):
    """A few numbers that identify the inputs a fixture was made from."""
    out = []
    for a in arrays:
        a = np.asarray(a)
        if np.iscomplexobj(a):
            a = np.stack([a.real, a.imag], -1)
        f = a.astype(np.float64).ravel()
        out += [f[:8], f[-8:], [f.sum(), (f * f).sum()]]
    return np.concatenate([np.asarray(o, np.float64).ravel() for o in out])


def load(name):
    return np.load(os.path.join(GOLDEN, f"{name}.npz"))


# ------------------------------------------------ float64 restatements

def restate_zi(sos):
    """scipy.signal.sosfilt_zi restated (a0 == 1)."""
    sos = np.asarray(sos, np.float64)
    zi = np.empty((sos.shape[0], 2))
    scale = 1.0
    for i, (b0, b1, b2, _, a1, a2) in enumerate(sos):
        K = (b0 + b1 + b2) / (1.0 + a1 + a2)
        zi[i] = scale * (K - b0), scale * (b2 - a2 * K)
        scale *= K
    return zi


def restate_padlen(sos):
    sos = np.asarray(sos)
    return 3 * (2 * sos.shape[0] + 1 - min((sos[:, 2] == 0).sum(), (sos[:, 5] == 0).sum()))


def _sosfilt(sos, zi, x):
    """Direct form II transposed over the last axis of x [rows, m] from the
    state zi[section] * x[:, 0], scipy's op order, float64."""
    x = np.array(x, np.float64)
    rows, m = x.shape
    z = np.stack([np.outer(zi[:, 0], x[:, 0]), np.outer(zi[:, 1], x[:, 0])], 0)  # [2, ns, rows]
    for t in range(m):
        u = x[:, t]
        for s, (b0, b1, b2, _, a1, a2) in enumerate(sos):
            v = b0 * u + z[0, s]
            z[0, s] = b1 * u - a1 * v + z[1, s]
            z[1, s] = b2 * u - a2 * v
            u = v
        x[:, t] = u
    return x


def restate_sosfiltfilt(sos, y):
    """scipy.signal.sosfiltfilt(sos, y, axis=-1) with its defaults, restated
    in float64 numpy for y [rows, n]: the odd extension is taken in y's own
    precision (as scipy's odd_ext does), everything after it in float64."""
    sos = np.asarray(sos, np.float64)
    y = np.asarray(y)
    p = restate_padlen(sos)
    if y.shape[-1] <= p:
        raise ValueError(f"The length of the input vector x must be greater than padlen, which is {p}.")
    two = y.dtype.type(2)
    ext = np.concatenate([two * y[:, :1] - y[:, p:0:-1], y, two * y[:, -1:] - y[:, -2:-(p + 2):-1]], axis=1)
    zi = restate_zi(sos)
    f = _sosfilt(sos, zi, ext)
    b = _sosfilt(sos, zi, f[:, ::-1])[:, ::-1]
    return b[:, p:-p] if p > 0 else b
