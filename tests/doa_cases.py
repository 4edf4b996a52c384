"""DoA test cases shared by the GPU tests, the CPU tests and
tools/gen_doa_golden.py (which writes tests/golden/doa/ from the reference's
plot_eval.py and whitenoise_bandpass_doa.py): inputs regenerated from seeds,
float64 numpy restatements of the reference's NormDAS score and circular
statistics, the synthetic plane-wave scenes of the frame estimators and the
restatement of their definition (parity with pyroomacoustics
is unpinned, the definition is the contract)."""
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "doa")
MICS = 8
DAS_SPEED = 343.8
DAS_KEYS = ("true_deg", "pred_deg", "gt_deg", "pred_vs_gt_error", "pred_vs_true_error", "gt_vs_true_error")
DAS_METHODS = ("NormDAS_soft-argmax", "NormDAS_argmax")

# name, N rows, IR length T (spectra have T/2 + 1 bins), fs, kind, position dtype
DAS_CASES = [
    ("g1", 8, 512, 16000, "noise", "float32"),       # one group, a flat power: fractional soft-argmax
    ("g5", 40, 512, 16000, "noise", "float32"),      # five groups (batch against single calls)
    ("ragged", 19, 300, 16000, "noise", "float32"),  # G = 2, three rows ignored; zero-padded to 512
    ("long48k", 16, 1600, 48000, "noise", "float32"),  # truncated to 512, another fs
    ("burst", 24, 512, 16000, "burst", "float32"),   # delayed copies of a burst: a sharp peak, soft = arg
]
# float64 positions (the trainer's dumps hold float32 ones): the reference then
# takes the mean in float64 too
DAS_CASES.append(("pos64", 16, 512, 16000, "noise", "float64"))
DAS = {c[0]: c for c in DAS_CASES}


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


def das_unit_circle():
    """The reference's array for its steering table: unit radius, uncentred."""
    ang = np.linspace(math.pi / 2, math.pi / 2 + 2 * math.pi, MICS + 1)[:-1]
    return np.stack([np.cos(ang), np.sin(ang)], -1)


def das_inputs(name, seed):
    """A synthetic validation dump: pred_sig / ori_sig complex64 [N, F],
    position_rx / position_tx [N, 3]."""
    _, N, T, fs, kind, pdt = DAS[name]
    rng = np.random.default_rng(seed)
    F = T // 2 + 1
    G = -(-N // MICS)

    def spectra():
        if kind == "noise":
            ir = rng.standard_normal((N, T)) * np.exp(-np.arange(T) / (0.3 * T))
            return np.fft.rfft(ir, axis=-1)
        # a short burst, advanced per microphone as a plane wave on the table's unit circle
        burst = np.zeros(T)
        burst[40:72] = rng.standard_normal(32) * np.hanning(32)
        B = np.fft.rfft(burst)
        f = np.arange(F) * fs / T
        spec = np.zeros((G * MICS, F), complex)
        for g in range(G):
            th = np.deg2rad(rng.uniform(0.0, 360.0))
            tau = das_unit_circle() @ np.array([np.cos(th), np.sin(th)]) / DAS_SPEED
            spec[g * MICS:(g + 1) * MICS] = B[None] * np.exp(2j * np.pi * f[None] * tau[:, None])
        spec[:, -1] = spec[:, -1].real
        return spec[:N]

    pred = spectra().astype(np.complex64)
    ori = spectra().astype(np.complex64)
    centre = rng.uniform(-2.0, 2.0, (G, 1, 3))
    phi = np.pi / 2 + 2 * np.pi * np.arange(MICS) / MICS
    ring = 0.0365 * np.stack([np.cos(phi), np.sin(phi), np.zeros(MICS)], -1)
    rx = (centre + ring[None]).reshape(-1, 3)[:N]
    tx = np.repeat(rng.uniform(-3.0, 3.0, (G, 1, 3)), MICS, 1).reshape(-1, 3)[:N]
    return dict(pred_sig=pred, ori_sig=ori, position_rx=rx.astype(pdt), position_tx=tx.astype(pdt))


def angular_error_deg(a, b):
    return min(abs(a - b), 360 - abs(a - b))


def restate_true_deg(rx, tx):
    """plot_eval.py:179-187 for one group (numpy's own mean, in the positions' precision)."""
    centre = np.mean(rx[:, :2], axis=0)
    dx, dy = tx[0][0] - centre[0], tx[0][1] - centre[1]
    return np.degrees(math.atan2(dy, dx)) % 360


def restate_das(d, fs=16000, n_fft=512, angle_resolution=1.0, beta=100.0):
    """plot_eval.py:134-265 in float64 numpy.  Returns (results, power) with
    results laid out as the reference's dictionary and power [G][2][K] (pred,
    ori) for the generator's peak-margin check."""
    pred_sig, ori_sig = np.asarray(d["pred_sig"]), np.asarray(d["ori_sig"])
    G = pred_sig.shape[0] // MICS
    angles = np.arange(0.0, 360.0, angle_resolution)
    rad = np.deg2rad(angles)
    u = np.stack([np.cos(rad), np.sin(rad)], -1)                 # [K, 2]
    delays = (u @ das_unit_circle().T) / DAS_SPEED               # [K, M]
    freqs = np.fft.rfftfreq(n_fft, 1 / fs)
    steer = np.exp(-2j * np.pi * delays[:, :, None] * freqs[None, None, :])
    res = {m: {k: [] for k in DAS_KEYS} for m in DAS_METHODS}
    powers = []
    for g in range(G):
        sl = slice(g * MICS, (g + 1) * MICS)
        true_deg = restate_true_deg(np.asarray(d["position_rx"])[sl], np.asarray(d["position_tx"])[sl])
        out = []
        for sig in (pred_sig, ori_sig):
            t = np.fft.irfft(sig[sl].astype(np.complex128), axis=-1)
            X = np.fft.rfft(t, n=n_fft, axis=-1)
            beam = np.einsum("mf,kmf->kf", X, steer) / MICS
            bp = np.abs(beam) ** 2
            power = (bp / (bp.sum(0, keepdims=True) + 1e-8)).sum(-1)
            z = beta * power
            w = np.exp(z - z.max())
            w /= w.sum()
            out.append((float((w * angles).sum()) % 360, float(angles[int(np.argmax(power))]) % 360, power))
        powers.append(np.stack([out[0][2], out[1][2]]))
        for mi, m in enumerate(DAS_METHODS):
            p, o = out[0][mi], out[1][mi]
            for k, v in zip(DAS_KEYS, (true_deg, p, o, angular_error_deg(p, o), angular_error_deg(p, true_deg),
                                       angular_error_deg(o, true_deg))):
                res[m][k].append(v)
    return res, np.stack(powers)


def peak_margin(power):
    """Smallest height of a maximum of power [..., K] above its two 1-step
    neighbours (circular)."""
    k = power.argmax(-1)[..., None]
    K = power.shape[-1]
    top = np.take_along_axis(power, k, -1)
    nb = np.maximum(np.take_along_axis(power, (k + 1) % K, -1), np.take_along_axis(power, (k - 1) % K, -1))
    return (top - nb)[..., 0]


# ------------------------------------------------------- circular statistics
# name, length, seed, kind
CIRC_CASES = [("empty", 0, 0, "uniform"), ("one", 1, 31, "uniform"), ("fifty", 50, 32, "cluster"),
              ("wrap", 50, 33, "wrap"), ("uniform", 50, 34, "uniform")]


def circ_angles(name):
    """Integer angles in [0, 360) as the frame estimators return them."""
    for nm, n, seed, kind in CIRC_CASES:
        if nm == name:
            rng = np.random.default_rng(seed)
            if kind == "uniform":  # R near 0
                a = rng.integers(0, 360, n)
            elif kind == "cluster":
                a = np.round(rng.normal(137.0, 12.0, n)).astype(np.int64) % 360
            else:  # clustered across the 0 / 360 wrap
                a = np.round(rng.normal(1.0, 9.0, n)).astype(np.int64) % 360
            return [float(v) for v in a]
    raise KeyError(name)


def restate_circ_stats(angles_deg):
    """whitenoise_bandpass_doa.py:36-49 (and :162-164 for an empty list)."""
    n = len(angles_deg)
    if n == 0:
        return float("nan"), float("nan"), float("nan")
    a = np.deg2rad(np.asarray(angles_deg, np.float64))
    C, S = float(np.cos(a).sum()), float(np.sin(a).sum())
    mu = (np.rad2deg(math.atan2(S, C)) + 360.0) % 360.0
    R = math.hypot(C, S) / n
    std = np.rad2deg(np.sqrt(max(0.0, -2.0 * math.log(max(R, 1e-12))))) if R > 0 else float("nan")
    return mu, 1.0 - R, std


# --------------------------------------------------------- frame estimators
FS = 16000
C_SOUND = 343.0
MIC_RADIUS = 0.0365
ALGOS = ("SRP", "MUSIC", "NormMUSIC")
# name, L, nfft, hop, win, freq_range, G, n_frames, kind, seed
SCENES = [
    ("hann256", 800, 256, 64, "hann", (500.0, 4000.0), 3, 7, "dry", 101),
    ("hann512", 1600, 512, 256, "hann", (500.0, 4000.0), 1, 7, "reverb", 112),
    ("rect512", 1600, 512, 256, "none", (500.0, 4000.0), 3, 1, "dry", 113),
    ("one_snapshot", 1200, 1024, 512, "none", (500.0, 4000.0), 1, 7, "dry", 104),  # J = 1
    ("hann1024", 3200, 1024, 256, "hann", (500.0, 4000.0), 3, 1, "reverb", 115),
    ("too_short", 200, 256, 64, "hann", (500.0, 4000.0), 1, 7, "dry", 106),        # J = 0: invalid
    ("bins39", 800, 256, 64, "hann", (700.0, 3100.0), 1, 7, "dry", 137),           # 39 bins
]
SCENE = {s[0]: s for s in SCENES}


def mic_ring(radius=MIC_RADIUS):
    phi = np.pi / 2 + 2 * np.pi * np.arange(MICS) / MICS
    return radius * np.stack([np.cos(phi), np.sin(phi)], -1)


def _plane_wave(src, theta_deg, fs=FS):
    """src [n] as it arrives at the 8 microphones from direction theta: the
    microphone nearer to the source hears it earlier (a fractional shift made
    in the frequency domain)."""
    n = src.size
    th = np.deg2rad(theta_deg)
    tau = mic_ring() @ np.array([np.cos(th), np.sin(th)]) / C_SOUND
    f = np.fft.rfftfreq(n, 1 / fs)
    return np.fft.irfft(np.fft.rfft(src)[None] * np.exp(2j * np.pi * f[None] * tau[:, None]), n=n, axis=-1)


def scene(name):
    """(y fp32 [G, 8, n], theta [G] in degrees, H): a white source per group
    as a plane wave from a random direction; "dry": 20 dB SNR; "reverb": six
    delayed, attenuated copies from other directions, 10 dB SNR.  H does not
    divide n - L."""
    _, L, nfft, hop, win, fr, G, nf, kind, seed = SCENE[name]
    rng = np.random.default_rng(seed)
    H = max(1, (3 * L) // 4 + 1)
    n = L + (nf - 1) * H + H // 3 + 1
    pad = 512
    ys, thetas = [], []
    for _ in range(G):
        theta = rng.uniform(0.0, 360.0)
        src = rng.standard_normal(n + 2 * pad)
        y = _plane_wave(src, theta)
        snr_db = 20.0
        if kind == "reverb":
            snr_db = 10.0
            for _ in range(6):
                d = int(rng.integers(20, 300))
                y = y + rng.uniform(0.2, 0.5) * np.roll(_plane_wave(src, rng.uniform(0.0, 360.0)), d, axis=-1)
        y = y[:, pad:pad + n]
        y = y + rng.standard_normal(y.shape) * np.sqrt(np.mean(y * y)) * 10 ** (-snr_db / 20)
        ys.append(y)
        thetas.append(theta)
    return np.stack(ys).astype(np.float32), np.array(thetas), H


def doa_bins(nfft, fs, freq_range):
    top = nfft // 2 + 1
    lo = min(max(int(round(freq_range[0] * nfft / fs)), 0), top)
    hi = min(max(int(round(freq_range[1] * nfft / fs)), lo), top)
    return lo, hi - lo


def restate_frames(y, L, H, nfft, hop, win="hann", algo="NormMUSIC", fs=FS, c=C_SOUND, mic_radius=MIC_RADIUS,
                   freq_range=(500.0, 4000.0), floor=1e-4, dtype=np.float64):
    """The definition of the frame estimators in numpy, in
    float64 / complex128, or with dtype=np.float32 in float32 / complex64 (the
    measure of what single precision alone costs).  Returns est [G, n_frames]
    int, valid [G, n_frames] bool, spectrum [G, n_frames, 360]."""
    rt = np.dtype(dtype)
    ct = np.complex128 if rt == np.float64 else np.complex64
    y = np.asarray(y).astype(np.float32).astype(rt)  # fp64 input is rounded to fp32 on load
    G, _, n = y.shape
    nf = (n - L) // H + 1 if n >= L else 0
    J = (L - nfft) // hop + 1 if L >= nfft else 0
    k_lo, K = doa_bins(nfft, fs, freq_range)
    t = np.arange(nfft)
    w = ((0.5 - 0.5 * np.cos(2 * np.pi * t / nfft)) if win == "hann" else np.ones(nfft)).astype(rt)
    th = np.deg2rad(np.arange(360.0))
    proj = mic_ring(mic_radius) @ np.stack([np.cos(th), np.sin(th)])          # [8, 360]
    f = (k_lo + np.arange(K)) * fs / nfft
    a = np.exp(2j * np.pi * f[:, None, None] * proj[None] / c).astype(ct)     # [K, 8, 360]
    est = np.full((G, nf), -1, np.int64)
    valid = np.zeros((G, nf), bool)
    spec = np.zeros((G, nf, 360), rt)
    for g in range(G):
        for i in range(nf):
            fr = y[g, :, i * H:i * H + L]
            if J < 1 or not np.isfinite(fr).all():
                continue
            seg = np.stack([fr[:, j * hop:j * hop + nfft] for j in range(J)]) * w   # [J, 8, nfft]
            X = np.fft.rfft(seg, axis=-1)[..., k_lo:k_lo + K].astype(ct)           # [J, 8, K]
            if algo == "SRP":
                X = X / np.maximum(np.abs(X), rt.type(1e-14))
            R = np.einsum("jmk,jnk->kmn", X, X.conj()) / rt.type(J)                 # [K, 8, 8]
            if algo == "SRP":
                Ra = np.einsum("kmn,knt->kmt", R, a)
                P = (a.conj() * Ra).sum(1).real.sum(0) / rt.type(K)   # per bin first, then over the bins
            else:
                _, vecs = np.linalg.eigh(R)
                e = vecs[:, :, -1]                                                 # [K, 8]
                q = np.abs(np.einsum("km,kmt->kt", e.conj(), a)) ** 2
                Pk = 1.0 / np.maximum(rt.type(8.0) - q, rt.type(8.0 * floor))
                if algo == "NormMUSIC":
                    Pk = Pk / Pk.max(-1, keepdims=True)
                P = Pk.sum(0) / rt.type(K)
            spec[g, i] = P.astype(rt)
            est[g, i] = int(np.argmax(P))
            valid[g, i] = True
    return est, valid, spec


def circ_dist(a, b):
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) % 360.0
    return np.minimum(d, 360.0 - d)


def frames_margin(spec):
    """Height of each frame's maximum of spec [..., 360] / max above both of
    its 1-degree neighbours."""
    s = spec / np.maximum(spec.max(-1, keepdims=True), 1e-300)
    return peak_margin(s)
