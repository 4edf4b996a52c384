"""Validation-metric test cases shared by the GPU tests, the CPU tests and
tools/gen_metrics_golden.py (which writes tests/golden/metrics/ from the
reference's utils/metric.py): seeded impulse responses, the irfft of
criterion_cases.spectra as fp32 arrays, which is what the runner hands to
metric_cal (avr_runner.py:381-385)."""
import os

import numpy as np
import torch

from criterion_cases import spectra

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics")

CASES = [
    # name, B, n, fs, seed, noise, leading zeros
    ("meshrir_1022", 2, 1022, 24000, 0, 0.3, 0),  # n <= int(0.05 fs): C50 is NaN by design
    ("raf_1600", 4, 1600, 16000, 1, 0.3, 0),
    ("min_258", 3, 258, 4000, 4, 0.3, 0),  # smallest legal n
    ("simu_4094", 1, 4094, 16000, 3, 0.3, 0),
    ("delay_1600", 4, 1600, 16000, 7, 0.3, 120),  # a propagation delay
    ("close_1600", 4, 1600, 16000, 2, 0.05, 0),  # a prediction close to the measurement
]
WINDOW = 32  # metric_cal's default, the only value the runner uses


def irs(B, n, seed, noise=0.3, delay=0):
    """(ori, pred) fp32 [B, n] numpy arrays."""
    pred, ori = spectra(B, n // 2 + 1, seed, noise=noise)
    ori_t = torch.fft.irfft(ori, n=n).float().numpy().copy()
    pred_t = torch.fft.irfft(pred, n=n).float().numpy().copy()
    ori_t[:, :delay] = 0.0
    pred_t[:, :delay] = 0.0
    return ori_t, pred_t


def digest(ori, pred):
    """A few numbers that identify the inputs a fixture was made from."""
    return np.concatenate([ori[:, 128:136].ravel(), pred[:, 128:136].ravel(),
                           (ori.astype(np.float64) ** 2).sum(1), (pred.astype(np.float64) ** 2).sum(1)])


def load(name):
    return np.load(os.path.join(GOLDEN, f"metrics_{name}.npz"))


def restate(ori, pred, fs, window=WINDOW):
    """Angle, Amplitude, Envelope and both energy curves of utils/metric.py
    restated with numpy alone in float64 (np.fft; no scipy), for shapes the
    fixtures do not cover.  tests/test_metrics_cpu.py pins it to the
    fixtures' reference values."""
    ori, pred = ori.astype(np.float64), pred.astype(np.float64)
    n = ori.shape[-1]
    fo, fp = np.fft.fft(ori, axis=-1), np.fft.fft(pred, axis=-1)
    ao, ap = np.angle(fo), np.angle(fp)
    angle = np.mean(np.abs(np.cos(ao) - np.cos(ap))) + np.mean(np.abs(np.sin(ao) - np.sin(ap)))

    def box(m):
        # scipy.ndimage.convolve1d(m, ones(w)), mode='reflect' (numpy calls it 'symmetric'):
        # output i sums inputs i + w//2 - w + 1 .. i + w//2
        ext = np.pad(m, ((0, 0), (window, window)), mode="symmetric")
        c = np.concatenate([np.zeros((m.shape[0], 1)), np.cumsum(ext, axis=-1)], axis=-1)
        i = np.arange(n) + window
        return c[:, i + window // 2 + 1] - c[:, i + window // 2 - window + 1]

    so, sp = box(np.abs(fo)), box(np.abs(fp))
    amp = np.mean(np.abs(so - sp) / so)

    def envelope(f):
        h = np.zeros(n)
        h[0] = h[n // 2] = 1.0
        h[1:n // 2] = 2.0
        return np.abs(np.fft.ifft(f * h, axis=-1))

    eo, ep = envelope(fo), envelope(fp)
    env = np.mean(np.abs(eo - ep) / eo.max(axis=1, keepdims=True))

    def curve(x):
        e = 10.0 * np.log10(np.cumsum(x[:, ::-1] ** 2 + 1e-9, axis=-1)[:, ::-1])
        return e - e[:, :1]

    return angle, amp, env, curve(ori), curve(pred)
