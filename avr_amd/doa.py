"""Direction-of-arrival evaluation on the GPU: the last link of the
reference's evaluation chain (`csrc/doa.hip`).

    res = das_doa(pred_spec, ori_spec, position_rx, position_tx)   # plot_eval.py:134-265
    res = das_doa_dump("val_iter000100.npz")

    d = auralize_dump(dump, x, sos)                                # avr_amd.auralize
    est, valid = doa_frames(d["pred"].view(G, 8, -1), L, H, nfft, hop, win="hann")
    stats = frame_stats(est, valid)                                # whitenoise_bandpass_doa.py:152-167

`das_doa` is the reference's NormDAS score (`run_delay_and_sum_on_npz`) for
all groups of 8 microphones and for prediction and measurement together.
`doa_frames` runs the frame-wise narrow-band estimators (SRP-PHAT, MUSIC,
NormMUSIC for one source) that the reference takes from pyroomacoustics; that
library could not be consulted, so the definition in DESIGN.md §19 is the
contract (parity unpinned).  `frame_stats` is the reference's
`circ_stats_deg` over the valid frames.

There is no CPU path (a CPU tensor raises) and no autograd.  After the first
call for a configuration has built its tables, a call makes no device-to-host
copy and no stream sync, allocates only through torch's caching allocator and
runs on torch's current stream.
"""
from __future__ import annotations

import ctypes
import math
import threading

import numpy as np
import torch

from . import _lib
from ._lib import _ptr, _stream

_MICS = 8
_DIRS = 360
_DT = {torch.float32: 0, torch.float64: 3}  # AVR_DTYPE_F32, AVR_DTYPE_F64
_ALGOS = {"SRP": 0, "MUSIC": 1, "NormMUSIC": 2}
DAS_METHODS = ("NormDAS_soft-argmax", "NormDAS_argmax")
DAS_KEYS = ("true_deg", "pred_deg", "gt_deg", "pred_vs_gt_error", "pred_vs_true_error", "gt_vs_true_error")
_DAS_SPEED = 343.8  # plot_eval.py:169, fixed in the reference

_LOCK = threading.Lock()
_DAS_TABLES: dict = {}
_FRAME_TABLES: dict = {}
_CIRC_TABLES: dict = {}


def _need_hip(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"avr_amd.doa: {name} must be a HIP tensor (no CPU fallback)")


def _cached(store, key, build):
    t = store.get(key)
    if t is None:
        with _LOCK:
            t = store.get(key)
            if t is None:
                t = store[key] = build()
    return t


# ------------------------------------------------------------------ NormDAS

def _das_tables(dev, fs, n_fft, resolution, speed):
    """(steer [K][8][F] complex64 as floats, angles [K] degrees fp32, fp64
    twiddles [n_fft][2]) built once per (device, fs, n_fft, resolution, speed)
    on the host with the reference's own torch ops in its order
    (plot_eval.py:166-167, 181-182, 200, 206-211): a unit-radius, uncentred
    8-microphone circle."""
    def build():
        angles = torch.arange(0.0, 360.0, step=resolution)
        angles_rad = torch.deg2rad(angles)
        mic_angles = torch.linspace(math.pi / 2, math.pi / 2 + 2 * math.pi, _MICS + 1)[:-1]
        mic_pos = torch.stack([torch.cos(mic_angles), torch.sin(mic_angles)], dim=-1)
        freqs = torch.fft.rfftfreq(n_fft, 1 / fs)
        steer = torch.zeros(len(angles), _MICS, freqs.numel(), dtype=torch.cfloat)
        for i, theta in enumerate(angles_rad):
            u = torch.tensor([torch.cos(theta), torch.sin(theta)])
            delays = (mic_pos @ u) / speed
            steer[i] = torch.exp(-1j * 2 * np.pi * delays[:, None] * freqs[None, :])
        j = np.arange(n_fft, dtype=np.float64)
        tw = np.stack([np.cos(2 * np.pi * j / n_fft), -np.sin(2 * np.pi * j / n_fft)], -1)
        return (torch.view_as_real(steer).contiguous().to(dev), angles.float().contiguous().to(dev),
                torch.from_numpy(tw).to(dev))
    return _cached(_DAS_TABLES, (dev.index, float(fs), int(n_fft), float(resolution), float(speed)), build)


def _spec_pairs(spec, name):
    if spec.is_complex():
        spec = torch.view_as_real(spec.detach().to(torch.complex64))
    if spec.dim() != 3 or spec.size(-1) != 2 or spec.size(1) < 2:
        raise ValueError(f"das_doa: {name} [N, F] complex or [N, F, 2] with F >= 2 expected, "
                         f"got {tuple(spec.shape)}")
    return spec.detach().float()


def das_doa(pred_spec, ori_spec, position_rx, position_tx, fs=16000, n_fft=512, angle_resolution=1.0,
            beta=100.0, speed=_DAS_SPEED):
    """plot_eval.py:134-265 `run_delay_and_sum_on_npz` for spectra [N, F]
    complex64 (or [N, F, 2]) and positions [N, 3]: G = N // 8 groups (left-over
    rows are ignored), prediction and measurement together, in a fixed number
    of launches.  Returns {"NormDAS_soft-argmax": {...}, "NormDAS_argmax":
    {...}} with the reference's keys (`DAS_KEYS`) as fp64 device tensors [G].

    The reference's quirks are kept: the steering table is a unit-radius,
    uncentred circle (its `mic_radius` is unused), the speed of sound is 343.8,
    the soft-argmax is a linear mean over the angles, the argmax is the first
    maximum.  The IRs come from `spectrum_to_ir` (fp32), the table from the
    reference's torch ops (fp32); the device sums in fp64."""
    from .renderer import spectrum_to_ir

    for t, nm in ((pred_spec, "pred_spec"), (ori_spec, "ori_spec"), (position_rx, "position_rx"),
                  (position_tx, "position_tx")):
        _need_hip(t, nm)
    dev = pred_spec.device
    pred = _spec_pairs(pred_spec, "pred_spec")
    ori = _spec_pairs(ori_spec, "ori_spec")
    if pred.shape != ori.shape:
        raise ValueError(f"das_doa: pred_spec {tuple(pred.shape)} and ori_spec {tuple(ori.shape)} differ")
    N = pred.size(0)
    G = N // _MICS
    if G < 1:
        raise ValueError("das_doa: at least 8 rows (one group) expected")
    rx, tx = position_rx.detach(), position_tx.detach()
    if rx.dim() != 2 or rx.size(1) != 3 or rx.shape != tx.shape or rx.size(0) < G * _MICS:
        raise ValueError("das_doa: position_rx and position_tx [N, 3] expected")
    dt = torch.float64 if rx.dtype == torch.float64 or tx.dtype == torch.float64 else torch.float32
    rx, tx = rx.to(dt).contiguous(), tx.to(dt).contiguous()
    n_fft = int(n_fft)
    steer, angles, tw = _das_tables(dev, fs, n_fft, angle_resolution, speed)
    K = angles.numel()
    with torch.no_grad():
        ir = spectrum_to_ir(torch.cat([pred[:G * _MICS], ori[:G * _MICS]], 0))
    n = ir.size(1)
    nb = ctypes.c_int64(0)
    _lib.call("avr_doa_das_workspace", G, n_fft, K, ctypes.byref(nb))
    ws = torch.empty(nb.value // 8, dtype=torch.float64, device=dev)
    out = torch.empty((2, len(DAS_KEYS), G), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.call("avr_doa_das", G, n, n_fft, K, _ptr(ir), ir.data_ptr() + G * _MICS * n * 4, _ptr(steer),
                  _ptr(angles), _ptr(tw), float(beta), _ptr(rx), _ptr(tx), _DT[dt], _ptr(out), _ptr(ws),
                  nb.value, _stream(dev))
    return {m: {k: out[i, j] for j, k in enumerate(DAS_KEYS)} for i, m in enumerate(DAS_METHODS)}


def das_doa_dump(path_or_arrays, device=None, **kw):
    """`das_doa` on a validation dump (`data.read_val_dump`: pred_sig, ori_sig,
    position_rx, position_tx), read from a path or given as its dictionary."""
    from .data import read_val_dump

    d = read_val_dump(path_or_arrays) if isinstance(path_or_arrays, (str, bytes)) or hasattr(
        path_or_arrays, "__fspath__") else path_or_arrays
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("avr_amd.doa: das_doa_dump needs a HIP device (no CPU fallback)")

    def spec(a):
        t = torch.as_tensor(np.asarray(a))
        return (t.to(torch.complex64) if t.is_complex() else t.float()).to(dev)
    kw.setdefault("fs", int(np.asarray(d["fs"])) if "fs" in d else 16000)
    return das_doa(spec(d["pred_sig"]), spec(d["ori_sig"]), torch.as_tensor(np.asarray(d["position_rx"])).to(dev),
                   torch.as_tensor(np.asarray(d["position_tx"])).to(dev), **kw)


# --------------------------------------------------------- frame estimators

def doa_bins(nfft, fs, freq_range):
    """(k_lo, K): the bins [round(f_lo nfft / fs), round(f_hi nfft / fs))
    clipped to [0, nfft / 2]."""
    top = nfft // 2 + 1
    lo = min(max(int(round(freq_range[0] * nfft / fs)), 0), top)
    hi = min(max(int(round(freq_range[1] * nfft / fs)), lo), top)
    return lo, hi - lo


def _frame_tables(dev, nfft, win, fs, c, mic_radius, k_lo, K):
    """(twiddles [nfft][2] = (cos, -sin), window [nfft], steering [K][8][360]
    complex64) of a configuration: fp64 on the host, rounded to fp32 once."""
    def build():
        t = np.arange(nfft, dtype=np.float64)
        tw = np.stack([np.cos(2 * np.pi * t / nfft), -np.sin(2 * np.pi * t / nfft)], -1).astype(np.float32)
        w = (0.5 - 0.5 * np.cos(2 * np.pi * t / nfft)) if win == "hann" else np.ones(nfft)
        phi = np.pi / 2 + 2 * np.pi * np.arange(_MICS) / _MICS
        th = np.deg2rad(np.arange(_DIRS, dtype=np.float64))
        proj = mic_radius * (np.cos(phi)[:, None] * np.cos(th)[None] + np.sin(phi)[:, None] * np.sin(th)[None])
        f = (k_lo + np.arange(K, dtype=np.float64)) * fs / nfft
        a = np.exp(2j * np.pi * f[:, None, None] * proj[None] / c)  # [K][8][360]
        st = np.stack([a.real, a.imag], -1).astype(np.float32)
        return (torch.from_numpy(tw).to(dev), torch.from_numpy(w.astype(np.float32)).to(dev),
                torch.from_numpy(st).contiguous().to(dev))
    key = (dev.index, int(nfft), win, float(fs), float(c), float(mic_radius), int(k_lo), int(K))
    return _cached(_FRAME_TABLES, key, build)


def doa_frames(y, L, H, nfft, hop, win="hann", algo="NormMUSIC", fs=16000, c=343.0, mic_radius=0.0365,
               freq_range=(500.0, 4000.0), floor=1e-4, return_spectrum=False):
    """Frame-wise direction of arrival of one source on `y` [G, 8, n] (fp32, or
    fp64 that is rounded to fp32 on load: the estimator's arithmetic is fp32).
    Frame i of a group is y[g, :, i*H : i*H + L], n_frames = (n - L) // H + 1
    (0 when n < L): the framing of `auralize.sliding_frames`, computed in the
    kernel, all (group, frame) pairs in one launch.

    Per frame (DESIGN.md §19 is the definition; parity with pyroomacoustics is
    unpinned): snapshots x_j = rfft(w * frame[:, j*hop : j*hop + nfft]),
    j < J = (L - nfft) // hop + 1, w the periodic Hann window or ones; bins
    `doa_bins(nfft, fs, freq_range)`; R_k = mean_j x_jk x_jk^H; steering
    a_m = exp(+2 pi i f_k (p_m . u_theta) / c) on the circle p_m =
    mic_radius (cos, sin)(pi/2 + 2 pi m / 8), theta = 0..359 degrees.
    "SRP": PHAT-weighted mean_k Re(a^H R_k a); "MUSIC": mean_k 1 / max(8 -
    |e_k^H a|^2, 8 floor) with e_k the principal unit eigenvector of R_k;
    "NormMUSIC": each bin's term divided by its maximum over theta first.

    Returns est_deg [G, n_frames] int32 (the first argmax; -1 where invalid),
    valid [G, n_frames] bool (False for J < 1 or a non-finite sample), and with
    `return_spectrum` the pseudo-spectrum [G, n_frames, 360] fp32 (0 where
    invalid).  Results repeat bitwise and do not depend on the batch."""
    _need_hip(y, "y")
    if y.dim() != 3 or y.size(1) != _MICS:
        raise ValueError(f"doa_frames: y [G, 8, n] expected, got {tuple(y.shape)}")
    if algo not in _ALGOS:
        raise ValueError(f"doa_frames: algo must be one of {sorted(_ALGOS)}")
    if win not in ("hann", "none"):
        raise ValueError('doa_frames: win must be "hann" or "none"')
    L, H, nfft, hop = int(L), int(H), int(nfft), int(hop)
    if min(L, H, hop) < 1 or nfft < 2:
        raise ValueError("doa_frames: L, H, hop must be positive and nfft >= 2")
    k_lo, K = doa_bins(nfft, fs, freq_range)
    if K < 1:
        raise ValueError(f"doa_frames: freq_range {freq_range} holds no bin at nfft {nfft}, fs {fs}")
    yy = y.detach()
    if yy.dtype not in _DT:
        yy = yy.float()
    yy = yy.contiguous()
    dev = yy.device
    G, _, n = yy.shape
    n_frames = (n - L) // H + 1 if n >= L else 0
    est = torch.empty((G, n_frames), dtype=torch.int32, device=dev)
    valid = torch.empty((G, n_frames), dtype=torch.bool, device=dev)
    spec = torch.empty((G, n_frames, _DIRS), dtype=torch.float32, device=dev) if return_spectrum else None
    if G * n_frames > 0:
        tw, w, steer = _frame_tables(dev, nfft, win, fs, c, mic_radius, k_lo, K)
        with torch.cuda.device(dev):
            _lib.call("avr_doa_frames", G, n, L, H, n_frames, nfft, hop, k_lo, K, _ALGOS[algo], float(floor),
                      _ptr(yy), _DT[yy.dtype], _ptr(tw), _ptr(w), _ptr(steer), _ptr(est), _ptr(valid),
                      _ptr(spec), _stream(dev))
    return (est, valid, spec) if return_spectrum else (est, valid)


# --------------------------------------------------------------- statistics

def frame_stats(est_deg, valid):
    """whitenoise_bandpass_doa.py:36-49 `circ_stats_deg` over the valid frames
    of each group of `est_deg` / `valid` [G, n_frames]: a dictionary of device
    tensors [G] with est_deg (the circular mean in [0, 360)), var_circ (1 - R)
    and std_circ_deg in fp64, n_frames and n_valid in int64.  A group without
    a valid frame has NaN statistics (doa_sample_from_frames:162-164)."""
    _need_hip(est_deg, "est_deg")
    _need_hip(valid, "valid")
    if est_deg.dim() != 2 or est_deg.shape != valid.shape:
        raise ValueError("frame_stats: est_deg and valid [G, n_frames] expected")
    dev = est_deg.device
    e = est_deg.detach().to(torch.int32).contiguous()
    v = valid.detach().to(torch.bool).contiguous()
    G, nf = e.shape
    out = torch.empty((3, G), dtype=torch.float64, device=dev)
    nv = torch.empty((G,), dtype=torch.int64, device=dev)
    if G > 0:
        # (cos, sin) of the whole degrees: numpy's values, as the reference takes them
        def build():
            rad = np.deg2rad(np.arange(float(_DIRS)))
            return torch.from_numpy(np.stack([np.cos(rad), np.sin(rad)], -1)).to(dev)
        cs = _cached(_CIRC_TABLES, dev.index, build)
        with torch.cuda.device(dev):
            _lib.call("avr_doa_frame_stats", G, nf, _ptr(e), _ptr(v), _ptr(cs), _ptr(out), _ptr(nv), _stream(dev))
    return dict(est_deg=out[0], var_circ=out[1], std_circ_deg=out[2],
                n_frames=torch.full((G,), nf, dtype=torch.int64, device=dev), n_valid=nv)
