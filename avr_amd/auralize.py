"""Auralization on the GPU: everything the reference's direction-of-arrival
evaluation runs in front of its estimators (whitenoise_bandpass_doa.py:93-117,
whitenoise_long_doa.py:95-104).

    x   = white_noise(seconds, fs, seed, device)      # the shared source
    y   = synth_observation(spec, x)                  # irfft + np.convolve(x, h_c, "full")
    y   = zero_phase_sos(y, butter_bandpass_sos(...)) # scipy.signal.sosfiltfilt
    L, H = seg_hop_samples(fs, seg_ms, overlap)
    frames = sliding_frames(y, L, H)                  # [..., n_frames, L], a view

`convolve_source` is one GEMM with a Toeplitz operand on the exact-fp32 MFMA
(`csrc/auralize.hip`, C-ABI `avr_conv_source`); `zero_phase_sos` runs scipy's
direct-form-II-transposed recurrence in fp64, one thread per row
(`avr_sosfiltfilt`).  There is no CPU path: a CPU tensor raises.  scipy is
imported by `butter_bandpass_sos` alone (filter design is not reimplemented).
After a first call has built the tables of a length / a filter, a call makes
no device-to-host copy and no stream sync, and allocates only through torch's
caching allocator.  Nothing here routes through autograd.
"""
from __future__ import annotations

import ctypes
import threading
import weakref

import numpy as np
import torch

from . import _lib
from ._lib import _ptr, _stream

_DT = {torch.float32: 0, torch.float64: 3}  # AVR_DTYPE_F32, AVR_DTYPE_F64
MAX_SECTIONS = 8

_LOCK = threading.Lock()
_SOS: dict = {}
_SOS_DEV: dict = {}


def _need_hip(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"avr_amd.auralize: {name} must be a HIP tensor (no CPU fallback)")


# ------------------------------------------------------------------ source

def white_noise(seconds, fs, seed, device):
    """whitenoise_bandpass_doa.py:93-96: `default_rng(seed).standard_normal(
    int(round(seconds * fs))).astype(float32)`, drawn on the host (the
    generator's stream is numpy's), as a tensor on `device`."""
    nt = int(round(seconds * fs))
    x = np.random.default_rng(seed).standard_normal(nt).astype(np.float32)
    return torch.from_numpy(x).to(device)


# ------------------------------------------------------------- convolution

def convolve_source(ir, x):
    """`np.convolve(x, h_c, "full")` of every row h_c of `ir` [C, Nh] with the
    source `x` [L] -> [C, L+Nh-1], or with S sources [S, L] -> [S, C, L+Nh-1],
    fp32.  Every output is an fp32 FMA chain in ascending tap order: bitwise
    repeatable, and a row does not depend on the rest of the batch."""
    _need_hip(ir, "ir")
    _need_hip(x, "x")
    if ir.dim() != 2 or x.dim() not in (1, 2):
        raise ValueError(f"convolve_source: ir [C, Nh] and x [L] or [S, L] expected, got "
                         f"{tuple(ir.shape)} and {tuple(x.shape)}")
    if ir.device != x.device:
        raise ValueError("convolve_source: ir and x are on different devices")
    h = ir.detach().float().contiguous()
    xs = x.detach().float().contiguous()
    C, Nh = h.shape
    L = xs.size(-1)
    S = 1 if xs.dim() == 1 else xs.size(0)
    if min(C, Nh, L, S) < 1:
        raise ValueError("convolve_source: empty input")
    dev = h.device
    y = torch.empty((S, C, L + Nh - 1), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.call("avr_conv_source", S, C, Nh, L, _ptr(h), _ptr(xs), _ptr(y), _stream(dev))
    return y[0] if x.dim() == 1 else y


def synth_observation(spec, x):
    """whitenoise_bandpass_doa.py:98-101: the irfft of the dumped spectra
    `spec` ([C, F] complex64 or [C, F, 2] float) -> [C, 2(F-1)] impulse
    responses (the HIP irfft behind `spectrum_to_ir`), convolved with `x`."""
    from .renderer import spectrum_to_ir

    _need_hip(spec, "spec")
    if spec.is_complex():
        spec = torch.view_as_real(spec.detach().to(torch.complex64))
    if spec.dim() != 3 or spec.size(-1) != 2 or spec.size(1) < 2:
        raise ValueError(f"synth_observation: spec [C, F] complex or [C, F, 2] with F >= 2 expected, "
                         f"got {tuple(spec.shape)}")
    with torch.no_grad():
        ir = spectrum_to_ir(spec.detach())
    return convolve_source(ir, x)


# ------------------------------------------------------- zero-phase filter

def _host_sos(sos):
    if isinstance(sos, torch.Tensor):
        sos = sos.detach().cpu().numpy()
    s = np.array(sos, dtype=np.float64)
    if s.ndim != 2 or s.shape[1] != 6:
        raise ValueError("sos must be shape (n_sections, 6)")
    if not (s[:, 3] == 1).all():
        raise ValueError("sos[:, 3] should be all ones")
    return s


def sosfilt_zi(sos):
    """`scipy.signal.sosfilt_zi(sos)` in float64 without scipy: per section
    the steady state of its step response, `scale * [K - b0, b2 - a2 K]` with
    K = sum(b) / sum(a) the section's gain at 0 Hz, and scale the product of
    the gains of the sections before it.  Returns a numpy array [n_sections, 2]."""
    s = _host_sos(sos)
    zi = np.empty((s.shape[0], 2), np.float64)
    scale = 1.0
    for i, (b0, b1, b2, _, a1, a2) in enumerate(s):
        K = (b0 + b1 + b2) / (1.0 + a1 + a2)
        zi[i, 0] = scale * (K - b0)
        zi[i, 1] = scale * (b2 - a2 * K)
        scale *= K
    return zi


def sos_padlen(sos):
    """sosfiltfilt's default padlen: 3 * ntaps with
    ntaps = 2 n_sections + 1 - min(#(b2 == 0), #(a2 == 0))."""
    s = _host_sos(sos)
    ntaps = 2 * s.shape[0] + 1 - min(int((s[:, 2] == 0).sum()), int((s[:, 5] == 0).sum()))
    return 3 * ntaps


def _sos_tables(sos, dev):
    """(sos, zi) device tables, padlen and n_sections of a filter, built once
    per filter and device.  zi and padlen are host work, so a device `sos` is
    read back once per tensor object (again after an in-place change): the
    entry is tied to the live tensor, never to its address alone."""
    if isinstance(sos, torch.Tensor) and sos.is_cuda:
        ident = id(sos)
        e = _SOS_DEV.get(ident)
        if e is not None and e[0]() is sos and e[1] == sos._version and e[2] == dev.index:
            return e[3]
        t = _sos_tables(_host_sos(sos), dev)
        _SOS_DEV[ident] = (weakref.ref(sos, lambda _, i=ident: _SOS_DEV.pop(i, None)), sos._version, dev.index, t)
        return t
    host = _host_sos(sos)
    key = (dev.index, host.tobytes())
    t = _SOS.get(key)
    if t is None:
        with _LOCK:
            t = _SOS.get(key)
            if t is None:
                if host.shape[0] > MAX_SECTIONS:
                    raise ValueError(f"zero_phase_sos: at most {MAX_SECTIONS} sections")
                t = (torch.from_numpy(host.copy()).to(dev), torch.from_numpy(sosfilt_zi(host)).to(dev),
                     sos_padlen(host), host.shape[0])
                _SOS[key] = t
    return t


def zero_phase_sos(y, sos, out_dtype=torch.float64):
    """`scipy.signal.sosfiltfilt(sos, y, axis=-1)` with its defaults (odd
    extension by padlen = 3 ntaps, each pass started from sosfilt_zi times its
    first sample) for `y` [..., n] fp32 or fp64 and a float64 `sos`
    [n_sections, 6] (host array / tensor or device tensor).  Returns fp64 as
    scipy does for either input, or fp32 (the fp64 result rounded) on request.
    `n <= padlen` raises ValueError as scipy does."""
    _need_hip(y, "y")
    if out_dtype not in _DT:
        raise ValueError("zero_phase_sos: out_dtype must be torch.float32 or torch.float64")
    dev = y.device
    sos_d, zi_d, padlen, ns = _sos_tables(sos, dev)
    if y.dim() < 1:
        raise ValueError("zero_phase_sos: y needs a time axis")
    n = y.size(-1)
    if n <= padlen:
        raise ValueError(f"The length of the input vector x must be greater than padlen, which is {padlen}.")
    yy = y.detach()
    if yy.dtype not in _DT:
        yy = yy.float()
    yy = yy.contiguous()
    out = torch.empty(yy.shape, dtype=out_dtype, device=dev)
    rows = yy.numel() // n
    if rows == 0:
        return out
    nb = ctypes.c_int64(0)
    _lib.call("avr_sosfiltfilt_workspace", rows, n, ns, padlen, ctypes.byref(nb))
    ws = torch.empty(nb.value // 8, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.call("avr_sosfiltfilt", rows, n, ns, padlen, _ptr(sos_d), _ptr(zi_d), _ptr(yy), _DT[yy.dtype],
                  _ptr(out), _DT[out_dtype], _ptr(ws), nb.value, _stream(dev))
    return out


def butter_bandpass_sos(low_hz, high_hz, fs, order=4):
    """whitenoise_bandpass_doa.py:103-104: `scipy.signal.butter(order,
    [low, high], btype="band", fs=fs, output="sos")`.  Filter design is
    scipy's; this is the only function here that imports it."""
    try:
        from scipy import signal
    except ImportError as e:
        raise RuntimeError("butter_bandpass_sos designs the filter with scipy.signal.butter, and scipy "
                           "is not installed; pass zero_phase_sos an sos table made elsewhere") from e
    return signal.butter(order, [low_hz, high_hz], btype="band", fs=fs, output="sos")


# ------------------------------------------------------------------ frames

def seg_hop_samples(fs, seg_ms, overlap):
    """whitenoise_bandpass_doa.py:109-112: (segment, hop) lengths in samples."""
    L = int(round(seg_ms * 1e-3 * fs))
    H = max(1, int(round(L * (1.0 - overlap))))
    return L, H


def sliding_frames(y, L, H):
    """whitenoise_bandpass_doa.py:114-117 as one strided view [..., n_frames, L]
    of `y` [..., n] (frame i = y[..., i*H : i*H+L]; no copy); n_frames is 0
    when n < L."""
    if L < 1 or H < 1:
        raise ValueError("sliding_frames: L and H must be positive")
    n = y.size(-1)
    if n < L:
        return y.as_strided((*y.shape[:-1], 0, L), (*y.stride()[:-1], H * y.stride(-1), y.stride(-1)))
    return y.unfold(-1, L, H)


# -------------------------------------------------------------------- dump

def auralize_dump(path_or_arrays, x, sos=None):
    """A validation dump (`data.read_val_dump`: pred_sig / ori_sig [N, F]
    complex spectra, positions) auralized with the source `x` (a HIP tensor
    [L] or [S, L]): a dictionary with the `pred` and `ori` observations
    ([N, L+Nh-1], band-passed to fp64 by `zero_phase_sos` when `sos` is
    given; `ori` is None for a dump without ori_sig) and `position_rx`,
    `position_tx`, all on x's device."""
    from .data import read_val_dump

    _need_hip(x, "x")
    d = read_val_dump(path_or_arrays) if isinstance(path_or_arrays, (str, bytes)) or hasattr(
        path_or_arrays, "__fspath__") else path_or_arrays
    dev = x.device
    out = {}
    for name, key in (("pred", "pred_sig"), ("ori", "ori_sig")):
        if key not in d or d[key] is None:
            out[name] = None
            continue
        spec = torch.as_tensor(np.asarray(d[key]))
        spec = spec.to(torch.complex64) if spec.is_complex() else spec.float()
        obs = synth_observation(spec.to(dev), x)
        out[name] = zero_phase_sos(obs, sos) if sos is not None else obs
    for key in ("position_rx", "position_tx"):
        out[key] = torch.as_tensor(np.asarray(d[key])).to(dev) if key in d and d[key] is not None else None
    return out
