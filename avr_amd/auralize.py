"""Auralization on the GPU: everything the reference's direction-of-arrival
evaluation runs in front of its estimators (whitenoise_bandpass_doa.py:93-117,
whitenoise_long_doa.py:95-104).

    x   = white_noise(seconds, fs, seed, device)      # the shared source
    y   = synth_observation(spec, x)                  # irfft + np.convolve(x, h_c, "full")
    y   = zero_phase_sos(y, butter_bandpass_sos(...)) # scipy.signal.sosfiltfilt
    L, H = seg_hop_samples(fs, seg_ms, overlap)
    frames = sliding_frames(y, L, H)                  # [..., n_frames, L], a view

Beyond the reference, a source or listener that moves:

    y = convolve_trajectory(ir, x, hop, fade)         # ir [P, C, Nh] at P path points
    y = synth_trajectory(spec, x, hop, fade)          # from spectra [P, C, F]
    y = auralize_path(renderer, rays_o, position_tx, x, hop)  # from P poses

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


# ---------------------------------------------------------------- trajectory

def _hop_fade(name, hop, fade):
    if isinstance(hop, bool) or not isinstance(hop, (int, np.integer)) or hop < 1:
        raise ValueError(f"{name}: hop must be an integer >= 1, got {hop!r}")
    fade = hop if fade is None else fade
    if isinstance(fade, bool) or not isinstance(fade, (int, np.integer)) or not 0 <= fade <= hop:
        raise ValueError(f"{name}: fade must be an integer in [0, hop = {hop}], got {fade!r}")
    if fade >= 1 << 23:
        raise ValueError(f"{name}: fade must be below 2^23, got {fade}")
    return int(hop), int(fade)


def trajectory_weights(P, L, hop, fade):
    """The weights of `convolve_trajectory` on the host, for tests and plots:
    w [P, L] float32, w[p, m] the share of source sample m played through path
    point p.  With q = min(m // hop, P-1) and j = m - ((q+1) hop - fade): in
    the crossfade at the end of interval q (q+1 < P, j >= 0)
    u = fp32(2j+1) / fp32(2 fade), w[q+1, m] = u, w[q, m] = fp32(1 - u);
    elsewhere w[q, m] = 1.  The last point holds to the end."""
    if P < 1 or L < 1:
        raise ValueError(f"trajectory_weights: P and L must be positive, got {P} and {L}")
    hop, fade = _hop_fade("trajectory_weights", hop, fade)
    m = np.arange(L, dtype=np.int64)
    q = np.minimum(m // hop, P - 1)
    j = m - ((q + 1) * hop - fade)
    cross = (q + 1 < P) & (j >= 0)
    mc, qc = m[cross], q[cross]
    u = (2 * j[cross] + 1).astype(np.float32) / np.float32(2 * fade) if mc.size else np.zeros(0, np.float32)
    w = np.zeros((P, L), np.float32)
    w[q, m] = 1.0
    w[qc, mc] = np.float32(1.0) - u
    w[qc + 1, mc] = u
    return w


def convolve_trajectory(ir, x, hop, fade=None):
    """The source `x` [L] heard along a path: `ir` [P, C, Nh] holds the impulse
    responses at P path points, one point every `hop` source samples, and
    every source sample is played through the IR in force when it is emitted
    (a moving source; to first order a slowly moving listener), crossfading
    linearly to the next point over the last `fade` samples of each hop
    (`trajectory_weights`; fade=None means hop: linear interpolation of the
    IRs along the path; 0 switches hard).  The last point holds to the end of
    `x`.  Returns [C, L+Nh-1] fp32, or [L+Nh-1] for `ir` [P, Nh].

    One launch on the exact-fp32 MFMA (C-ABI `avr_conv_trajectory`), a fixed
    summation order: bitwise repeatable, a row does not depend on the other
    channels, and P = 1, or fade = 0 with equal IRs, gives
    `convolve_source(ir[0], x)` bitwise."""
    _need_hip(ir, "ir")
    _need_hip(x, "x")
    if ir.dim() not in (2, 3) or x.dim() != 1:
        raise ValueError(f"convolve_trajectory: ir [P, C, Nh] or [P, Nh] and x [L] expected, got "
                         f"{tuple(ir.shape)} and {tuple(x.shape)}")
    if ir.device != x.device:
        raise ValueError("convolve_trajectory: ir and x are on different devices")
    hop, fade = _hop_fade("convolve_trajectory", hop, fade)
    h = ir.detach().float().contiguous()
    xs = x.detach().float().contiguous()
    P, Nh = h.size(0), h.size(-1)
    C = 1 if h.dim() == 2 else h.size(1)
    L = xs.size(0)
    if min(P, C, Nh, L) < 1:
        raise ValueError("convolve_trajectory: empty input")
    dev = h.device
    y = torch.empty((C, L + Nh - 1), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.call("avr_conv_trajectory", P, C, Nh, L, hop, fade, _ptr(h), _ptr(xs), _ptr(y), _stream(dev))
    return y[0] if ir.dim() == 2 else y


def synth_trajectory(spec, x, hop, fade=None):
    """`synth_observation` along a path: the irfft of the spectra `spec`
    ([P, C, F] complex64 or [P, C, F, 2] float) at the P path points
    (`spectrum_to_ir`) -> [P, C, 2(F-1)], then `convolve_trajectory`."""
    from .renderer import spectrum_to_ir

    _need_hip(spec, "spec")
    if spec.is_complex():
        spec = torch.view_as_real(spec.detach().to(torch.complex64))
    if spec.dim() != 4 or spec.size(-1) != 2 or spec.size(2) < 2:
        raise ValueError(f"synth_trajectory: spec [P, C, F] complex or [P, C, F, 2] with F >= 2 expected, "
                         f"got {tuple(spec.shape)}")
    P, C, F = spec.shape[:3]
    with torch.no_grad():
        ir = spectrum_to_ir(spec.detach().reshape(P * C, F, 2))
    return convolve_trajectory(ir.view(P, C, -1), x, hop, fade)


def auralize_path(renderer, rays_o, position_tx, x, hop, fade=None, direction_tx=None, ch_idx=None,
                  ray_gain=None, pose_chunk=64, sh_decoder=None):
    """`x` heard while moving through the rendered field: the P poses
    `rays_o` [P, 3] (listener) and `position_tx` [P, 3] or [3] (source;
    `direction_tx` [P, 3] or [3] and `ch_idx` [P] or one value where the
    network takes them) are rendered
    with `renderer.render_ir` under `no_grad`, `pose_chunk` poses per call,
    and `x` is convolved along them (`convolve_trajectory`).  Returns
    [C, L+T-1]: C = 1 for the omnidirectional receiver, the channels of
    `ray_gain` ([C, R] or a callable, see `AVRRender.forward`; a per-pose
    gain [P, C, R], or a callable with `per_pose` set such as
    `spatial.ambisonic(3, rotation=heads)` with P head rotations, is cut with
    the poses) for a directional one, the E ears of `sh_decoder` (see
    `AVRRender.forward`) where one is given: with both, a head-tracked
    binaural walk through the field.

    The azimuth jitter is drawn once (`draw_jitter`, the CPU generator's two
    draws of one render) and handed to every chunk: all points of the path
    look at the same sphere of rays."""
    from .renderer import draw_jitter

    _need_hip(x, "x")
    if rays_o.dim() != 2 or rays_o.size(-1) != 3 or rays_o.size(0) < 1:
        raise ValueError(f"auralize_path: rays_o [P, 3] expected, got {tuple(rays_o.shape)}")
    if pose_chunk < 1:
        raise ValueError("auralize_path: pose_chunk must be positive")
    hop, fade = _hop_fade("auralize_path", hop, fade)
    P = rays_o.size(0)

    def per_pose(t, name):
        if t is None:
            return None
        if t.dim() == 1 and t.size(0) == 3:
            return t.expand(P, 3)
        if tuple(t.shape) != (P, 3):
            raise ValueError(f"auralize_path: {name} [{P}, 3] or [3] expected, got {tuple(t.shape)}")
        return t

    position_tx = per_pose(position_tx, "position_tx")
    direction_tx = per_pose(direction_tx, "direction_tx")
    if ch_idx is not None:  # the network's channel of each pose; one value serves all
        ch_idx = torch.as_tensor(ch_idx).reshape(-1)
        if ch_idx.numel() not in (1, P):
            raise ValueError(f"auralize_path: ch_idx needs 1 or {P} entries, got {ch_idx.numel()}")
        ch_idx = ch_idx.expand(P)
    per_pose_gain = (isinstance(ray_gain, torch.Tensor) and ray_gain.dim() == 3) or \
        bool(getattr(ray_gain, "per_pose", False))
    if per_pose_gain and len(ray_gain) != P:
        raise ValueError(f"auralize_path: a per-pose ray_gain needs {P} poses, got {len(ray_gain)}")
    u_azi = draw_jitter(renderer.n_azi, renderer.n_ele)
    irs = []
    with torch.no_grad():
        for i in range(0, P, pose_chunk):
            s = slice(i, i + pose_chunk)
            _, ir = renderer.render_ir(rays_o[s], position_tx[s], None if direction_tx is None else direction_tx[s],
                                       None if ch_idx is None else ch_idx[s], ray_gain=ray_gain[s] if per_pose_gain else ray_gain,
                                       u_azi=u_azi, **({} if sh_decoder is None else {"sh_decoder": sh_decoder}))
            irs.append(ir.reshape(ir.size(0), -1, ir.size(-1)))
    return convolve_trajectory(irs[0] if len(irs) == 1 else torch.cat(irs), x, hop, fade)


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
