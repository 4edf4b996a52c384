"""Validation metrics on the GPU: drop-in for `utils/metric.py:metric_cal`
and the runner's `calculate_metrics` (avr_runner.py:374-407).

`metric_cal(ori_ir, pred_ir, fs=48000, window=32)` takes HIP tensors [B, n]
(or [n]) and returns the reference's 9-tuple in its order

    (angle_error, amp_error, env_error, t60_error, edt_error, C50_error,
     multi_stft_loss, ori_energy, pred_energy)

with the seven metrics as 0-dim device tensors and the two normalised energy
decay curves as [B, n] device tensors.  Everything runs in the HIP kernels of
`csrc/metrics.hip` through the C-ABI `avr_metrics`; scipy and numpy are not
on the call path and there is no CPU path: a CPU tensor raises.  After a
first call has built the tables for a length, a call does no device-to-host
copy, no stream sync and no allocation outside torch's caching allocator, so
it can be captured in a graph.

Where the reference raises (`stats.linregress` on a row whose -25 dB sample
is not after its -5 dB sample, i.e. fewer than two regression points) that
row's T60 is NaN here, and so is the batch's T60 error; a zero decay slope,
which divides by zero in the reference, is NaN too.  The multi-resolution
STFT term restates auraloss (absent here) exactly as the criterion does:
it is the criterion's resolutions 0-2.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from ._lib import _ptr, _stream
from .criterion import _window_table
from .renderer import _ir_twiddle

METRIC_KEYS = ("Angle", "Amplitude", "Envelope", "T60", "C50", "EDT", "multi_stft")
# columns of metric_rows()'s table (AVR_METRICS_COLS)
ROW_COLS = ("t60_ori", "t60_pred", "edt_ori", "edt_pred", "c50_ori", "c50_pred",
            "angle_sum", "amplitude_sum", "envelope_sum")

_WS: dict = {}


def _ws_bytes(B, n):
    key = (B, n)
    v = _WS.get(key)
    if v is None:
        out = ctypes.c_int64(0)
        _lib.call("avr_metrics_workspace", B, n, ctypes.byref(out))
        v = int(out.value)
        _WS[key] = v
    return v


def _rows_of(ir, name):
    if not isinstance(ir, torch.Tensor) or not ir.is_cuda:
        raise RuntimeError(f"avr_amd.metrics: {name} must be a HIP tensor (no CPU fallback)")
    if ir.dim() == 1:
        ir = ir.unsqueeze(0)
    if ir.dim() != 2:
        raise ValueError(f"{name}: expected [B, n] or [n], got {tuple(ir.shape)}")
    return ir.detach().float().contiguous()


def _run(ori_ir, pred_ir, fs, window):
    ori = _rows_of(ori_ir, "ori_ir")
    pred = _rows_of(pred_ir, "pred_ir")
    if ori.shape != pred.shape or ori.device != pred.device:
        raise ValueError(f"ori_ir {tuple(ori.shape)} and pred_ir {tuple(pred.shape)} differ")
    B, n = ori.shape
    dev = ori.device
    nbytes = _ws_bytes(B, n)  # refuses an illegal (B, n) before anything is built
    win = _window_table(dev)
    tw512 = _ir_twiddle(512, dev)
    irtw = _ir_twiddle(n, dev)
    f32 = dict(dtype=torch.float32, device=dev)
    ws = torch.empty(nbytes // 4, **f32)
    rows = torch.empty(B, len(ROW_COLS), **f32)
    means = torch.empty(7, **f32)
    ori_energy = torch.empty(B, n, **f32)
    pred_energy = torch.empty(B, n, **f32)
    s50 = int(0.05 * fs)  # metric.py:62, in double as Python does
    with torch.cuda.device(dev):
        _lib.call("avr_metrics", B, n, float(fs), s50, int(window), _ptr(ori), _ptr(pred), _ptr(irtw),
                  _ptr(win), _ptr(tw512), _ptr(rows), _ptr(means), _ptr(ori_energy), _ptr(pred_energy),
                  _ptr(ws), nbytes, _stream(dev))
    return rows, means, ori_energy, pred_energy


def metric_cal(ori_ir, pred_ir, fs=48000, window=32):
    """utils/metric.py:8-74 on the GPU; see the module docstring."""
    _, means, ori_energy, pred_energy = _run(ori_ir, pred_ir, fs, window)
    return (*means.unbind(0), ori_energy, pred_energy)


def metric_rows(ori_ir, pred_ir, fs=48000, window=32):
    """The per-row table [B, 9] behind metric_cal's means, columns ROW_COLS:
    T60, EDT and C50 of each signal, and the row's Angle, Amplitude and
    Envelope sums (over the n bins / samples; their batch metric is the sum
    over rows divided by B * n)."""
    return _run(ori_ir, pred_ir, fs, window)[0]


def calculate_metrics(criterion, pred_sig, ori_sig, fs):
    """avr_runner.py:374-407: (losses, metrics, ori_time, pred_time) with the
    runner's dictionaries; every value is a device tensor."""
    (spec_loss, amplitude_loss, angle_loss, time_loss, energy_loss, multi_stft_loss, das_reg_loss,
     das_ce_loss, ori_time, pred_time) = criterion(pred_sig, ori_sig)
    angle, amp, env, t60, edt, c50, mr, _, _ = metric_cal(ori_time, pred_time, fs=fs)
    losses = {
        'spec_loss': spec_loss,
        'fft_loss': amplitude_loss + angle_loss,
        'time_loss': time_loss,
        'energy_loss': energy_loss,
        'multi_stft_loss': multi_stft_loss,
        'das_reg_loss': das_reg_loss,
        'das_ce_loss': das_ce_loss,
    }
    metrics = {'Angle': angle, 'Amplitude': amp, 'Envelope': env, 'T60': t60, 'C50': c50,
               'EDT': edt, 'multi_stft': mr}
    return losses, metrics, ori_time, pred_time


class MetricAccumulator:
    """The validation loop's bookkeeping (avr_runner.py:265-269, 305-307) on
    the device: `add(metrics)` adds a batch's dictionary to running sums and
    keeps the per-batch values; `result()` syncs once and returns
    (avg, std): the sums over the number of batches and the population
    standard deviation (np.std) of the per-batch values, as Python floats."""

    def __init__(self, keys=METRIC_KEYS):
        self.keys = tuple(keys)
        self._sum = None
        self._batches = []

    def add(self, metrics):
        v = torch.stack([metrics[k].reshape(()).float() for k in self.keys])
        self._sum = v if self._sum is None else self._sum + v
        self._batches.append(v)

    def __len__(self):
        return len(self._batches)

    def result(self):
        if not self._batches:
            raise RuntimeError("MetricAccumulator.result(): no batch was added")
        per = torch.stack(self._batches).double()
        avg = self._sum.double() / len(self._batches)
        std = per.std(dim=0, unbiased=False)
        host = torch.stack([avg, std]).cpu()  # the one sync
        return (dict(zip(self.keys, host[0].tolist())), dict(zip(self.keys, host[1].tolist())))
