"""Per-pose bias + ReLU of the channel-embedding "add" networks
(`csrc/chembed.hip`): the reference's `h = layer(x) + emb[ch]; x = relu(h)`
(model.py:55-61) after each hidden layer, as one pass over the layer output
forward and one pass (plus a small fixed-order sum) backward.

`group_bias_relu` is what the model calls; it takes the HIP kernels where
they apply and the torch-op composition, in the reference's promotion order,
everywhere else (CPU tensors, `KernelOptions(chembed=False)`, shapes the
kernels refuse)."""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from ._lib import _ptr as _vp, _stream
from .options import DEFAULT

_CODES = {torch.float32: _lib.DTYPE_F32, torch.float16: _lib.DTYPE_F16, torch.bfloat16: _lib.DTYPE_BF16}


def bias_relu_fwd(y, table, idx, rows_per_group, out=None):
    """`avr_group_bias_relu_fwd`: out = round(relu(float(y) + table[idx[group]]))
    for y [N, W] (contiguous), table [C, W] fp32, idx [N / rows_per_group] int64."""
    N, W = y.shape
    if out is None:
        out = torch.empty_like(y)
    with torch.cuda.device(y.device):
        _lib.call("avr_group_bias_relu_fwd", N, W, int(rows_per_group), table.size(0), _vp(y), _CODES[y.dtype],
                  _vp(table), _vp(idx), _vp(out), _stream(y.device))
    return out


def bias_relu_bwd(gy, out, idx, rows_per_group, n_channels, g_table=None):
    """`avr_group_bias_relu_bwd`: (g, g_table) with g = threshold_backward(gy,
    out, 0) in gy's dtype and g_table [C, W] fp32 the per-channel column sums
    of g, every element stored (a given `g_table` is overwritten)."""
    N, W = gy.shape
    dev = gy.device
    g = torch.empty_like(gy)
    nb = ctypes.c_int64(0)
    _lib.call("avr_group_bias_relu_workspace", N, W, int(rows_per_group), ctypes.byref(nb))
    ws = torch.empty(max(nb.value // 4, 1), dtype=torch.float32, device=dev)
    if g_table is None:
        g_table = torch.empty(n_channels, W, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.call("avr_group_bias_relu_bwd", N, W, int(rows_per_group), int(n_channels), _vp(gy), _vp(out),
                  _CODES[gy.dtype], _vp(idx), _vp(g), _vp(ws), nb.value, _vp(g_table), _stream(dev))
    return g, g_table


class _GroupBiasReLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, table, idx, rows_per_group):
        out = bias_relu_fwd(y, table, idx, rows_per_group)
        ctx.save_for_backward(out, idx)
        ctx.meta = (rows_per_group, table.size(0))
        return out

    @staticmethod
    def backward(ctx, gy):
        out, idx = ctx.saved_tensors
        rows_per_group, C = ctx.meta
        gy = gy.to(out.dtype).contiguous()
        if gy.data_ptr() % 16:  # a contiguous view at an odd offset: the kernel loads 16-byte vectors
            gy = gy.clone()
        g, g_table = bias_relu_bwd(gy, out, idx, rows_per_group, C)
        return (g if ctx.needs_input_grad[0] else None), (g_table if ctx.needs_input_grad[1] else None), None, None


def kernel_ok(y, table, idx, rows_per_group, opts=DEFAULT):
    """The shapes `avr_group_bias_relu_*` takes (include/avr_hip.h)."""
    if not (opts.chembed and y.is_cuda and y.dim() == 2 and y.dtype in _CODES):
        return False
    N, W = y.shape
    return (0 < N < 2 ** 31 and W % 8 == 0 and 8 <= W <= 1024 and rows_per_group > 0
            and N % rows_per_group == 0 and idx.numel() * rows_per_group == N
            and y.is_contiguous() and y.data_ptr() % 16 == 0
            and table.is_cuda and table.dtype == torch.float32 and table.dim() == 2 and table.size(1) == W
            and 0 < table.size(0) <= 65535 and table.is_contiguous() and table.data_ptr() % 16 == 0
            and idx.is_cuda and idx.dtype == torch.int64 and idx.is_contiguous())


class _ReLURound(torch.autograd.Function):
    """round_dtype(relu(h)) for the fp32 sum h.  The backward selects on the
    saved rounded output, as the kernel and `_LinearReLU` do (out <= 0 -> 0):
    the two paths then pass the same gradient elements.  (A selection on h
    itself differs only where a positive fp32 sum rounds to 0 in the 16-bit
    type, where the next layer reads 0 either way.)"""

    @staticmethod
    def forward(ctx, h, dtype):
        out = torch.relu(h).to(dtype)
        ctx.save_for_backward(out)
        ctx.h_dtype = h.dtype
        return out

    @staticmethod
    def backward(ctx, gy):
        (out,) = ctx.saved_tensors
        return torch.ops.aten.threshold_backward(gy.to(out.dtype), out, 0).to(ctx.h_dtype), None


def bias_relu_torch(y, table, idx, rows_per_group):
    """The same step by torch ops in the reference's promotion order: the
    16-bit layer output plus the gathered fp32 embedding row is an fp32 sum,
    ReLU runs on it, and the next layer's input is rounded to y's dtype."""
    G = idx.numel()
    h = y.reshape(G, rows_per_group, y.size(-1)) + table[idx].unsqueeze(1)
    return _ReLURound.apply(h, y.dtype).reshape(y.shape)


def group_bias_relu(y, table, idx, rows_per_group, opts=DEFAULT):
    """relu(y + table[idx[row // rows_per_group]]) in y's dtype for y [N, W],
    table [C, W] fp32 and idx [N / rows_per_group] int64; differentiable in y
    and table (table.grad is fp32)."""
    if kernel_ok(y, table, idx, rows_per_group, opts):
        return _GroupBiasReLU.apply(y, table, idx, int(rows_per_group))
    return bias_relu_torch(y, table, idx, int(rows_per_group))
