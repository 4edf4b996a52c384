"""Shared pieces of the pose-gradient tests (no reference text).

* `encode64` / `encode_dx64`: the hash grid's trilinear interpolant and its
  derivative with respect to the point, evaluated in float64 on the cell the
  forward chooses (`oracle.hashgrid_oracle`'s fp32 rule for cell and frac).
* `AnalyticStub`: a small smooth network for the sampling backward's golden
  fixtures (`tools/gen_pose_grad_golden.py`, tests/golden/pose_grad).
"""
from __future__ import annotations

import os

import numpy as np
import torch

from oracle import hashgrid_oracle as hgo

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_grad")
GOLDEN_CASES = ("meshrir_c1", "raf_dir_tx")
RENDER_KEYS = ("n_samples", "near", "far", "n_azi", "n_ele", "speed", "fs", "pathloss", "xyz_min", "xyz_max")
INT_KEYS = ("n_samples", "n_azi", "n_ele")


def _locate(x, scale, frac_dtype):
    """(cell int64 [N,3], frac float64 [N,3]) of level scale: p = scale x + 0.5
    rounded to fp32 as the forward does, or kept in float64."""
    p = np.float64(scale) * np.asarray(x, np.float32).astype(np.float64) + 0.5
    if np.dtype(frac_dtype) == np.float32:
        p = p.astype(np.float32)
        cell = np.floor(p)
        frac = (p - cell).astype(np.float32).astype(np.float64)
    else:
        cell = np.floor(p)
        frac = p - cell
    return cell.astype(np.int64), frac


def _corners(cell, frac, size, res, base):
    """For k = 0..7: (omega [N,3], entry [N]) with omega_e = frac_e where bit
    e of k is set and 1 - frac_e otherwise."""
    for k in range(8):
        bits = np.array([(k >> d) & 1 for d in range(3)])
        om = np.where(bits[None, :] == 1, frac, 1.0 - frac)
        e = base + hgo._index(size, res, cell + bits[None, :])
        yield k, bits, om, e


def encode64(x, table, off, scale, res, frac_dtype=np.float32):
    """The interpolant [N, 2L] in float64."""
    table = np.asarray(table, np.float64).reshape(-1, 2)
    N, L = len(x), len(scale)
    out = np.zeros((N, 2 * L))
    for l in range(L):
        cell, frac = _locate(x, scale[l], frac_dtype)
        for _, _, om, e in _corners(cell, frac, int(off[l + 1] - off[l]), int(res[l]), int(off[l])):
            out[:, 2 * l:2 * l + 2] += om.prod(axis=1)[:, None] * table[e]
    return out


def encode_dx64(x, table, off, scale, res, g, frac_dtype=np.float32):
    """(grad_x [N,3], term_abs [N,3]) in float64:

        grad_x[i,d] = sum_l sum_f g[i, 2l+f] scale_l sum_k s_d(k) prod_{e != d} omega_e(k) table_l[e(k)][f]

    with s_d(k) = +1 where bit d of k is set and -1 otherwise; term_abs sums
    the absolute values of the same terms."""
    table = np.asarray(table, np.float64).reshape(-1, 2)
    g = np.asarray(g, np.float64)
    N, L = len(x), len(scale)
    grad = np.zeros((N, 3))
    tabs = np.zeros((N, 3))
    for l in range(L):
        cell, frac = _locate(x, scale[l], frac_dtype)
        for _, bits, om, e in _corners(cell, frac, int(off[l + 1] - off[l]), int(res[l]), int(off[l])):
            v = table[e]
            for d in range(3):
                sgn = 1.0 if bits[d] else -1.0
                w = np.float64(scale[l]) * sgn * np.prod(np.delete(om, d, axis=1), axis=1)
                for f in range(2):
                    term = w * v[:, f] * g[:, 2 * l + f]
                    grad[:, d] += term
                    tabs[:, d] += np.abs(term)
    return grad, tabs


class AnalyticStub(torch.nn.Module):
    """network_fn for the golden pose gradients, smooth in pts, tx and dir_tx:

        attn      = softplus(pts.a + tx.b + c)
        signal[t] = A sin(omega_t (pts.u + tx.v [+ dir_tx.w]) + phi_t)

    `params`: dict of arrays a, b, u, v, w [3], c, A scalars, omega, phi [T]."""

    NAMES = ("a", "b", "c", "A", "omega", "phi", "u", "v", "w")

    def __init__(self, params, dtype=torch.float32):
        super().__init__()
        for n in self.NAMES:
            self.register_buffer(n, torch.as_tensor(np.asarray(params[n]), dtype=dtype))

    @staticmethod
    def draw(rng, T):
        unit = lambda: (lambda v: v / np.linalg.norm(v))(rng.standard_normal(3))  # noqa: E731
        return dict(a=1.5 * unit(), b=0.7 * unit(), c=np.float64(0.3), A=np.float64(0.2),
                    omega=rng.uniform(0.5, 2.0, size=T), phi=rng.uniform(0, 2 * np.pi, size=T),
                    u=unit(), v=0.8 * unit(), w=0.6 * unit())

    def forward(self, pts, view, tx, dir_tx=None, ch_idx=None):
        attn = torch.nn.functional.softplus((pts * self.a).sum(-1) + (tx * self.b).sum(-1) + self.c)
        arg = (pts * self.u).sum(-1) + (tx * self.v).sum(-1)
        if dir_tx is not None:
            arg = arg + (dir_tx * self.w).sum(-1)
        signal = self.A * torch.sin(self.omega * arg.unsqueeze(-1) + self.phi)
        return attn.unsqueeze(-1), signal


def load_golden(name):
    """(render cfg dict, npz) of tests/golden/pose_grad/<name>.npz."""
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    cfg = {k: (int(z["cfg_" + k]) if k in INT_KEYS else float(z["cfg_" + k])) for k in RENDER_KEYS}
    return cfg, z


def stub_of(z, dtype=torch.float32):
    return AnalyticStub({n: z["stub_" + n] for n in AnalyticStub.NAMES}, dtype)
