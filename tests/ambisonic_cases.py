"""Cases and float64 references for higher-order ambisonics and the binaural
decode.  Importable without a GPU.  `tests/golden/ambisonic/c1_sh3.npz`
(tools/gen_ambisonic_golden.py) holds the real reference's renders behind a
stub network that returns signal * Y_k(dir_r), k < 16.
"""
from __future__ import annotations

import json
import math
import os

import numpy as np

import spatial_cases as sc
from render_stage_cases import ReduceCase
from avr_amd.workloads import Workload

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ambisonic")
U32 = sc.U32

CHANNELS = (1, 5, 9, 16)
# the 16-byte cases of the vector kernels' stage test (R = 7 pads a ray
# group, R = 5 with 4 splits leaves one empty), and R = 37: whole batches of
# ray groups and a ragged tail at both element sizes.  2 x 1022 halves are
# 2044 elements, no multiple of the 8 of a 16-byte vector: that shape has no
# 16-byte form, the launcher must refuse it (MC16_REFUSED), and 4 x 1022
# stands beside it so that the float16 kernel runs R = 37 too.
MC16_FWD = [c for c in sc.MC_FWD if c.vector] + [ReduceCase(2, 1022, "float32", R=37, n_splits=(1, 2)),
                                                 ReduceCase(4, 1022, "float16", R=37, n_splits=(1, 2))]
MC16_REFUSED = [ReduceCase(2, 1022, "float16", R=37, n_splits=(1, 2))]

# (fs, IR length) of the decoder tests
RATES = ((16000.0, 254), (48000.0, 1022))


class AmbisonicCase(sc.SpatialCase):
    """A fixture of tests/golden/ambisonic with SpatialCase's interface."""

    def __init__(self, name):
        z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
        self.name = name
        self.z = {k: z[k] for k in z.files}
        m = self.meta = json.loads(str(self.z["meta"]))
        self.workload = Workload(m["workload"], dict(m["render"]), m["T"], m["batch"], with_dir_tx=m["with_dir_tx"],
                                 signal_dtype=m["signal_dtype"], attn_dtype=m["attn_dtype"])
        self.seed, self.C = m["seed"], m["channels"]


def sh_reference(dirs, order=3):
    """[K, J] float64: real spherical harmonics, ACN order, SN3D weights,
    from the associated Legendre recurrence (no Condon-Shortley phase) and
    cos / sin of the azimuth: N_nm P_n^|m|(z) {cos(m phi), sin(|m| phi)},
    N_nm = sqrt((2 - [m = 0]) (n - |m|)! / (n + |m|)!)."""
    d = np.asarray(dirs, np.float64)
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    z, phi = d[:, 2], np.arctan2(d[:, 1], d[:, 0])
    s = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    P = {}
    for m in range(order + 1):
        pmm = np.ones_like(z)
        for i in range(1, m + 1):
            pmm = pmm * (2 * i - 1) * s
        P[m, m] = pmm
        if m + 1 <= order:
            P[m + 1, m] = z * (2 * m + 1) * pmm
        for n in range(m + 2, order + 1):
            P[n, m] = ((2 * n - 1) * z * P[n - 1, m] - (n + m - 1) * P[n - 2, m]) / (n - m)
    rows = []
    for n in range(order + 1):
        for m in range(-n, n + 1):
            a = abs(m)
            norm = math.sqrt((1 if m == 0 else 2) * math.factorial(n - a) / math.factorial(n + a))
            rows.append(norm * P[n, a] * (np.cos(a * phi) if m >= 0 else np.sin(a * phi)))
    return np.stack(rows)


def gauss_legendre_grid(n_z=16, n_phi=32):
    """(dirs [n_z * n_phi, 3], weights summing to 1): exact for the products
    of two harmonics up to order 3 (degree 6 in z, 6 in the azimuth)."""
    z, wz = np.polynomial.legendre.leggauss(n_z)
    phi = 2 * np.pi * np.arange(n_phi) / n_phi
    zz, pp = np.meshgrid(z, phi, indexing="ij")
    s = np.sqrt(1 - zz * zz)
    dirs = np.stack([s * np.cos(pp), s * np.sin(pp), zz], -1).reshape(-1, 3)
    w = np.repeat(wz / 2, n_phi) / n_phi
    return dirs, w


def fibonacci_sphere(n):
    """n nearly uniform unit directions [n, 3] (float64)."""
    i = np.arange(n) + 0.5
    z = 1 - 2 * i / n
    phi = np.pi * (1 + 5 ** 0.5) * i
    s = np.sqrt(1 - z * z)
    return np.stack([s * np.cos(phi), s * np.sin(phi), z], -1)


def ref_decode(dec, amb):
    """out[b,e,f] = sum_k dec[e,k,f] amb[b,k,f] in complex128, and the sum of
    the terms' magnitudes."""
    dec, amb = np.asarray(dec, np.complex128), np.asarray(amb, np.complex128)
    return np.einsum("ekf,bkf->bef", dec, amb), np.einsum("ekf,bkf->bef", np.abs(dec), np.abs(amb))


def ref_decode_adjoint(dec, grad_out):
    """grad_amb[b,k,f] = sum_e conj(dec[e,k,f]) grad_out[b,e,f], and the sum
    of the terms' magnitudes."""
    dec, g = np.asarray(dec, np.complex128), np.asarray(grad_out, np.complex128)
    return np.einsum("ekf,bef->bkf", dec.conj(), g), np.einsum("ekf,bef->bkf", np.abs(dec), np.abs(g))


def as_complex(a):
    a = np.asarray(a)
    return a[..., 0].astype(np.float64) + 1j * a[..., 1].astype(np.float64)
