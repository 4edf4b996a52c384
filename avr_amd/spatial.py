"""Receiver patterns for `AVRRender(..., ray_gain=...)`: per-ray gains from ray directions.

A directional receiver weights ray r of output channel c with a real gain
g[c, r], constant over frequency; the renderer sums `g[c, r] * ray r` where
the omnidirectional receiver sums the rays with weight 1.  Everything here is
plain torch on [R]-sized tensors (it is not a hot path) and runs on whatever
device `dirs` lives on.  `dirs` [R, 3] are the render's unit ray directions
(x, y, z), azimuth counted from +x towards +y as in the reference's
`ray_directions` (renderer.py:133-165).

    from avr_amd import spatial
    out = renderer(rays_o, tx, ray_gain=spatial.foa)                    # [B, 4, F, 2]
    out = renderer(rays_o, tx, ray_gain=spatial.cardioid_pair(90, 110))  # [B, 2, F, 2]

Binaural output goes through spherical harmonics: `ambisonic(3)` renders 16
frequency-independent channels, and a decoder `sh_decoder(hrtf, dirs, 3)`
[2, 16, F], fitted to a head's transfer functions, turns them into two ears
per frequency bin (`AVRRender(..., sh_decoder=...)`):

    dec = spatial.sh_decoder(spatial.spherical_head_hrtf(grid, fs, T), grid, 3, fs=fs)
    out, ir = renderer.render_ir(rays_o, tx, ray_gain=spatial.ambisonic(3), sh_decoder=dec)  # [B, 2, F, 2], [B, 2, T]
"""
from __future__ import annotations

import math

import numpy as np
import torch


def azimuth(dirs):
    """Azimuth [R] of the directions in (-pi, pi], atan2(y, x)."""
    return torch.atan2(dirs[..., 1], dirs[..., 0])


def wide_cardioid_beam_pattern(facing_direction, phi, base_level=2.0):
    """The reference's `utils/spatialization.py::wide_cardioid_beam_pattern`,
    op for op: a cardioid main lobe towards `facing_direction` (radians) over
    the query azimuths `phi`, raised by `base_level` (a falsy one counts as
    1.0) and divided by its maximum over the queried `phi`."""
    main_lobe_gain = (1 + torch.cos(phi - facing_direction)) / 2
    if not base_level:
        base_level = 1.0
    gain = main_lobe_gain + base_level
    gain /= torch.max(gain)
    return gain


def _unit(v):
    return v / torch.linalg.vector_norm(v, dim=-1, keepdim=True)


def first_order(dirs, axis, alpha):
    """alpha + (1 - alpha) * <dir, axis> [R]: omnidirectional at alpha = 1,
    cardioid at 0.5, figure-of-eight at 0.  `axis` (3 values) is normalised."""
    axis = _unit(torch.as_tensor(axis, dtype=dirs.dtype, device=dirs.device))
    return alpha + (1 - alpha) * (dirs * axis).sum(-1)


def foa(dirs):
    """First-order ambisonics [4, R]: W, Y, Z, X (ACN order) with SN3D
    weights, i.e. 1 and the components of the normalised direction."""
    d = _unit(dirs)
    return torch.stack([torch.ones_like(d[..., 0]), d[..., 1], d[..., 2], d[..., 0]])


def cardioid_pair(yaw_deg, spread_deg):
    """A callable `dirs -> [2, R]` for a coincident stereo pair of horizontal
    cardioids: the pair looks along azimuth `yaw_deg`, the left capsule is
    turned `spread_deg / 2` towards +azimuth and the right one as far back."""
    def gains(dirs):
        rows = []
        for sign in (1.0, -1.0):
            a = math.radians(yaw_deg + sign * spread_deg / 2)
            rows.append(first_order(dirs, (math.cos(a), math.sin(a), 0.0), 0.5))
        return torch.stack(rows)

    return gains


# --------------------------------------------------------------------------
# higher-order ambisonics and the binaural decode
# --------------------------------------------------------------------------
def head_rotation(yaw, pitch=0.0, roll=0.0):
    """Head-to-world rotation matrices `Rz(yaw) @ Ry(pitch) @ Rx(roll)`
    (radians, right-handed; head frame +x front, +y left, +z up: a positive
    yaw turns the head to its left).  Scalars give [3, 3]; any argument with
    P entries gives [P, 3, 3] (float64)."""
    a = [torch.as_tensor(v, dtype=torch.float64).reshape(-1) for v in (yaw, pitch, roll)]
    P = max(v.numel() for v in a)
    if any(v.numel() not in (1, P) for v in a):
        raise ValueError("head_rotation: yaw, pitch and roll need one or the same number of entries")
    single = all(torch.as_tensor(v).dim() == 0 for v in (yaw, pitch, roll))
    y, p, r = (v.expand(P) for v in a)
    one, zero = torch.ones_like(y), torch.zeros_like(y)

    def mat(rows):
        return torch.stack([torch.stack(row, -1) for row in rows], -2)

    cy, sy, cp, sp, cr, sr = y.cos(), y.sin(), p.cos(), p.sin(), r.cos(), r.sin()
    rz = mat([[cy, -sy, zero], [sy, cy, zero], [zero, zero, one]])
    ry = mat([[cp, zero, sp], [zero, one, zero], [-sp, zero, cp]])
    rx = mat([[one, zero, zero], [zero, cr, -sr], [zero, sr, cr]])
    m = rz @ ry @ rx
    return m[0] if single else m


_SQ3, _SQ15, _SQ58, _SQ38 = math.sqrt(3.0), math.sqrt(15.0), math.sqrt(5.0 / 8.0), math.sqrt(3.0 / 8.0)


def _sh_rows(d, order):
    """Real spherical harmonics of the unit directions d [..., 3], ACN order,
    SN3D weights, as polynomials in (x, y, z): (order+1)^2 tensors [...]."""
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    rows = [torch.ones_like(x)]
    if order >= 1:
        rows += [y, z, x]
    if order >= 2:
        xx, yy, zz = x * x, y * y, z * z
        rows += [_SQ3 * (x * y), _SQ3 * (y * z), (3.0 * zz - 1.0) / 2.0, _SQ3 * (x * z), (_SQ3 / 2.0) * (xx - yy)]
    if order >= 3:
        rows += [_SQ58 * (y * (3.0 * xx - yy)), _SQ15 * (x * y * z), _SQ38 * (y * (5.0 * zz - 1.0)),
                 z * (5.0 * zz - 3.0) / 2.0, _SQ38 * (x * (5.0 * zz - 1.0)), (_SQ15 / 2.0) * (z * (xx - yy)),
                 _SQ58 * (x * (xx - 3.0 * yy))]
    return rows


class Ambisonic:
    """`ambisonic(order, rotation)`: a callable `dirs [R, 3] -> [K, R]`,
    K = (order+1)^2, for `ray_gain=`.  With per-pose rotations [P, 3, 3] it
    returns [P, K, R], `per_pose` is True, `len()` is P and slicing it slices
    the rotations (`auralize_path` cuts it with the poses)."""

    def __init__(self, order, rotation=None):
        if order not in (0, 1, 2, 3):
            raise ValueError(f"ambisonic: order {order!r}; 0 to 3 are supported")
        if rotation is not None:
            rotation = torch.as_tensor(rotation)
            if rotation.dim() not in (2, 3) or tuple(rotation.shape[-2:]) != (3, 3):
                raise ValueError(f"ambisonic: rotation [3, 3] or [P, 3, 3] expected, got {tuple(rotation.shape)}")
        self.order, self.rotation = order, rotation
        self.channels = (order + 1) ** 2

    @property
    def per_pose(self):
        return self.rotation is not None and self.rotation.dim() == 3

    def __len__(self):
        if not self.per_pose:
            raise TypeError("ambisonic: no per-pose rotation")
        return self.rotation.size(0)

    def __getitem__(self, idx):
        if not self.per_pose:
            raise TypeError("ambisonic: no per-pose rotation to slice")
        rot = self.rotation[idx]
        return Ambisonic(self.order, rot[None] if rot.dim() == 2 else rot)

    def __call__(self, dirs):
        d = dirs
        if self.rotation is not None:
            d = d @ self.rotation.to(device=dirs.device, dtype=dirs.dtype)  # head-frame components
        return torch.stack(_sh_rows(_unit(d), self.order), -2)


def ambisonic(order, rotation=None):
    """Ambisonics of `order` 0 to 3 as a receiver pattern: real spherical
    harmonics in ACN channel order with SN3D weights, closed-form polynomials
    in the unit ray direction (rows 0 to 3 are `foa`).  `rotation` ([3, 3], or
    [P, 3, 3] per pose; `head_rotation`) maps the head frame (+x front, +y
    left, +z up) to the world: the gains are those of `dirs @ rotation`."""
    return Ambisonic(order, rotation)


def _np64(a):
    return a.detach().cpu().double().numpy() if torch.is_tensor(a) else np.asarray(a, np.float64)


def spherical_head_hrtf(dirs, fs, n, radius=0.0875, c=343.0):
    """Transfer functions [J, 2, n//2+1] (complex128; ear 0 left at +y, ear 1
    right at -y) of a rigid spherical head for plane waves from the head-frame
    directions `dirs` [J, 3], on the bins of an n-point rfft at rate `fs`:
    the Brown-Duda structural model.  With theta the angle between the source
    and the ear's axis, w0 = c/radius: a one-pole/one-zero head shadow
    (1 + i alpha w/(2 w0)) / (1 + i w/(2 w0)), alpha = 1.05 + 0.95 cos(1.2 theta),
    and Woodworth's delay, -(a/c) cos(theta) in front of the ear and
    (a/c)(theta - pi/2) behind it, plus a/c so that every response is causal."""
    d = _np64(dirs)
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    w = 2.0 * np.pi * fs * np.arange(n // 2 + 1) / n
    tau = radius / c
    out = np.empty((d.shape[0], 2, w.size), np.complex128)
    for e, sign in enumerate((1.0, -1.0)):
        theta = np.arccos(np.clip(sign * d[:, 1], -1.0, 1.0))[:, None]
        alpha = 1.05 + 0.95 * np.cos(1.2 * theta)
        x = 0.5j * w[None, :] * tau  # i w / (2 w0)
        delay = np.where(theta < np.pi / 2, -tau * np.cos(theta), tau * (theta - np.pi / 2)) + tau
        out[:, e] = (1.0 + alpha * x) / (1.0 + x) * np.exp(-1j * w[None, :] * delay)
    return torch.from_numpy(out)


def sh_decoder(hrtf, dirs, order, method="magls", fs=None, cutoff_hz=1500.0, reg=0.0, n=None,
               dtype=torch.complex64):
    """Decoder D [E, K, F] (complex64, or `dtype`) from ambisonics of `order` to the E
    ears of `hrtf`, so that H(dir, e, f) ~ sum_k Y_k(dir) D[e, k, f] over the
    measurement directions `dirs` [J, 3] (head frame).  `hrtf` is [J, E, F]
    complex, or impulse responses [J, E, taps] (real) with the transform
    length `n`.  Solved in float64:

    * "ls": D = (Y^T Y + reg I)^-1 Y^T H, bin by bin;
    * "magls": the same below `cutoff_hz`; above it, bin by bin, the target
      keeps |H(f)| and takes the phase of the previous bin's fit Y D(f-1)
      (the ear is insensitive to phase there, and an order-3 fit of the
      complex H is not possible).  Needs `fs`."""
    if method not in ("ls", "magls"):
        raise ValueError(f"sh_decoder: method {method!r}; 'ls' or 'magls'")
    H = hrtf.detach().cpu().numpy() if torch.is_tensor(hrtf) else np.asarray(hrtf)
    if H.ndim != 3:
        raise ValueError(f"sh_decoder: hrtf [J, E, F] or [J, E, taps] expected, got {H.shape}")
    if not np.iscomplexobj(H):
        if n is None:
            raise ValueError("sh_decoder: impulse responses need the transform length n=")
        H = np.fft.rfft(H.astype(np.float64), n=n, axis=-1)
    H = H.astype(np.complex128)
    J, E, F = H.shape
    d = torch.from_numpy(_np64(dirs))
    if tuple(d.shape) != (J, 3):
        raise ValueError(f"sh_decoder: dirs [{J}, 3] expected, got {tuple(d.shape)}")
    Y = ambisonic(order)(d).numpy().T  # [J, K]
    K = Y.shape[1]
    pinv = np.linalg.solve(Y.T @ Y + reg * np.eye(K), Y.T)  # [K, J]
    D = np.einsum("kj,jef->ekf", pinv, H)
    if method == "magls":
        if fs is None:
            raise ValueError("sh_decoder: method 'magls' needs fs=")
        if F < 2:
            raise ValueError("sh_decoder: method 'magls' needs at least two bins")
        freqs = fs * np.arange(F) / (2 * (F - 1))
        for f in range(max(1, int(np.searchsorted(freqs, cutoff_hz))), F):
            fit = np.einsum("jk,ek->je", Y, D[:, :, f - 1])
            D[:, :, f] = np.einsum("kj,je->ek", pinv, np.abs(H[:, :, f]) * np.exp(1j * np.angle(fit)))
    return torch.from_numpy(D).to(dtype)
