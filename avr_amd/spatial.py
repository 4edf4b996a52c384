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
"""
from __future__ import annotations

import math

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
