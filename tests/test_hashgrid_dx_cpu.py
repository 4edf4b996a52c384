"""CPU: the float64 statement of the hash grid's input gradient
(tests/hashgrid_dx_cases.py) that the GPU kernel is checked against, and the
entry point's declaration."""
import os
import re

import numpy as np

import hashgrid_dx_cases as hdc
from avr_amd import _lib
from avr_amd.encoding import level_layout
from oracle import hashgrid_oracle as hgo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _grid(n_levels, log2, base):
    off, scale, res = level_layout(n_levels, log2, base)
    rng = np.random.default_rng(21)
    table = rng.uniform(-1, 1, size=int(off[-1]) * 2).astype(np.float32)
    return off, scale, res, table


def test_helper_forward_matches_restatement():
    """encode64 on the fp32 cell and frac is the restatement's interpolant:
    2e-6, the fp32 corner chain's rounding."""
    off, scale, res, table = _grid(8, 14, 16)
    x = np.random.default_rng(22).uniform(0, 1, size=(512, 3)).astype(np.float32)
    ref = hgo.encode(x, table, off, scale, res)
    got = hdc.encode64(x, table, off, scale, res)
    np.testing.assert_allclose(got, ref, rtol=2e-6, atol=2e-6)


def test_analytic_derivative_matches_central_differences():
    """Formula and signs: with p kept in float64 the derivative equals central
    differences (h = 1e-6) of the float64 interpolant to 1e-6 term_abs, on a
    coarse grid with dense and hashed levels, at 64 interior points at least
    1e-3 of a cell away from every cell face of every level."""
    off, scale, res, table = _grid(4, 10, 4)
    sizes = np.diff(off)
    dense = [int(r) ** 3 <= int(s) for r, s in zip(res, sizes)]
    assert any(dense) and not all(dense)
    rng = np.random.default_rng(23)
    pts = []
    while len(pts) < 64:
        x = rng.uniform(0.05, 0.95, size=3).astype(np.float32)
        p = scale.astype(np.float64)[:, None] * x.astype(np.float64)[None, :] + 0.5
        if np.abs(p - np.round(p)).min() >= 1e-3:
            pts.append(x)
    x = np.stack(pts)
    g = rng.standard_normal(size=(64, 2 * len(scale)))
    grad, tabs = hdc.encode_dx64(x, table, off, scale, res, g, frac_dtype=np.float64)
    h = 1e-6
    fd = np.zeros_like(grad)
    for d in range(3):
        e = np.zeros(3)
        e[d] = h
        up = _encode_at(x.astype(np.float64) + e, table, off, scale, res)
        dn = _encode_at(x.astype(np.float64) - e, table, off, scale, res)
        fd[:, d] = ((up - dn) * g).sum(axis=1) / (2 * h)
    assert np.all(tabs > 0)
    assert np.all(np.abs(grad - fd) <= 1e-6 * tabs), float((np.abs(grad - fd) / tabs).max())


def _encode_at(x64, table, off, scale, res):
    """The float64 interpolant at float64 points (p never rounded)."""
    t = np.asarray(table, np.float64).reshape(-1, 2)
    out = np.zeros((len(x64), 2 * len(scale)))
    for l in range(len(scale)):
        p = np.float64(scale[l]) * x64 + 0.5
        cell = np.floor(p)
        frac = p - cell
        for _, _, om, e in hdc._corners(cell.astype(np.int64), frac, int(off[l + 1] - off[l]), int(res[l]),
                                        int(off[l])):
            out[:, 2 * l:2 * l + 2] += om.prod(axis=1)[:, None] * t[e]
    return out


def test_entry_point_is_declared_and_bound():
    text = open(os.path.join(ROOT, "include", "avr_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("avr_hashgrid_bwd_input", "avr_hashgrid_bwd_input_workspace"):
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert name in _lib.EXPORTS
