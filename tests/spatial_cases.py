"""Cases and float64 stage references for directional receivers.

A receiver pattern is a per-ray gain g[b,c,r] on the ray sum; channel c of a
C-channel ray reduction is the single-channel reduction with the weights
w*g[c], so the references here are `render_stage_cases.ref_reduce_fwd/bwd`
(imported, not edited) applied per channel and summed.  Importable without a
GPU.  `tests/golden/spatial/*.npz` (tools/gen_spatial_golden.py) hold the real
reference's renders behind a stub network that returns signal*g[c,r].
"""
from __future__ import annotations

import glob
import json
import os

import numpy as np
import torch

import render_stage_cases as rsc
from render_stage_cases import ReduceCase
from avr_amd.workloads import Workload, make_inputs
from oracle import avr_oracle as orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spatial")
U32 = rsc.U32
# relative rounding error of one store in the signal's type (half an ulp)
STORE_U = {"float32": 0.0, "float16": 2.0 ** -11, "bfloat16": 2.0 ** -8}

CHANNELS = (1, 2, 3, 4, 5, 9)  # blocks 1 | 2 | 2+1 | 4 | 4+1 | 4+4+1

# forward: 512 / 1024 threads and 1-4 chunks per lane (fp32), both 16-bit
# types, the element-wise form (S*T not a multiple of the vector width, and a
# tensor one element off 16-byte alignment); R = 7 with 1, 2 and 4 splits,
# R = 5 with 4 splits (the last one empty)
MC_FWD = (
    [ReduceCase(2, T, "float32") for T in (2046, 8194, 16384)]
    + [ReduceCase(4, T, d) for d in ("float16", "bfloat16") for T in (8190, 8194)]
    + [ReduceCase(3, 510, "float32", vector=False), ReduceCase(3, 1026, "bfloat16", vector=False),
       ReduceCase(2, 2050, "float32", vector=False, offset=1)]
)
_MC_BASE = len(MC_FWD)
MC_FWD = MC_FWD + list(rsc.CPT_EDGES)  # both sides of every chunks-per-lane boundary, splits (1, 4)
MC_FWD = MC_FWD + [ReduceCase(c.S, c.T, c.dtype, R=5, n_splits=(4,), vector=c.vector, offset=c.offset)
                   for c in MC_FWD[:_MC_BASE]]
# backward: the same shapes (R = 7; it picks its own splits) plus two short rows
MC_BWD = [c for c in MC_FWD if c.R == 7] + [ReduceCase(5, 254, "float32"), ReduceCase(3, 1022, "float32")]


def synth_gain(case: ReduceCase, C: int, per_pose: bool) -> np.ndarray:
    """fp32 gains in [-1, 1] with exact zeros (about one in five, and ray 0 of
    channel 0), [C,R] or [B,C,R]."""
    rng = rsc.case_rng("gain", case.id, C, per_pose)
    shape = (case.B, C, case.R) if per_pose else (C, case.R)
    g = rng.uniform(-1.0, 1.0, shape).astype(np.float32)
    g[rng.random(shape) < 0.2] = 0.0
    g[..., 0, 0] = 0.0
    return g


def synth_gz(case: ReduceCase, C: int) -> np.ndarray:
    return rsc.case_rng("gz", case.id, C).standard_normal((case.B, C, case.S, case.T)).astype(np.float32)


def _per_pose(gain, B):
    g = np.asarray(gain, np.float64)
    return np.broadcast_to(g, (B,) + g.shape[-2:]) if g.ndim == 2 else g


def ref_reduce_mc_fwd(x, w, delay, shift, gain, n_split):
    """(part [n_split,B,C,S,T], sum |g w x| over the live rays of the split,
    rays per split) in float64."""
    B = np.shape(x)[0]
    g = _per_pose(gain, B)
    parts, mags = [], []
    for c in range(g.shape[1]):
        wc = np.asarray(w, np.float64) * g[:, c, :, None]
        part, mag, n_r = rsc.ref_reduce_fwd(x, wc, delay, shift, n_split, with_bound=True)
        parts.append(part)
        mags.append(mag)
    return np.stack(parts, 2), np.stack(mags, 2), n_r


def ref_reduce_mc_bwd(x, gz, w, delay, shift, gain):
    """gz [B,C,S,T] -> (grad_x, grad_w, |w| sum_c |g gz| [live], sum_c |g| sum_t |gz x| [live],
    live samples per row) in float64."""
    B = np.shape(x)[0]
    g = _per_pose(gain, B)
    w64 = np.asarray(w, np.float64)
    gx = gw = mag_x = mag_w = 0.0
    for c in range(g.shape[1]):
        gx_c, gw_c, mag_c, n_live = rsc.ref_reduce_bwd(x, np.asarray(gz)[:, c], w64, delay, shift, with_bound=True)
        gc = g[:, c, :, None]
        gx = gx + gc[..., None] * gx_c
        mag_x = mag_x + np.abs(gc[..., None] * gx_c)
        gw = gw + gc * gw_c
        mag_w = mag_w + np.abs(gc) * mag_c
    return gx, gw, mag_x, mag_w, n_live


# --------------------------------------------------------------------------
# golden fixtures
# --------------------------------------------------------------------------
def render_case_names():
    names = sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(GOLDEN, "*.npz")))
    return [n for n in names if n != "patterns"]


def load_patterns():
    z = np.load(os.path.join(GOLDEN, "patterns.npz"), allow_pickle=False)
    rows = json.loads(str(z["meta"]))["rows"]
    return [(r, z[r["phi"]], z[r["key"]]) for r in rows]


class SpatialCase:
    def __init__(self, name):
        z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
        self.name = name
        self.z = {k: z[k] for k in z.files}
        m = self.meta = json.loads(str(self.z["meta"]))
        self.workload = Workload(m["workload"], dict(m["render"]), m["T"], m["batch"], with_dir_tx=m["with_dir_tx"],
                                 signal_dtype=m["signal_dtype"], attn_dtype=m["attn_dtype"])
        self.seed, self.C = m["seed"], m["channels"]

    def inputs(self):
        return make_inputs(self.workload, self.seed)

    def grad_probe(self):
        """G [B,C,F,2] of the loss sum_c <out_c, G_c> (tools/gen_spatial_golden.py)."""
        rng = np.random.default_rng(20_000 + self.seed)
        return rng.standard_normal(size=(self.workload.batch, self.C, self.workload.F, 2)).astype(np.float32)

    def has(self, key):
        return key in self.z

    def __getitem__(self, key):
        return self.z[key]


def scaled_signal(signal, gain, c, B, R):
    """The stub network's output for channel c: signal.float() * g[b,c,r]."""
    g = gain[c] if gain.dim() == 2 else gain[:, c]
    s = signal.float().view(B, R, -1, signal.size(-1))
    return (s * g.reshape(-1, R, 1, 1)).view(B, -1, signal.size(-1))


def oracle_render(case: SpatialCase):
    """(out [B,C,F,2] by the oracle on the scaled signals, its record)."""
    w, inp = case.workload, case.inputs()
    attn, signal = torch.from_numpy(inp["attn"]), torch.from_numpy(inp["signal"])
    gain = torch.from_numpy(case["gain"])
    dtx = None if inp["direction_tx"] is None else torch.from_numpy(inp["direction_tx"])
    cfg = orc.RenderConfig.from_kwargs(**w.render)
    outs, rec = [], {}
    for c in range(case.C):
        torch.manual_seed(case.seed)
        stub = orc.StubNetwork(attn, scaled_signal(signal, gain, c, w.batch, w.n_rays))
        outs.append(orc.render_spectrum(cfg, stub, torch.from_numpy(inp["rays_o"]),
                                        torch.from_numpy(inp["position_tx"]), dtx, record=rec))
    return torch.stack(outs, 1), rec, cfg
