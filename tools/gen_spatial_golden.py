"""Golden vectors for directional receivers (build container only).

A receiver pattern is a per-ray gain g[c, r] on the ray sum.  The signal
enters the reference's render linearly (after the masks, before the rFFT, the
weights and the sum over rays), so the reference renderer run behind a stub
network that returns `signal.float() * g[c, r]` is by definition channel c of
the gain-weighted render.  Like `tools/gen_golden.py` (whose reference import
and digest helpers are reused) this runs the real `renderer_cpu.AVRRender`
and `utils/spatialization.wide_cardioid_beam_pattern` on seeded inputs,
refuses a case unless the repository's oracle reproduces the reference bit
for bit on the same scaled signal, and writes data-only fixtures to
`tests/golden/spatial/*.npz`.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_spatial_golden.py [case ...]
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gen_golden as gg  # noqa: E402  (puts the repository root on sys.path)

from avr_amd import spatial  # noqa: E402
from avr_amd.workloads import RAF, WORKLOADS, Workload, make_inputs  # noqa: E402
from oracle import avr_oracle as orc  # noqa: E402

OUT = os.path.join(gg.OUT, "spatial")
C1 = WORKLOADS["c1_meshrir_plumbing"]  # R = 32, S = 64, T = 254

PATTERN_BASE_LEVELS = (2.0, 0, 0.5)
PATTERN_N = (6, 73)
PATTERN_FACING = (0, 2.1)


def _ref_pattern():
    gg._ref_module()  # the reference's root on sys.path
    from utils import spatialization  # noqa: WPS433  (reference, container only)
    return spatialization.wide_cardioid_beam_pattern


def gain_foa(w, seed, dirs, inp):
    return spatial.foa(dirs)


def gain_pair(w, seed, dirs, inp):
    """The reference's pattern as a 2-channel pair, facing per pose: [B,2,R]."""
    pattern = _ref_pattern()
    phi = spatial.azimuth(dirs)
    rng = np.random.default_rng(31_000 + seed)
    facing = rng.uniform(-np.pi, np.pi, size=w.batch)
    return torch.stack([torch.stack([pattern(float(f) + 0.6, phi), pattern(float(f) - 0.6, phi)])
                        for f in facing])


def gain_random5(w, seed, dirs, inp):
    """Five channels of gains in [-1, 1] with exact zeros and an all-ones row."""
    rng = np.random.default_rng(32_000 + seed)
    g = rng.uniform(-1.0, 1.0, size=(5, w.n_rays)).astype(np.float32)
    g[rng.random(g.shape) < 0.2] = 0.0
    g[3] = 1.0
    return torch.from_numpy(g)


CASES = {
    "c1_foa": (C1.replace(batch=2), 11, gain_foa),
    "c1_pair": (C1.replace(batch=2), 12, gain_pair),
    "c1_pair_fp16": (C1.replace(batch=2, signal_dtype="float16"), 13, gain_pair),
    "raf_c5": (Workload("raf_block_c5", dict(RAF, n_azi=6, n_ele=3, n_samples=5, far=2), 130, 2,
                        with_dir_tx=True), 14, gain_random5),
}


def spatial_grad_probe(w, C, seed):
    """Fixed upstream gradient G [B,C,F,2] of the loss sum_c <out_c, G_c>."""
    rng = np.random.default_rng(20_000 + seed)
    return rng.standard_normal(size=(w.batch, C, w.F, 2)).astype(np.float32)


def scaled_signal(signal, gain, c, B, R):
    """signal [B,R*S,T] (any float dtype) -> float32 * g[b,c,r]."""
    g = gain[c] if gain.dim() == 2 else gain[:, c]  # [R] or [B,R]
    s = signal.float().view(B, R, -1, signal.size(-1))
    return (s * g.reshape(-1, R, 1, 1)).view(B, -1, signal.size(-1))


def run_case(name, w, seed, gain_fn):
    rc = gg._ref_module()
    inp = make_inputs(w, seed)
    rays_o = torch.from_numpy(inp["rays_o"])
    tx = torch.from_numpy(inp["position_tx"])
    dtx = None if inp["direction_tx"] is None else torch.from_numpy(inp["direction_tx"])
    attn = torch.from_numpy(inp["attn"]).requires_grad_(True)
    signal = torch.from_numpy(inp["signal"]).requires_grad_(True)
    B, R = w.batch, w.n_rays

    torch.manual_seed(seed)
    dirs_ref, _, _ = rc.ray_directions(w.render["n_azi"], w.render["n_ele"])
    gain = gain_fn(w, seed, dirs_ref, inp).float().contiguous()
    C = gain.size(-2)
    G = torch.from_numpy(spatial_grad_probe(w, C, seed))

    # one cast for all channels: autograd then sums the channels' gradients in
    # fp32 and rounds a 16-bit signal's gradient once (a cast per channel would
    # round every channel's share and add them in the 16-bit type)
    signal_f = signal.float()
    outs, loss, rec = [], 0.0, {}
    for c in range(C):
        stub = orc.StubNetwork(attn, scaled_signal(signal_f, gain, c, B, R))
        torch.manual_seed(seed)
        ref = rc.AVRRender(stub, **w.render)
        out_c = ref(rays_o, tx, dtx) if dtx is not None else ref(rays_o, tx)
        loss = loss + (out_c * G[:, c]).sum()
        # the oracle on the same scaled signal: bit for bit, or no fixture
        torch.manual_seed(seed)
        stub2 = orc.StubNetwork(attn.detach(), scaled_signal(signal.detach(), gain, c, B, R))
        out_orc = orc.render_spectrum(orc.RenderConfig.from_kwargs(**w.render), stub2, rays_o, tx, dtx, record=rec)
        if not (torch.equal(out_orc, out_c.detach()) and torch.equal(rec["dirs"], dirs_ref)):
            raise SystemExit(f"{name}: oracle differs from the reference in channel {c} "
                             f"(max |d out| = {(out_orc - out_c.detach()).abs().max().item()})")
        outs.append(out_c.detach())
    loss.backward()
    out = torch.stack(outs, 1)  # [B,C,F,2]
    ir = torch.stack([orc.spectrum_to_ir(o) for o in outs], 1)

    store = {}
    gg._digest("grad_attn", attn.grad, seed, store)
    if "grad_attn" not in store:
        store["grad_attn"] = attn.grad.numpy()
    gg._digest("grad_signal", signal.grad.float(), seed, store)
    store["grad_signal_dot_signal"] = np.array(
        (signal.grad.double() * signal.detach().double()).sum().item())
    dl = rec["delay"].detach()
    meta = dict(case=name, workload=w.name, render=w.render, T=w.T, batch=w.batch,
                with_dir_tx=w.with_dir_tx, signal_dtype=w.signal_dtype, attn_dtype=w.attn_dtype,
                seed=seed, grads=True, channels=C, torch=torch.__version__)
    store.update(meta=np.array(json.dumps(meta)), u_azi=rec["u_azi"].numpy(), dirs=dirs_ref.numpy(),
                 gain=gain.numpy(), out=out.numpy(), ir=ir.numpy(), delay=dl.numpy().astype(np.int16))
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **store)
    print(f"{name}: ok, C={C} ({os.path.getsize(path) / 1024:.1f} KiB)", flush=True)


def run_patterns():
    """wide_cardioid_beam_pattern of the reference on jittered azimuth grids."""
    pattern = _ref_pattern()
    store, rows = {}, []
    for n in PATTERN_N:
        torch.manual_seed(n)
        phi = torch.linspace(0, np.pi * 2, n + 1)[:-1] + (np.pi * 2 / n) * torch.rand(n)
        store[f"phi_{n}"] = phi.numpy()
        for bi, base in enumerate(PATTERN_BASE_LEVELS):
            for fi, facing in enumerate(PATTERN_FACING):
                key = f"gain_{n}_{bi}_{fi}"
                store[key] = pattern(facing, phi, base_level=base).numpy()
                rows.append(dict(key=key, phi=f"phi_{n}", base_level=base, facing=facing))
    store["meta"] = np.array(json.dumps(dict(rows=rows, torch=torch.__version__)))
    path = os.path.join(OUT, "patterns.npz")
    np.savez_compressed(path, **store)
    print(f"patterns: ok, {len(rows)} rows ({os.path.getsize(path) / 1024:.1f} KiB)", flush=True)


def main(argv):
    os.makedirs(OUT, exist_ok=True)
    names = argv or ["patterns"] + list(CASES)
    for n in names:
        if n == "patterns":
            run_patterns()
        else:
            run_case(n, *CASES[n])


if __name__ == "__main__":
    main(sys.argv[1:])
