"""Golden pose gradients of the sampling stage (build container only).

Runs the real `renderer_cpu.AVRRender` (reference import of
`tools/gen_golden.py`) behind the analytic stub network of
`tests/hashgrid_dx_cases.py` with poses that require grad, and stores what
torch autograd gives for (out * G).sum(): the gradients with respect to
rays_o, position_tx and direction_tx.  The delays and masks are rounded in
the reference and contribute nothing; the gradient flows through the network
inputs only, which is what `avr_amd.renderer._SamplePoses` implements.

A fixture is refused (the seed redrawn) unless every stored gradient is at
least 0.05 of the sum of its per-sample contributions' norms, so cancellation
between the samples of a pose cannot hide an error in a few of them.

Data-only fixtures, a few KB each: tests/golden/pose_grad/*.npz.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_pose_grad_golden.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gen_golden as gg  # noqa: E402  (puts the repository root on sys.path)

sys.path.insert(0, os.path.join(gg.REPO, "tests"))

import hashgrid_dx_cases as hdc  # noqa: E402
from avr_amd.workloads import MESHRIR, RAF  # noqa: E402

OUT = os.path.join(gg.OUT, "pose_grad")
MIN_CONDITION = 0.05
MAX_TRIES = 64

# name -> (render keys, T, B, direction_tx, pose range)
CASES = {
    "meshrir_c1": (dict(MESHRIR, n_azi=6, n_ele=5, n_samples=64), 254, 2, False, 2.0),
    "raf_dir_tx": (dict(RAF, n_azi=6, n_ele=5, n_samples=32), 254, 2, True, 1.0),
}


class _Recording(torch.nn.Module):
    """The stub, keeping the network inputs' gradients (per-sample contributions)."""

    def __init__(self, stub):
        super().__init__()
        self.stub, self.seen = stub, None

    def forward(self, pts, view, tx, dir_tx=None):
        self.seen = [t for t in (pts, tx, dir_tx) if t is not None]
        for t in self.seen:
            t.retain_grad()
        return self.stub(pts, view, tx, dir_tx)


def _draw(cfg, T, B, with_dtx, span, seed):
    rng = np.random.default_rng(50_000 + seed)
    ro = rng.uniform(-span, span, size=(B, 3)).astype(np.float32)
    tx = rng.uniform(-span, span, size=(B, 3)).astype(np.float32)
    dtx = None
    if with_dtx:
        v = rng.standard_normal(size=(B, 3))
        dtx = (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)
    stub = {k: np.asarray(v, np.float32) for k, v in hdc.AnalyticStub.draw(rng, T).items()}
    G = rng.standard_normal(size=(B, T // 2 + 1, 2)).astype(np.float32)
    return ro, tx, dtx, stub, G


def generate(name):
    cfg, T, B, with_dtx, span = CASES[name]
    ref = gg._ref_module()
    for seed in range(MAX_TRIES):
        ro, tx, dtx, stub, G = _draw(cfg, T, B, with_dtx, span, seed)
        poses = [torch.from_numpy(a).requires_grad_(True) for a in (ro, tx, dtx) if a is not None]
        net = _Recording(hdc.AnalyticStub(stub))
        torch.manual_seed(seed)
        u_azi = torch.rand(cfg["n_azi"])
        torch.manual_seed(seed)
        out = ref.AVRRender(net, **cfg)(*poses)
        (out * torch.from_numpy(G)).sum().backward()
        k = 2.0 / (cfg["xyz_max"] - cfg["xyz_min"])
        scales = (k, k, 1.0)
        cond = []
        for p, s, sc in zip(poses, net.seen, scales):
            # the pose's gradient is sc * sum_n (its network input's gradient)
            per = sc * s.grad.norm(dim=-1).sum(dim=1)
            cond.append(float((p.grad.norm(dim=-1) / per).min()))
        if min(cond) < MIN_CONDITION or not float(out.detach().abs().max()) > 0:
            print(f"{name}: seed {seed} refused (condition {min(cond):.3f})")
            continue
        store = {"cfg_" + k_: np.asarray(cfg[k_]) for k_ in hdc.RENDER_KEYS}
        store.update({"stub_" + n: v for n, v in stub.items()})
        store.update(seed=np.asarray(seed), T=np.asarray(T), u_azi=u_azi.numpy(), rays_o=ro, position_tx=tx,
                     G=G, out=out.detach().numpy(), grad_rays_o=poses[0].grad.numpy(),
                     grad_position_tx=poses[1].grad.numpy(), condition=np.asarray(cond))
        if with_dtx:
            store.update(direction_tx=dtx, grad_direction_tx=poses[2].grad.numpy())
        os.makedirs(OUT, exist_ok=True)
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **store)
        print(f"{name}: seed {seed}, condition {min(cond):.3f}, {os.path.getsize(path)} bytes")
        return
    raise SystemExit(f"{name}: no well-conditioned seed in {MAX_TRIES} tries")


if __name__ == "__main__":
    for case in sys.argv[1:] or list(CASES):
        generate(case)
