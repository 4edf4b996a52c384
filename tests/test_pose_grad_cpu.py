"""CPU: the oracle's autograd reproduces the reference's pose gradients.

tests/golden/pose_grad/*.npz hold what torch autograd through the
reference's `renderer_cpu.AVRRender` gives for (out * G).sum() behind the
analytic stub network (tools/gen_pose_grad_golden.py).  The same stub through
`oracle.avr_oracle.render_spectrum` must give the same gradients: relative L2
per pose at most 1e-5, 10x under the 1e-4 the GPU test holds the renderer to.

Measured floor (fp32 CPU, both cases, every pose): 0 for the spectrum and for
every gradient; the oracle restates the reference's operations in the
reference's order, and its autograd graph gives the same bits."""
import numpy as np
import pytest
import torch

import hashgrid_dx_cases as hdc
from oracle import avr_oracle as orc

BOUND = 1e-5


def rel_l2_rows(got, ref):
    return np.linalg.norm(got - ref, axis=-1) / np.linalg.norm(ref, axis=-1)


@pytest.mark.parametrize("name", hdc.GOLDEN_CASES)
def test_oracle_autograd_reproduces_reference_pose_gradients(name):
    cfg, z = hdc.load_golden(name)
    names = ["rays_o", "position_tx"] + (["direction_tx"] if "direction_tx" in z.files else [])
    poses = [torch.from_numpy(z[n]).requires_grad_(True) for n in names]
    torch.manual_seed(int(z["seed"]))
    rec = {}
    out = orc.render_spectrum(orc.RenderConfig.from_kwargs(**cfg), hdc.stub_of(z), *poses, record=rec)
    np.testing.assert_array_equal(rec["u_azi"].numpy(), z["u_azi"])
    (out * torch.from_numpy(z["G"])).sum().backward()
    err_out = float(np.linalg.norm(out.detach().numpy() - z["out"]) / np.linalg.norm(z["out"]))
    print(f"pose grad cpu {name}: out rel l2 {err_out:.3e}")
    assert err_out <= BOUND
    for n, p in zip(names, poses):
        ref = z["grad_" + n]
        assert np.all(np.linalg.norm(ref, axis=-1) > 0)
        err = rel_l2_rows(p.grad.numpy(), ref)
        print(f"pose grad cpu {name}: grad_{n} rel l2 per pose {err}")
        assert np.all(err <= BOUND), (n, err)


@pytest.mark.parametrize("name", hdc.GOLDEN_CASES)
def test_fixture_is_well_conditioned(name):
    """The generator's own rule, stored with the fixture: each gradient is at
    least 0.05 of the sum of its per-sample contributions' norms."""
    _, z = hdc.load_golden(name)
    assert float(z["condition"].min()) >= 0.05
