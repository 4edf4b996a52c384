"""GPU: the hash grid's input gradient (avr_hashgrid_bwd_input) against the
float64 statement of tests/hashgrid_dx_cases.py.

Bound: |grad_x - ref| <= 1e-4 term_abs + 1e-30 with term_abs the sum of the
absolute values of all terms of a component.  Derived: a component is about
340 rounded fp32 operations at 20 levels (per level 8 corners x (2 weight
products, 2 for g.v, 1 fma) + the scale and the level sum), so the forward
error bound is gamma ~ 340 x 2^-24 ~ 2e-5 of term_abs; 1e-4 is 5x that.  For
fp16 encodings the reference reads the fp16-rounded table and gradient (the
kernel upcasts both exactly and rounds no weight to half)."""
import ctypes

import numpy as np
import pytest
import torch

import hashgrid_dx_cases as hdc
from avr_amd import _lib
from avr_amd.encoding import HashGridEncoding, _code
from avr_amd.model import _unit
from avr_amd.options import KernelOptions
from oracle import hashgrid_oracle as hgo
from test_gpu_hashgrid import CFG, _points

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SMALL = dict(CFG, n_levels=8, log2_hashmap_size=14)


def _enc(cfg, dtype, seed, **kw):
    enc = HashGridEncoding(3, cfg, dtype=dtype, seed=seed, **kw).to(DEV)
    with torch.no_grad():
        enc.params.uniform_(-1, 1)
    return enc


def _grad_x(enc, x_host, g_host):
    """(x.grad, the gradient values the kernel read) of out.backward(g)."""
    x = torch.from_numpy(x_host).to(DEV).requires_grad_(True)
    out = enc(x)
    g = torch.from_numpy(g_host).to(DEV).to(out.dtype)
    out.backward(g)
    assert x.grad.dtype == torch.float32 and x.grad.shape == x.shape
    return x.grad, g.float().cpu().numpy()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("cfg,n", [(SMALL, 2048), (CFG, 20000)], ids=["small", "full"])
def test_input_gradient_matches_float64(cfg, n, dtype):
    enc = _enc(cfg, dtype, 31)
    x = _points(n, 3)
    g = np.random.default_rng(32).standard_normal(size=(n, enc.n_output_dims)).astype(np.float32)
    got, g_used = _grad_x(enc, x, g)
    table = enc.params.detach().to(enc.param_dtype).float().cpu().numpy()
    ref, tabs = hdc.encode_dx64(x, table, enc._off, enc._scale, enc._res, g_used)
    err = np.abs(got.double().cpu().numpy() - ref)
    print(f"hashgrid dx {dtype} n={n}: max err / term_abs {float((err / (tabs + 1e-300)).max()):.3e}")
    assert np.isfinite(err).all()
    assert np.all(err <= 1e-4 * tabs + 1e-30)
    assert np.abs(ref).max() > 0


@pytest.mark.parametrize("impl", ["partitioned", "atomic"])
def test_repeatable_and_table_gradient_unchanged(impl):
    enc = _enc(SMALL, torch.float32, 33, options=KernelOptions(hashgrid_bwd=impl))
    x = _points(2048, 1)
    g = np.random.default_rng(2).standard_normal(size=(2048, enc.n_output_dims)).astype(np.float32)
    a, _ = _grad_x(enc, x, g)
    ref = hgo.encode_backward(x, g, enc._off, enc._scale, enc._res, enc.n_params)
    np.testing.assert_allclose(enc.params.grad.cpu().numpy(), ref, rtol=1e-5, atol=1e-5)
    enc.params.grad = None
    b, _ = _grad_x(enc, x, g)
    assert torch.equal(a, b)
    assert float(a.abs().max()) > 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_no_input_gradient_requested_is_the_plain_path(dtype):
    """x without requires_grad: no gradient for x, nothing kept for one, and
    the output of the forward entry point called directly, bit for bit."""
    enc = _enc(SMALL, dtype, 34)
    x = torch.from_numpy(_points(2048, 4)).to(DEV)
    out = enc(x)
    assert out.grad_fn.table is None
    out.backward(torch.ones_like(out))
    assert x.grad is None and enc.params.grad is not None
    table = enc.table(False)
    raw = torch.empty_like(out)
    _lib.call("avr_hashgrid_fwd", x.size(0), enc.n_levels, x.data_ptr(), table.data_ptr(), _code(table.dtype),
              *enc.level_meta(), raw.data_ptr(), _code(raw.dtype), torch.cuda.current_stream(DEV).cuda_stream)
    assert torch.equal(out.detach(), raw)
    # and with x requiring grad the forward and the table gradient are the same
    gp = enc.params.grad.clone()
    enc.params.grad = None
    xg = x.clone().requires_grad_(True)
    out2 = enc(xg)
    out2.backward(torch.ones_like(out2))
    assert torch.equal(out2.detach(), raw)
    # (2048 points add with fp32 atomics, whose order is not fixed)
    torch.testing.assert_close(enc.params.grad, gp, rtol=1e-5, atol=1e-5)


def test_through_unit_map_halves_exactly():
    enc = _enc(SMALL, torch.float32, 35)
    u = torch.from_numpy(_points(2048, 5)).to(DEV)
    g = torch.randn(2048, enc.n_output_dims, device=DEV, generator=torch.Generator(device=DEV).manual_seed(36))
    x = (u * 2 - 1).requires_grad_(True)
    xu = _unit(x.detach()).requires_grad_(True)
    enc(xu).backward(g)
    enc(_unit(x)).backward(g)
    assert torch.equal(x.grad, 0.5 * xu.grad)
    assert float(x.grad.abs().max()) > 0


def test_frozen_grid_returns_only_the_input_gradient():
    enc = _enc(SMALL, torch.float32, 37)
    x = _points(2048, 6)
    g = np.random.default_rng(7).standard_normal(size=(2048, enc.n_output_dims)).astype(np.float32)
    a, _ = _grad_x(enc, x, g)
    enc.params.grad = None
    enc.params.requires_grad_(False)
    b, _ = _grad_x(enc, x, g)
    assert enc.params.grad is None and torch.equal(a, b)


def test_entry_point_refuses_a_small_workspace():
    enc = _enc(SMALL, torch.float32, 38)
    n = 64
    x = torch.from_numpy(_points(n, 8)).to(DEV)
    g = torch.zeros(n, enc.n_output_dims, device=DEV)
    gx = torch.zeros(n, 3, device=DEV)
    nb = ctypes.c_int64()
    _lib.call("avr_hashgrid_bwd_input_workspace", n, enc.n_levels, ctypes.byref(nb))
    assert nb.value >= n * enc.n_levels * 12
    ws = torch.empty(nb.value, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="workspace too small"):
        _lib.call("avr_hashgrid_bwd_input", n, enc.n_levels, x.data_ptr(), enc.params.data_ptr(), _code(torch.float32),
                  g.data_ptr(), _code(g.dtype), *enc.level_meta(), gx.data_ptr(), ws.data_ptr(),
                  n * enc.n_levels * 12 - 1, torch.cuda.current_stream(DEV).cuda_stream)
