"""GPU: the time-varying convolution `avr_amd.auralize.convolve_trajectory`
 against the float64 restatement of its definition
(tests/trajectory_cases.py), its bitwise properties, known answers, and the
functions built on it.  Every test prints its figures before it asserts.

Bar (the form §19b uses): max|y - y64| <= max(8 e32, 1e-6) max|y64|, with
e32 the distance of a sequential fp32 restatement from float64, computed here
by trajectory_cases.seq32 and never by the code under test.
tests/test_trajectory_cpu.py holds e32 <= 1e-5 on every case, and shows that
a wrong point costs 1e-2 or more.

Measured on MI355X (fractions of max|y64|, with the case's e32): one_point
2.4e-8 (2.4e-8), tiny_hop 3.4e-7 (3.4e-7), full_fade_group 9.2e-7 (9.2e-7),
wide17 9.7e-7 (9.7e-7), wide40 4.9e-7 (5.4e-7), rect 4.1e-7 (4.1e-7),
short_x 1.5e-7 (2.1e-7), hold_tail 5.1e-7 (5.3e-7), seam_at_block 4.2e-7
(5.2e-7), meshrir 1.5e-6 (1.6e-6); the seam impulses 2.8e-8 and 2.5e-8; every
exact test exact.
"""
import numpy as np
import pytest
import torch

import trajectory_cases as tc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


@pytest.fixture(scope="module")
def aur():
    from avr_amd import auralize

    return auralize


def _t(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # a copy: the cases' arrays are read-only


def _run(aur, name, ir=None, x=None, **over):
    ir0, x0 = tc.inputs(name)
    *_, hop, fade = tc.CASES[name]
    return aur.convolve_trajectory(_t(ir0 if ir is None else ir), _t(x0 if x is None else x),
                                   over.get("hop", hop), over.get("fade", fade))


@pytest.fixture(scope="module")
def outs(aur):
    """Every case computed once, shared by the tests below."""
    out = {name: _run(aur, name) for name in tc.NAMES}
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------ against the definition

@pytest.mark.parametrize("name", tc.NAMES)
def test_matches_the_float64_restatement(name, outs):
    P, C, Nh, L, hop, fade = tc.CASES[name]
    y64, e32 = tc.reference(name)
    y = outs[name]
    assert y.dtype == torch.float32 and tuple(y.shape) == (C, L + Nh - 1)
    y = y.cpu().numpy()
    err = np.abs(y - y64).max() / np.abs(y64).max()
    bar = max(8 * e32, 1e-6)
    print(f"trajectory {name}: err {err:.2e}, e32 {e32:.2e}, bar {bar:.2e}")
    assert np.isfinite(y).all()
    assert err <= bar


# ------------------------------------------------------ bitwise properties

def test_runs_repeat_bitwise(aur, outs):
    for name in ("tiny_hop", "wide40", "meshrir"):
        same = torch.equal(_run(aur, name), outs[name])
        print(f"{name}: second run bitwise equal: {same}")
        assert same


@pytest.mark.parametrize("name", ["wide17", "wide40"])
def test_rows_do_not_depend_on_the_other_channels(name, aur, outs):
    ir, _ = tc.inputs(name)
    C = ir.shape[1]
    full = outs[name]
    for lo, n in [(0, 1), (C - 1, 1), (0, 8), (C - 8, 8), (0, 16), (C - 16, 16)]:
        part = _run(aur, name, ir=ir[:, lo:lo + n])  # C <= 16: the 16-row kernel against the 32-row one
        same = torch.equal(part, full[lo:lo + n])
        print(f"{name}: rows {lo}..{lo + n - 1} as a batch of {n} == in the batch of {C}: {same}")
        assert same


@pytest.mark.parametrize("name", tc.NAMES)
def test_one_point_is_convolve_source(name, aur):
    ir, x = tc.inputs(name)
    for p1 in (ir[:1], ir[-1:]):
        got = _run(aur, name, ir=p1)
        want = aur.convolve_source(_t(p1[0]), _t(x))
        same = torch.equal(got, want)
        print(f"{name}: P = 1 == convolve_source: {same}")
        assert same


@pytest.mark.parametrize("name", tc.NAMES)
def test_hard_switch_between_equal_irs_is_convolve_source(name, aur):
    ir, x = tc.inputs(name)
    same_ir = np.ascontiguousarray(np.broadcast_to(ir[:1], ir.shape))
    got = _run(aur, name, ir=same_ir, fade=0)
    want = aur.convolve_source(_t(ir[0]), _t(x))
    same = torch.equal(got, want)
    print(f"{name}: fade = 0, equal IRs == convolve_source: {same}")
    assert same


def test_two_dimensional_ir_is_the_single_channel_row(aur, outs):
    for name in ("seam_at_block", "one_point"):
        ir, _ = tc.inputs(name)
        flat = _run(aur, name, ir=ir[:, 0])
        assert flat.dim() == 1 and torch.equal(flat, outs[name][0])
    ir, _ = tc.inputs("wide17")
    assert torch.equal(_run(aur, "wide17", ir=ir[:, 5]), outs["wide17"][5])


# ------------------------------------------------------------ known answers

def test_an_impulse_in_a_hold_region_returns_that_points_ir(aur):
    name = "wide17"
    P, C, Nh, L, hop, fade = tc.CASES[name]
    ir, _ = tc.inputs(name)
    for p, m in [(0, 0), (0, hop - fade - 1), (1, hop), (1, hop + 17), (2, 2 * hop), (2, L - 1)]:
        x = np.zeros(L, np.float32)
        x[m] = 1.0
        y = _run(aur, name, x=x).cpu().numpy()
        want = np.zeros_like(y)
        want[:, m:m + Nh] = ir[p]
        bad = int((y != want).sum())
        print(f"impulse at {m} (point {p}): {bad} elements differ")
        assert bad == 0


def test_an_impulse_at_a_seam_returns_the_mean_of_both_irs(aur):
    name = "seam_at_block"
    P, C, Nh, L, hop, fade = tc.CASES[name]
    ir, _ = tc.inputs(name)
    for p in range(P - 1):
        m = (p + 1) * hop - 1  # the one crossfade sample: u = 1/2
        x = np.zeros(L, np.float32)
        x[m] = 1.0
        y = _run(aur, name, x=x).cpu().numpy().astype(np.float64)
        want = np.zeros_like(y)
        want[:, m:m + Nh] = 0.5 * ir[p].astype(np.float64) + 0.5 * ir[p + 1].astype(np.float64)
        err = np.abs(y - want).max() / np.abs(want).max()
        print(f"impulse at the seam {m}: err {err:.2e}")
        assert err <= 1e-6


# ------------------------------------------------------------- built on it

def test_synth_trajectory_is_irfft_then_convolve(aur):
    from avr_amd import spectrum_to_ir

    P, C, F, L, hop, fade = 3, 8, 128, 700, 250, 100
    rng = np.random.default_rng(31)
    spec = (rng.standard_normal((P, C, F)) + 1j * rng.standard_normal((P, C, F))).astype(np.complex64)
    x = _t(rng.standard_normal(L).astype(np.float32))
    sd = _t(spec)
    got = aur.synth_trajectory(sd, x, hop, fade)
    ir = spectrum_to_ir(torch.view_as_real(sd).reshape(P * C, F, 2)).view(P, C, -1)
    want = aur.convolve_trajectory(ir, x, hop, fade)
    assert tuple(got.shape) == (C, L + 2 * (F - 1) - 1)
    assert torch.equal(got, want)
    assert torch.equal(aur.synth_trajectory(torch.view_as_real(sd), x, hop, fade), want)


def test_errors(aur):
    ir, x = torch.zeros(2, 3, 8, device=DEV), torch.zeros(16, device=DEV)
    with pytest.raises(RuntimeError, match="HIP tensor"):
        aur.convolve_trajectory(ir.cpu(), x, 4)
    with pytest.raises(RuntimeError, match="HIP tensor"):
        aur.convolve_trajectory(ir, x.cpu(), 4)
    for hop, fade in [(4, 5), (0, 0), (-2, None), (4, -1), (2.5, 1), (1 << 24, 1 << 23)]:
        with pytest.raises(ValueError):
            aur.convolve_trajectory(ir, x, hop, fade)
    for bad_ir, bad_x in [(ir[0, 0], x), (ir[None], x), (ir, x[None]), (ir[:, :, :0], x), (ir, x[:0])]:
        with pytest.raises(ValueError):
            aur.convolve_trajectory(bad_ir, bad_x, 4)
    with pytest.raises(ValueError):
        aur.synth_trajectory(torch.zeros(2, 5, dtype=torch.complex64, device=DEV), x, 4)
    assert aur.convolve_trajectory(ir, x, 4).shape == (3, 23)  # fade=None is hop


def test_captures_into_a_graph(aur, outs):
    """No sync, no device-to-host copy, no allocation outside torch's caching
    allocator: a call captures on one stream and its replay equals eager."""
    name = "full_fade_group"
    ir, x = tc.inputs(name)
    *_, hop, fade = tc.CASES[name]
    ird, xd = _t(ir), _t(x)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = aur.convolve_trajectory(ird, xd, hop, fade)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured, outs[name])


# ------------------------------------------------------------ auralize_path

class PathNet(torch.nn.Module):
    """A stub network whose outputs depend on the sample positions."""

    def __init__(self, T):
        super().__init__()
        self.freq = torch.linspace(0.5, 3.0, T, device=DEV)

    def forward(self, pts, view, tx, dir_tx=None):
        s = pts[..., 0:1] * 1.3 + pts[..., 1:2] * 0.7 - pts[..., 2:3] * 0.4 + tx[..., 0:1] * 0.2
        return s.abs() * 0.5, torch.sin(s * self.freq) * 0.1


@pytest.fixture(scope="module")
def path():
    from avr_amd import AVRRender
    from avr_amd.workloads import WORKLOADS

    w = WORKLOADS["c1_meshrir_plumbing"]
    r = AVRRender(PathNet(w.T), **w.render)
    P, L = 5, 600
    rng = np.random.default_rng(77)
    a, b = rng.uniform(-1.5, 1.5, 3), rng.uniform(-1.5, 1.5, 3)
    ro = _t(np.linspace(a, b, P).astype(np.float32))
    tx = _t(rng.uniform(-1.0, 1.0, 3).astype(np.float32))
    x = _t(rng.standard_normal(L).astype(np.float32))
    return w, r, ro, tx, x


@pytest.mark.parametrize("chunk", [1, 2, 5])
def test_auralize_path_is_the_chunks_rendered_by_hand(chunk, aur, path):
    from avr_amd.renderer import draw_jitter

    w, r, ro, tx, x = path
    P, hop, fade = ro.size(0), 120, 60
    torch.manual_seed(7)
    got = aur.auralize_path(r, ro, tx, x, hop, fade, pose_chunk=chunk)
    state = torch.get_rng_state()
    torch.manual_seed(7)
    u = draw_jitter(w.render["n_azi"], w.render["n_ele"])
    assert torch.equal(torch.get_rng_state(), state)  # one draw for the whole path
    with torch.no_grad():
        irs = [r.render_ir(ro[i:i + chunk], tx.expand(P, 3)[i:i + chunk], u_azi=u)[1] for i in range(0, P, chunk)]
    ir = torch.cat(irs)
    assert tuple(ir.shape) == (P, w.T)
    assert not torch.equal(ir[0], ir[-1])  # the IR does change along the path
    want = aur.convolve_trajectory(ir[:, None, :], x, hop, fade)
    assert tuple(got.shape) == (1, x.numel() + w.T - 1)
    assert torch.equal(got, want)
    torch.manual_seed(7)  # position_tx [P, 3] is the same path as [3]
    assert torch.equal(aur.auralize_path(r, ro, tx.expand(P, 3), x, hop, fade, pose_chunk=chunk), want)
    assert float(got.abs().max()) > 0


def test_auralize_path_with_a_directional_receiver(aur, path):
    from avr_amd import spatial
    from avr_amd.renderer import draw_jitter

    w, r, ro, tx, x = path
    torch.manual_seed(3)
    got = aur.auralize_path(r, ro, tx, x, 150, ray_gain=spatial.foa, pose_chunk=2)
    assert tuple(got.shape) == (4, x.numel() + w.T - 1)
    torch.manual_seed(3)
    u = draw_jitter(w.render["n_azi"], w.render["n_ele"])
    with torch.no_grad():
        ir = torch.cat([r.render_ir(ro[i:i + 2], tx.expand(5, 3)[i:i + 2], ray_gain=spatial.foa, u_azi=u)[1]
                        for i in range(0, 5, 2)])
    assert tuple(ir.shape) == (5, 4, w.T)
    assert torch.equal(got, aur.convolve_trajectory(ir, x, 150))


def test_forward_without_u_azi_draws_as_before(path):
    from avr_amd.renderer import draw_jitter

    w, r, ro, tx, _ = path
    txp = tx.expand(ro.size(0), 3)
    with torch.no_grad():
        torch.manual_seed(11)
        a = r(ro, txp)
        after_a = torch.get_rng_state()
        torch.manual_seed(11)
        u = draw_jitter(w.render["n_azi"], w.render["n_ele"])
        after_u = torch.get_rng_state()
        b = r(ro, txp, u_azi=u)
        assert torch.equal(torch.get_rng_state(), after_u)  # a given jitter draws nothing
        torch.manual_seed(11)
        _, ir = r.render_ir(ro, txp)
        _, ir_u = r.render_ir(ro, txp, u_azi=u)
    assert torch.equal(after_a, after_u)
    assert torch.equal(a, b)
    assert torch.equal(ir, ir_u)
