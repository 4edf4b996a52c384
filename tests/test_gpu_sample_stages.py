"""GPU: the stage in front of the render core against the oracle's own
functions (tests/sample_stage_cases.py): the resident tables and twiddles,
the ray directions, and the network inputs of every entry path of
`AVRRender.sample`, compared as full arrays.

Tolerances (what each is measured against):
  d_vals, frac, shift, pl      oracle, fp32 op for op            equal
  phase                        oracle.phase_rotation             abs <= 2^-23
  twiddle, ir twiddle          float64, rounded once             abs <= 2^-24
  dirs                         oracle.sphere_directions, same u  abs <= 5e-7
  pts, view, tx, dir_tx        oracle.network_inputs on the kernel's own
                               dirs / d_vals                     equal
  entry paths, shard slices    each other                        equal

Every output buffer starts as NaN and must come back without one.  Run with
`pytest -s` for the measured figures (lines starting with SAMPLE-STAGE)."""
import ctypes
import functools
from unittest import mock

import numpy as np
import pytest
import torch

import sample_stage_cases as ssc

from avr_amd import AVRRender, _lib
from avr_amd.renderer import get_tables, ray_directions, render_params

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NET = ("pts", "view", "tx", "dir_tx")


def _st():
    return torch.cuda.current_stream().cuda_stream


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def _report(what, *figures):
    print("SAMPLE-STAGE |", what, "|", " | ".join(str(f) for f in figures))


def _spacings(got, ref):
    """max |got - ref| in units of the fp32 spacing at ref"""
    d = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    return float((d / np.spacing(np.maximum(np.abs(ref), np.float32(1e-30)))).max()) if d.size else 0.0


def _same(got, ref, what):
    """Bit for bit, every element written."""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert not np.isnan(got).any(), f"{what}: elements the stage owns were not written"
    np.testing.assert_array_equal(got, ref, err_msg=what)


# ------------------------------------------------------------------ tables
@functools.lru_cache(maxsize=None)
def _device_tables(case):
    """avr_tables / avr_ir_twiddle / avr_depth_samples into NaN-filled buffers -> host arrays."""
    p = render_params(case.cfg(), case.T)
    S, T = case.S, case.T
    F = T // 2 + 1
    n = 2 * (F - 1)
    d_vals, frac, pl, phase, tw = _nan(S), _nan(S), _nan(p.pl_len), _nan(S, F, 2), _nan(T, 2)
    shift = torch.full((S,), -12345, dtype=torch.int32, device=DEV)
    irtw, depth = _nan(n, 2), _nan(S)
    _lib.call("avr_tables", ctypes.byref(p), d_vals.data_ptr(), frac.data_ptr(), shift.data_ptr(), pl.data_ptr(),
              phase.data_ptr(), tw.data_ptr(), _st())
    _lib.call("avr_ir_twiddle", n, irtw.data_ptr(), _st())
    _lib.call("avr_depth_samples", ctypes.byref(p), depth.data_ptr(), _st())
    torch.cuda.synchronize()
    assert p.pl_len == case.pl_len and p.near_clamp == case.near_n
    got = dict(d_vals=d_vals, frac=frac, shift=shift, pl=pl, phase=phase, twiddle=tw, ir_twiddle=irtw, depth=depth)
    return p, {k: v.cpu().numpy() for k, v in got.items()}


@functools.lru_cache(maxsize=None)
def _table_refs(case):
    return ssc.table_references(case)


@pytest.mark.parametrize("case", ssc.TABLE_CASES, ids=ssc.run_id)
def test_depth_delay_and_path_loss_tables_equal_the_oracle(case):
    """d_vals, frac, shift and pl bit for bit (the device's fp32 division is
    correctly rounded: frac and pl measured 0 spacings off on every case);
    avr_depth_samples equals the table's d_vals."""
    _, got = _device_tables(case)
    ref = _table_refs(case)
    _report("tables " + case.id, "frac spacings", _spacings(got["frac"], ref["frac"]),
            "pl spacings", _spacings(got["pl"], ref["pl"]), "pl via", "oracle" if case.copy_in_range else "formula")
    for k in ("d_vals", "frac", "pl"):
        _same(got[k], ref[k], k)
    np.testing.assert_array_equal(got["shift"], ref["shift"])
    _same(got["depth"], got["d_vals"], "avr_depth_samples")


@pytest.mark.parametrize("case", ssc.TABLE_CASES, ids=ssc.run_id)
def test_phase_table_matches_the_oracle(case):
    """exp(i theta) with theta = fp32(fp32(c f) frac[s]) as the reference
    rounds it; an angle formed in double is 6e-5 to 1e-4 away."""
    _, got = _device_tables(case)
    ref = _table_refs(case)["phase"]
    assert got["phase"].shape == ref.shape and not np.isnan(got["phase"]).any()
    err = float(np.abs(got["phase"].astype(np.float64) - ref).max())
    _report("phase " + case.id, "max abs", err, "bound", ssc.PHASE_ATOL)
    assert err <= ssc.PHASE_ATOL


@pytest.mark.parametrize("case", ssc.TABLE_CASES, ids=ssc.run_id)
def test_twiddles_match_float64(case):
    """(cos, -sin)(2 pi k / T) of avr_tables and (cos, +sin)(2 pi k / n) of avr_ir_twiddle."""
    _, got = _device_tables(case)
    n = 2 * (case.T // 2)
    for name, ref in (("twiddle", ssc.twiddle_reference(case.T, -1.0)), ("ir_twiddle", ssc.twiddle_reference(n, 1.0))):
        assert got[name].shape == ref.shape and not np.isnan(got[name]).any()
        err = float(np.abs(got[name].astype(np.float64) - ref).max())
        _report(name + " " + case.id, "max abs", err, "bound", ssc.TWIDDLE_ATOL)
        assert err <= ssc.TWIDDLE_ATOL, name


@pytest.mark.parametrize("case", ssc.TABLE_CASES, ids=ssc.run_id)
def test_get_tables_holds_what_avr_tables_writes(case):
    p, got = _device_tables(case)
    tb = get_tables(p, DEV)
    torch.cuda.synchronize()
    for k in ("d_vals", "frac", "shift", "pl", "phase", "twiddle"):
        _same(getattr(tb, k).cpu().numpy(), got[k], k)
    assert tb.ir_n == got["ir_twiddle"].shape[0]
    _same(tb.ir_twiddle[:tb.ir_n].cpu().numpy(), got["ir_twiddle"], "ir_twiddle")
    assert tb.max_shift == int(got["shift"].max())


# ------------------------------------------------------------------ sampling
def _nan_empty():
    """torch.empty that hands out NaN (floating) buffers: an element sample()
    leaves unwritten cannot look like the value another route left in a
    recycled block."""
    real = torch.empty

    def empty(*a, **kw):
        t = real(*a, **kw)
        return t.fill_(float("nan")) if t.is_floating_point() else t

    return mock.patch.object(torch, "empty", empty)


@functools.lru_cache(maxsize=None)
def _sample(case, with_dtx, route, ray_range=None):
    """AVRRender.sample through one route -> host arrays (pts, view, tx, dir_tx, dirs[, pose_out]).
    Routes: "host" (u_azi a CPU tensor: the fused launch, or the three-launch
    fallback above AVR_MAX_AZI), "dev" (u_azi a HIP tensor), "staged"."""
    ro, tx, dtx = ssc.poses(case, with_dtx)
    u = ssc.jitter(case)
    r = AVRRender(None, **case.cfg())
    r.ray_range = ray_range
    pose_out = None
    with _nan_empty():
        if route == "staged":
            blk = ssc.staged_block(ro, tx, dtx, u).to(DEV)
            pose_out = _nan(9 * case.B)
            r._staged = (blk.data_ptr(), pose_out)
            try:
                out = r.sample(ro, tx, dtx)
                torch.cuda.synchronize()
            finally:
                r._staged = None
        else:
            out = r.sample(ro.to(DEV), tx.to(DEV), None if dtx is None else dtx.to(DEV),
                           u_azi=u.to(DEV) if route == "dev" else u)
            torch.cuda.synchronize()
    pts, view, txn, dtxn, geom = out
    res = dict(pts=pts, view=view, tx=txn, dir_tx=dtxn, dirs=geom["dirs"], pose_out=pose_out,
               geom_ro=geom["rays_o"], geom_tx=geom["position_tx"])
    assert geom["B"] == case.B and geom["n_rays"] == (case.R if ray_range is None else ray_range[1] - ray_range[0])
    return {k: None if v is None else v.cpu().numpy() for k, v in res.items()}


@functools.lru_cache(maxsize=None)
def _d_vals(case):
    tb = get_tables(render_params(case.cfg(), 2), DEV)
    torch.cuda.synchronize()
    return tb.d_vals.cpu()


def _check_against_references(case, with_dtx, got, rays=None):
    """dirs against the oracle's for the same draw; the network inputs against
    the oracle's on the kernel's own dirs and d_vals."""
    r0, r1 = rays if rays is not None else (0, case.R)
    ro, tx, dtx = ssc.poses(case, with_dtx)
    ref_dirs = ssc.sphere_directions_for(case.n_azi, case.n_ele, ssc.jitter(case)).numpy()[r0:r1]
    dirs = got["dirs"]
    assert dirs.shape == ref_dirs.shape and not np.isnan(dirs).any()
    err = float(np.abs(dirs - ref_dirs).max())
    np.testing.assert_allclose(dirs, ref_dirs, rtol=0, atol=ssc.DIRS_ATOL)
    if r1 > case.R - 2:  # the poles are exact
        np.testing.assert_array_equal(dirs[max(case.R - 2, r0) - r0:], ref_dirs[max(case.R - 2, r0) - r0:])
    ref = ssc.network_input_reference(case, ro, tx, dtx, torch.from_numpy(dirs), _d_vals(case))
    assert (got["dir_tx"] is None) == (not with_dtx) == (ref[3] is None)
    for k, want in zip(NET, ref):
        if want is not None:
            _same(got[k], want, f"{case.name} {k}")
    return err


@pytest.mark.parametrize("case,with_dtx", ssc.SAMPLE_RUNS, ids=ssc.run_id)
def test_directions_and_network_inputs_match_the_oracle(case, with_dtx):
    """The default entry (fused launch; three launches for `wide`): dirs
    within 5e-7 with exact poles, pts / view / tx / dir_tx bit for bit."""
    got = _sample(case, with_dtx, "host")
    err = _check_against_references(case, with_dtx, got)
    _report("dirs " + case.name, "max abs", err, "bound", ssc.DIRS_ATOL)
    assert got["pts"].shape == (case.B, case.R * case.S, 3)


@pytest.mark.parametrize("case,with_dtx", [(c, d) for c, d in ssc.SAMPLE_RUNS if c.fused], ids=ssc.run_id)
def test_entry_paths_agree(case, with_dtx):
    """Host jitter, device jitter and the staged block: one kernel, so every
    output is bit-identical, and the staged route publishes the pose."""
    host, dev, staged = (_sample(case, with_dtx, route) for route in ("host", "dev", "staged"))
    for k in NET + ("dirs",):
        if host[k] is None:
            assert k == "dir_tx" and not with_dtx and dev[k] is None and staged[k] is None
            continue
        _same(dev[k], host[k], f"{case.name} dev {k}")
        _same(staged[k], host[k], f"{case.name} staged {k}")
    ro, tx, dtx = ssc.poses(case, with_dtx)
    B = case.B
    po = staged["pose_out"]
    _same(po[:3 * B], ro.numpy().reshape(-1), "pose_out rays_o")
    _same(po[3 * B:6 * B], tx.numpy().reshape(-1), "pose_out position_tx")
    if with_dtx:
        _same(po[6 * B:], dtx.numpy().reshape(-1), "pose_out direction_tx")
    else:
        assert np.isnan(po[6 * B:]).all()  # untouched
    _same(staged["geom_ro"], ro.numpy(), "geom rays_o")
    _same(staged["geom_tx"], tx.numpy(), "geom position_tx")


@pytest.mark.parametrize("with_dtx", ssc.SAMPLE_BY_NAME["wide"].dir_tx, ids=ssc.run_id)
def test_fused_kernel_above_max_azi_through_the_device_entry(with_dtx):
    """avr_sample_rays_dev has no n_azi cap: on `wide` it meets the same
    references as the three-launch fallback (separate kernels; on the device
    the two were bit-equal in every output)."""
    case = ssc.SAMPLE_BY_NAME["wide"]
    ro, tx, dtx = ssc.poses(case, with_dtx)
    B, R, S = case.B, case.R, case.S
    p = render_params(case.cfg(), 2)
    ro_d, tx_d, u_d = ro.to(DEV), tx.to(DEV), ssc.jitter(case).to(DEV)
    dtx_d = None if dtx is None else dtx.to(DEV)
    dirs, pts, view, txn = _nan(R, 3), _nan(B, R * S, 3), _nan(B, R * S, 3), _nan(B, R * S, 3)
    dtxn = _nan(B, R * S, 3) if with_dtx else None
    _lib.call("avr_sample_rays_dev", ctypes.byref(p), B, u_d.data_ptr(), 0, ro_d.data_ptr(), tx_d.data_ptr(),
              _lib._ptr(dtx_d), dirs.data_ptr(), pts.data_ptr(), view.data_ptr(), txn.data_ptr(), _lib._ptr(dtxn),
              _st())
    torch.cuda.synchronize()
    got = dict(pts=pts, view=view, tx=txn, dir_tx=dtxn, dirs=dirs)
    got = {k: None if v is None else v.cpu().numpy() for k, v in got.items()}
    _check_against_references(case, with_dtx, got)
    fb = _sample(case, with_dtx, "host")
    equal = {k: bool(np.array_equal(got[k], fb[k])) for k in got if got[k] is not None}
    _report("wide fused vs fallback", "bit-equal", equal)
    # the route sample() takes for a HIP-tensor jitter is this entry point
    via = _sample(case, with_dtx, "dev")
    for k in got:
        if got[k] is not None:
            _same(via[k], got[k], f"wide sample(u on device) {k}")


@pytest.mark.parametrize("case,shard", ssc.SHARD_RUNS, ids=ssc.run_id)
def test_ray_range_shards_are_slices_of_the_full_outputs(case, shard):
    """ray_range = (r0, r1): dirs is rows [r0:r1] and pts / view / tx the
    [:, r0*S : r1*S] slices of the full-sphere outputs, bit for bit."""
    r0, r1 = shard
    S = case.S
    with_dtx = case.dir_tx[0]
    for route in (("host", "staged") if case.fused else ("host",)):
        full = _sample(case, with_dtx, route)
        part = _sample(case, with_dtx, route, shard)
        _same(part["dirs"], full["dirs"][r0:r1], f"{route} dirs")
        for k in NET:
            if full[k] is None:
                assert part[k] is None
                continue
            assert part[k].shape == (case.B, (r1 - r0) * S, 3)
            _same(part[k], full[k][:, r0 * S:r1 * S], f"{route} {k}")
        _check_against_references(case, with_dtx, part, shard)


@pytest.mark.parametrize("n_azi,n_ele", [(5, 3), (300, 1), (1, 1)])
@pytest.mark.parametrize("random_azi", [True, False])
def test_public_ray_directions(n_azi, n_ele, random_azi):
    """renderer.ray_directions against the oracle under the same seed; it
    consumes the CPU generator exactly as the oracle does."""
    seed = 5
    ref, _, ref_next = ssc.seeded_sphere_directions(n_azi, n_ele, seed, jitter=random_azi)
    torch.manual_seed(seed)
    with _nan_empty():
        dirs, a, b = ray_directions(n_azi, n_ele, random_azi, device=DEV)
    nxt = torch.rand(1)
    assert a is None and b is None
    got = dirs.cpu().numpy()
    assert got.shape == (n_azi * n_ele + 2, 3) and not np.isnan(got).any()
    np.testing.assert_allclose(got, ref.numpy(), rtol=0, atol=ssc.DIRS_ATOL)
    np.testing.assert_array_equal(got[-2:], [[0, 0, 1], [0, 0, -1]])
    assert torch.equal(nxt, ref_next)


def test_refusals_before_any_launch():
    """Argument checks of the fused entry points and of AVRRender.sample."""
    wide, odd = ssc.SAMPLE_BY_NAME["wide"], ssc.SAMPLE_BY_NAME["odd"]

    def call(entry, case, n_rays, r0):
        ro, tx, _ = ssc.poses(case, False)
        ro_d, tx_d = ro.to(DEV), tx.to(DEV)
        u = ssc.jitter(case)
        B, S = case.B, case.S
        p = render_params(case.cfg(), 2, n_rays=n_rays)
        outs = [_nan(n_rays, 3)] + [_nan(B, n_rays * S, 3) for _ in range(3)]
        ptrs = [t.data_ptr() for t in outs]
        try:
            if entry == "avr_sample_rays_staged":
                blk = ssc.staged_block(ro, tx, None, u).to(DEV)
                pose_out = _nan(9 * B)
                outs.append(pose_out)
                _lib.call(entry, ctypes.byref(p), B, blk.data_ptr(), 0, r0, pose_out.data_ptr(), *ptrs, None, _st())
            else:
                u_arg = u.to(DEV) if entry == "avr_sample_rays_dev" else u
                _lib.call(entry, ctypes.byref(p), B, u_arg.data_ptr(), r0, ro_d.data_ptr(), tx_d.data_ptr(), None,
                          *ptrs, None, _st())
        finally:
            torch.cuda.synchronize()
            assert all(bool(torch.isnan(t).all()) for t in outs), "a refused call wrote output"

    with pytest.raises(RuntimeError, match="AVR_MAX_AZI"):
        call("avr_sample_rays", wide, wide.R, 0)
    for entry in ("avr_sample_rays", "avr_sample_rays_dev", "avr_sample_rays_staged"):
        with pytest.raises(RuntimeError, match="ray range outside the sphere"):
            call(entry, odd, 5, odd.R - 4)  # one ray past the south pole
        with pytest.raises(RuntimeError, match="ray range outside the sphere"):
            call(entry, odd, 5, -1)
    ro, tx, _ = ssc.poses(odd, False)
    r = AVRRender(None, **odd.cfg())
    for bad in ((5, 5), (0, odd.R + 1)):
        r.ray_range = bad
        with pytest.raises(ValueError, match="ray_range"):
            r.sample(ro.to(DEV), tx.to(DEV), u_azi=ssc.jitter(odd))
