"""No GPU: the conditions on tests/sample_stage_cases.py that keep
tests/test_gpu_sample_stages.py from going vacuous."""
import numpy as np
import pytest
import torch

import sample_stage_cases as ssc
from oracle import avr_oracle as orc


# ------------------------------------------------------------------ sampling cases
@pytest.mark.parametrize("case", ssc.SAMPLE_CASES, ids=ssc.run_id)
def test_sampling_case_reaches_its_edges(case):
    assert case.edges
    for e in case.edges:
        assert getattr(case, e) is True, (case.name, e)
    assert case.fused == (case.name != "wide")
    for r0, r1 in case.shards:
        assert 0 <= r0 < r1 <= case.R


def test_sampling_cases_figures():
    """The figures the case list quotes, from B, R, S and 256."""
    by = ssc.SAMPLE_BY_NAME
    one = by["one"]
    assert (one.R, one.n, one.listeners_per_block, one.pose_copy_rounds) == (3, 600, 86, 3)
    assert (by["odd"].R, by["odd"].n) == (17, 1683)
    assert by["row"].n_blocks == by["row"].B * by["row"].R
    assert by["long"].rays_per_block == 2
    assert by["max"].n_azi == ssc.MAX_AZI and by["wide"].n_azi == ssc.MAX_AZI + 1
    assert by["wide"].dir_tx == (False, True)
    # every edge is reached by some case, and the shards cover both fallbacks
    reached = {e for c in ssc.SAMPLE_CASES for e in c.edges}
    assert reached >= {"many_listeners_per_block", "multi_round_pose_copy", "ragged_last_block",
                       "ray_straddles_blocks", "listener_straddles_blocks", "one_ray_per_block",
                       "ray_spans_two_blocks", "offset_cube", "last_fused_n_azi", "fallback",
                       "shard_crosses_into_poles", "shard_of_poles_only"}
    assert any(c.S == 1 for c in ssc.SAMPLE_CASES)
    assert {c.name for c, _ in ssc.SHARD_RUNS} == {"odd", "wide"}
    # the shards of a case tile or overlap the whole sphere
    for c in (by["odd"], by["wide"]):
        assert set().union(*(range(a, b) for a, b in c.shards)) == set(range(c.R))


@pytest.mark.parametrize("case", ssc.SAMPLE_CASES, ids=ssc.run_id)
def test_jitter_and_poses(case):
    u = ssc.jitter(case)
    assert u.dtype == torch.float32 and u.shape == (case.n_azi,)
    assert torch.equal(u, ssc.jitter(case))
    assert (u >= 0).all() and (u < 1).all()
    if case.n_azi >= 3:
        assert u[0] == 0.0 and u[1] == ssc.BELOW_ONE < 1.0
        assert np.float32(ssc.BELOW_ONE) + np.float32(2.0 ** -24) == np.float32(1)
    c = case.cfg()
    for with_dtx in (False, True):
        ro, tx, dtx = ssc.poses(case, with_dtx)
        assert (dtx is not None) == with_dtx
        for t in (ro, tx):
            assert t.shape == (case.B, 3) and t.dtype == torch.float32
            assert t.min() >= c["xyz_min"] + 1 and t.max() <= c["xyz_max"] - 1
    # listeners differ, so a wrong listener index in a block cannot pass
    assert len({tuple(r) for r in ro.tolist()}) == case.B


def test_forced_draw_is_the_oracles_draw():
    """sphere_directions_for(u) is sphere_directions when u is what it would
    draw, consumes nothing from the generator, and responds to u."""
    for n_azi, n_ele in ((5, 3), (1, 1)):
        dirs, u, nxt = ssc.seeded_sphere_directions(n_azi, n_ele, 11)
        torch.manual_seed(4)
        before = torch.get_rng_state()
        forced = ssc.sphere_directions_for(n_azi, n_ele, u)
        assert torch.equal(torch.get_rng_state(), before)
        assert torch.equal(forced, dirs)
        assert not torch.equal(ssc.sphere_directions_for(n_azi, n_ele, torch.zeros(n_azi)), dirs)
        assert torch.equal(ssc.sphere_directions_for(n_azi, n_ele, u, jitter=False),
                           ssc.sphere_directions_for(n_azi, n_ele, torch.zeros(n_azi)))
    assert torch.equal(dirs[-2:], torch.tensor([[0.0, 0, 1], [0, 0, -1]]))


# ------------------------------------------------------------------ staged block
@pytest.mark.parametrize("case,with_dtx", ssc.SAMPLE_RUNS, ids=ssc.run_id)
def test_staged_block_round_trips(case, with_dtx):
    ro, tx, dtx = ssc.poses(case, with_dtx)
    u = ssc.jitter(case)
    blk = ssc.staged_block(ro, tx, dtx, u)
    B = case.B
    assert blk.dtype == torch.float32 and blk.shape == (9 * B + case.n_azi,)
    ro2, tx2, dtx2, u2 = ssc.unstage_block(blk, B, with_dtx)
    assert torch.equal(ro2, ro) and torch.equal(tx2, tx) and torch.equal(u2, u)
    if with_dtx:
        assert torch.equal(dtx2, dtx)
    else:
        assert dtx2 is None and not blk[6 * B:9 * B].any()  # the slots are there either way
    # the layout of avr_amd.graph: element i of listener b's rays_o at 3b + i
    assert blk[3 * (B - 1) + 2] == ro[B - 1, 2] and blk[3 * B] == tx[0, 0] and blk[9 * B] == u[0]


# ------------------------------------------------------------------ table cases
def test_table_case_list():
    ids = [c.id for c in ssc.TABLE_CASES]
    assert len(set(ids)) == len(ids)
    have = {(c.block, c.S, c.T) for c in ssc.TABLE_CASES}
    assert have >= {("meshrir", 64, 254), ("meshrir", 256, 1022), ("meshrir", 33, 255), ("meshrir", 1, 254),
                    ("raf", 32, 1600), ("raf", 2, 130), ("simu", 512, 4094), ("simu", 64, 16384),
                    ("ragged", 40, 250)}
    assert min(c.T for c in ssc.TABLE_CASES) == 2 and max(c.T for c in ssc.TABLE_CASES) == 16384
    assert {0, 1} <= {c.near_n for c in ssc.TABLE_CASES}
    assert [c.id for c in ssc.TABLE_CASES if not c.copy_in_range] == ["meshrir-S3-T2"]


@pytest.mark.parametrize("case", ssc.TABLE_CASES, ids=ssc.run_id)
def test_table_case_within_the_references_guard(case):
    """shift <= 1.5 T: every row table[shift : shift + T] of the reference's
    stack (renderer.py:100) lies inside the ceil(2.5 T) entries."""
    c = case.oracle_cfg()
    _, shift = orc.receiver_delay(c, orc.depth_samples(c))
    assert int(shift.max()) + case.T <= case.pl_len
    if case.copy_in_range:
        orc.path_loss_rows(c, shift, case.T)  # raises like the reference


@pytest.mark.parametrize("case", ssc.TABLE_CASES, ids=ssc.run_id)
def test_path_loss_formula_is_the_oracles_table(case):
    """The formula used where the reference's near-field copy has no source
    entry equals the oracle's table, bit for bit, wherever that exists."""
    f = ssc.path_loss_formula(case)
    assert f.dtype == torch.float32 and f.shape == (case.pl_len,)
    if case.copy_in_range:
        assert torch.equal(f, orc.path_loss_table(case.oracle_cfg(), case.T))
        assert torch.equal(ssc.path_loss_reference(case), f)
    else:
        c = case.oracle_cfg()
        assert case.pl_len <= case.near_n  # every entry is the near-field value
        k = torch.tensor([float(case.near_n + 1)])
        assert torch.equal(f, (c.pathloss / (k / c.fs * c.speed + 1e-3)).expand(case.pl_len))
        with pytest.raises(IndexError):
            orc.path_loss_table(c, case.T)


def test_references_respond_to_what_the_gpu_tests_must_catch():
    """The tolerances separate the errors named in the tests' docstrings
    from a correct table (CPU restatements of those errors)."""
    case = ssc.TABLE_CASES[0]
    ref = ssc.table_references(case)
    S, T = case.S, case.T
    F = T // 2 + 1
    assert ref["phase"].shape == (S, F, 2) and ref["pl"].shape == (case.pl_len,)
    # a float64 angle moves the phase by far more than the bound
    th64 = (-2 * np.pi / T) * np.arange(F)[None, :] * ref["frac"].astype(np.float64)[:, None]
    ph64 = np.stack([np.cos(th64), np.sin(th64)], -1)
    assert np.abs(ph64 - ref["phase"]).max() > 100 * ssc.PHASE_ATOL
    # the near-field entries copied from near_n instead of near_n + 1
    c = case.oracle_cfg()
    wrong = c.pathloss / (np.float32(case.near_n) / np.float32(c.fs) * np.float32(c.speed) + np.float32(1e-3))
    assert case.near_n > 0 and ref["pl"][0] != np.float32(wrong)
    # the two twiddles differ in the sine's sign only
    fwd, inv = ssc.twiddle_reference(T, -1.0), ssc.twiddle_reference(T, 1.0)
    assert fwd.dtype == np.float32 and fwd.shape == (T, 2)
    assert np.array_equal(fwd[:, 0], inv[:, 0]) and np.array_equal(fwd[:, 1], -inv[:, 1])
    assert np.abs(fwd[:, 1] - inv[:, 1]).max() > 1.9
