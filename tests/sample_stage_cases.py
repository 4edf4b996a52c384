"""Case lists and references for the stage in front of the render core: the
resident tables (`avr_tables`, `avr_ir_twiddle`) and the ways
`AVRRender.sample` turns a pose into network inputs.

Importable without a GPU: numpy / torch-CPU only, no call into the HIP
library.  The references are the oracle's own functions (pinned to the real
reference by tests/golden); the only restatements here are the float64
twiddles and the path-loss formula for tables too short for the reference's
near-field copy.

`tests/test_sample_stages_cpu.py` checks the conditions on the case lists;
`tests/test_gpu_sample_stages.py` runs the kernels against the references.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from unittest import mock

import numpy as np
import torch

from avr_amd.workloads import MESHRIR, RAF, SIMU
from oracle import avr_oracle as orc

THREADS = 256  # threads (= ray-samples) per block of sample_rays_kernel
MAX_AZI = 512  # AVR_MAX_AZI: the last n_azi the fused launch takes
RAGGED = dict(MESHRIR, xyz_min=0, xyz_max=10, far=3, fs=8000)
BLOCKS = {"meshrir": MESHRIR, "raf": RAF, "simu": SIMU, "ragged": RAGGED,
          # int(0.1 / speed * fs) is 1 and 0: the near-field copy is one entry / a no-op
          "lowfs1": dict(MESHRIR, fs=4000), "lowfs0": dict(MESHRIR, fs=3000)}

# tolerances of tests/test_gpu_sample_stages.py, with what each is measured against
PHASE_ATOL = 2.0 ** -23    # same fp32 angle; kernel correctly rounded from double, torch within one spacing
TWIDDLE_ATOL = 2.0 ** -24  # both round one double value once; one spacing for a last-bit libm difference
DIRS_ATOL = 5e-7           # the project's bound on kernel vs torch-CPU trig (test_gpu_render.py)
BELOW_ONE = float(np.nextafter(np.float32(1), np.float32(0)))  # the largest fp32 below 1


# --------------------------------------------------------------------------
# tables
# --------------------------------------------------------------------------
@dataclass(frozen=True)
class TableCase:
    block: str
    S: int
    T: int
    far: float | None = None  # replaces the block's `far` (see TABLE_CASES)

    @property
    def id(self):
        return f"{self.block}-S{self.S}-T{self.T}"

    def cfg(self):
        r = dict(BLOCKS[self.block], n_azi=5, n_ele=3, n_samples=self.S)
        if self.far is not None:
            r["far"] = self.far
        return r

    def oracle_cfg(self):
        return orc.RenderConfig.from_kwargs(**self.cfg())

    @property
    def pl_len(self):
        return int(math.ceil(self.T * 2.5))

    @property
    def near_n(self):
        c = self.cfg()
        return int(0.1 / c["speed"] * c["fs"])

    @property
    def copy_in_range(self):
        """Whether the reference's `table[0:near_n] = table[near_n + 1]` finds its source entry."""
        return self.near_n + 1 < self.pl_len


TABLE_CASES = [
    TableCase("meshrir", 64, 254),
    TableCase("meshrir", 256, 1022),
    TableCase("meshrir", 33, 255),  # odd S, odd T
    TableCase("meshrir", 1, 254),   # S = 1: linspace's n == 1 branch
    TableCase("raf", 32, 1600),
    # far = 4 m instead of the block's 6: with S = 2 the last depth is `far`
    # itself and 6 m is 277 samples, past the reference's shift <= 1.5 T guard
    TableCase("raf", 2, 130, far=4.0),
    TableCase("simu", 512, 4094),
    TableCase("simu", 64, 16384),   # the longest T the library accepts
    TableCase("ragged", 40, 250),
    # T = 2, the shortest: 5 path-loss entries, fewer than near_n + 2 = 8, so
    # the reference's near-field copy has no source entry (copy_in_range is
    # False) and `pl` is compared with the formula at k = near_n + 1 for every
    # entry (path_loss_reference).  far keeps the shift within 1.5 T = 3.
    TableCase("meshrir", 3, 2, far=0.04),
    TableCase("lowfs1", 16, 254),   # near_n = 1: one copied entry
    TableCase("lowfs0", 16, 254),   # near_n = 0: the copy is a no-op
]


def path_loss_reference(case: TableCase):
    """The path-loss table [ceil(2.5 T)] fp32: the oracle's, or, where the
    table is too short for the reference's near-field copy, its formula
    `pathloss / (fp32(k / fs * speed) + 1e-3)` with the same torch ops at
    k = near_n + 1 for the entries below near_n and k = i elsewhere (equal to
    the oracle's table wherever that exists; test_sample_stages_cpu)."""
    c = case.oracle_cfg()
    if case.copy_in_range:
        return orc.path_loss_table(c, case.T)
    return path_loss_formula(case)


def path_loss_formula(case: TableCase):
    c = case.oracle_cfg()
    i = torch.arange(0, case.T * 2.5)
    k = torch.where(i < case.near_n, torch.full_like(i, case.near_n + 1), i)
    return c.pathloss / (k / c.fs * c.speed + 1e-3)


def table_references(case: TableCase):
    """dict of the oracle's d_vals, frac, shift (int32), pl and phase [S, F, 2] as numpy."""
    c = case.oracle_cfg()
    d = orc.depth_samples(c)
    frac, shift = orc.receiver_delay(c, d)
    phase = torch.view_as_real(orc.phase_rotation(frac, case.T))
    assert phase.dtype == torch.float32
    return dict(d_vals=d.numpy(), frac=frac.numpy(), shift=shift.numpy().astype(np.int32),
                pl=path_loss_reference(case).numpy(), phase=phase.numpy())


def twiddle_reference(n: int, sign: float):
    """[n, 2] fp32: (cos, sign * sin)(2 pi k / n) in float64, rounded once.
    sign = -1 is avr_tables' forward-DFT twiddle, +1 avr_ir_twiddle's."""
    a = 2 * np.pi * np.arange(n, dtype=np.float64) / n
    return np.stack([np.cos(a), sign * np.sin(a)], -1).astype(np.float32)


# --------------------------------------------------------------------------
# sampling
# --------------------------------------------------------------------------
@dataclass(frozen=True)
class SampleCase:
    name: str
    block: str
    n_azi: int
    n_ele: int
    S: int
    B: int
    dir_tx: tuple  # the values of with_dir_tx the case runs with
    shards: tuple = ()
    seed: int = 0
    # names of the properties below that must hold (test_sample_stages_cpu)
    edges: tuple = field(default=(), compare=False)

    @property
    def id(self):
        return self.name

    @property
    def R(self):
        return self.n_azi * self.n_ele + 2

    @property
    def n(self):
        """ray-samples (threads) of a full-sphere launch"""
        return self.B * self.R * self.S

    @property
    def n_blocks(self):
        return -(-self.n // THREADS)

    @property
    def fused(self):
        return self.n_azi <= MAX_AZI

    def cfg(self):
        return dict(BLOCKS[self.block], n_azi=self.n_azi, n_ele=self.n_ele, n_samples=self.S)

    def oracle_cfg(self):
        return orc.RenderConfig.from_kwargs(**self.cfg())

    # ---- the edges of the 256-thread block logic, from B, R, S and 256
    def _block_spans(self):
        """(first, last) flattened (listener, ray) index of every block."""
        for i0 in range(0, self.n, THREADS):
            yield i0 // self.S, (min(self.n, i0 + THREADS) - 1) // self.S

    @property
    def ragged_last_block(self):
        return self.n % THREADS != 0

    @property
    def listeners_per_block(self):
        return max(b1 // self.R - b0 // self.R + 1 for b0, b1 in self._block_spans())

    @property
    def rays_per_block(self):
        return max(b1 - b0 + 1 for b0, b1 in self._block_spans())

    @property
    def pose_copy_rounds(self):
        """rounds of the staged route's 256-thread pose_out copy loop"""
        return -(-3 * self.B // THREADS)

    @property
    def ray_straddles_blocks(self):
        """some ray's samples lie in two blocks"""
        return any((i0 % self.S) != 0 for i0 in range(THREADS, self.n, THREADS))

    @property
    def listener_straddles_blocks(self):
        return any((i0 % (self.R * self.S)) != 0 for i0 in range(THREADS, self.n, THREADS))

    @property
    def one_ray_per_block(self):
        return self.S == THREADS and self.rays_per_block == 1

    @property
    def ray_spans_two_blocks(self):
        return self.S > THREADS

    @property
    def many_listeners_per_block(self):
        return self.R * self.S < THREADS and self.listeners_per_block > 2

    @property
    def multi_round_pose_copy(self):
        return self.pose_copy_rounds > 1

    @property
    def multi_block(self):
        return self.n_blocks > 1

    @property
    def last_fused_n_azi(self):
        return self.n_azi == MAX_AZI

    @property
    def fallback(self):
        return self.n_azi == MAX_AZI + 1

    @property
    def offset_cube(self):
        c = self.cfg()
        return c["xyz_min"] != -c["xyz_max"]

    @property
    def shard_crosses_into_poles(self):
        """a shard with r_begin > 0 holds grid rays and a pole"""
        grid = self.R - 2
        return any(0 < r0 < grid < r1 for r0, r1 in self.shards)

    @property
    def shard_of_poles_only(self):
        return any(r0 >= self.R - 2 for r0, _ in self.shards)


SAMPLE_CASES = [
    # 86 listeners per block; pose_out copy loop runs more than one round
    # (600 > 256); ragged last block
    SampleCase("one", "meshrir", 1, 1, 1, 200, (True,),
               edges=("many_listeners_per_block", "multi_round_pose_copy", "ragged_last_block", "multi_block")),
    # rays and listeners straddle blocks; n = 1683
    SampleCase("odd", "meshrir", 5, 3, 33, 3, (False,), shards=((0, 6), (6, 16), (15, 17), (16, 17)),
               edges=("ray_straddles_blocks", "listener_straddles_blocks", "ragged_last_block",
                      "shard_crosses_into_poles", "shard_of_poles_only")),
    # exactly one ray per block
    SampleCase("row", "meshrir", 5, 1, 256, 2, (False,), edges=("one_ray_per_block", "multi_block")),
    # a ray spans two blocks
    SampleCase("long", "meshrir", 3, 1, 300, 2, (True,), edges=("ray_spans_two_blocks", "ray_straddles_blocks")),
    # the ragged block's cube 0..10: lo != -hi
    SampleCase("ragcube", "ragged", 3, 1, 40, 3, (False,), edges=("offset_cube", "ragged_last_block")),
    # cube +-12
    SampleCase("raf", "raf", 6, 4, 32, 4, (True,), edges=("multi_block", "listener_straddles_blocks")),
    # the last n_azi the fused launch takes
    SampleCase("max", "meshrir", 512, 1, 2, 2, (False,), edges=("last_fused_n_azi", "multi_block")),
    # the three-launch fallback
    SampleCase("wide", "meshrir", 513, 1, 2, 2, (False, True), shards=((0, 200), (200, 515)),
               edges=("fallback", "shard_crosses_into_poles")),
]
SAMPLE_BY_NAME = {c.name: c for c in SAMPLE_CASES}
SAMPLE_RUNS = [(c, d) for c in SAMPLE_CASES for d in c.dir_tx]
SHARD_RUNS = [(c, sh) for c in SAMPLE_CASES for sh in c.shards]


def run_id(v):
    if isinstance(v, (SampleCase, TableCase)):
        return v.id
    if isinstance(v, bool):
        return "dtx" if v else "nodtx"
    if isinstance(v, tuple):
        return "r%d-%d" % v
    return None


def jitter(case: SampleCase):
    """The case's azimuth draw [n_azi] fp32 in [0, 1): seeded; where there is
    room, entry 0 is 0.0 and entry 1 the largest fp32 below 1."""
    g = torch.Generator().manual_seed(1000 + case.seed)
    u = torch.rand(case.n_azi, generator=g)
    if case.n_azi >= 3:
        u[0] = 0.0
        u[1] = BELOW_ONE
    return u


def poses(case: SampleCase, with_dir_tx: bool):
    """(rays_o, position_tx, direction_tx or None), each [B, 3] fp32: seeded
    uniform inside the cube with a 1 m margin (directions: unit vectors)."""
    c = case.cfg()
    rng = np.random.default_rng(2000 + case.seed)
    lo, hi = c["xyz_min"] + 1.0, c["xyz_max"] - 1.0
    ro = torch.from_numpy(rng.uniform(lo, hi, (case.B, 3)).astype(np.float32))
    tx = torch.from_numpy(rng.uniform(lo, hi, (case.B, 3)).astype(np.float32))
    d = rng.standard_normal((case.B, 3))
    d = torch.from_numpy((d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32))
    return ro, tx, (d if with_dir_tx else None)


def sphere_directions_for(n_azi: int, n_ele: int, u_azi, jitter=True):
    """oracle.sphere_directions [R, 3] with its azimuth draw replaced by
    `u_azi` (the elevation draw is multiplied by zero there)."""
    real = torch.rand
    calls = []

    def rand(n):
        calls.append(n)
        return u_azi.clone() if len(calls) == 1 else real(n)

    state = torch.get_rng_state()
    try:
        with mock.patch.object(torch, "rand", rand):
            dirs, u = orc.sphere_directions(n_azi, n_ele, jitter)
    finally:
        torch.set_rng_state(state)
    assert calls == [n_azi, n_ele] and torch.equal(u, u_azi)
    return dirs.float()


def seeded_sphere_directions(n_azi: int, n_ele: int, seed: int, jitter=True):
    """(dirs, u_azi, the next torch.rand(1)) of oracle.sphere_directions under torch.manual_seed(seed)."""
    torch.manual_seed(seed)
    dirs, u = orc.sphere_directions(n_azi, n_ele, jitter)
    return dirs.float(), u, torch.rand(1)


def network_input_reference(case: SampleCase, rays_o, position_tx, direction_tx, dirs, d_vals):
    """oracle.network_inputs on host copies of the kernel's own dirs [R', 3]
    and d_vals [S] -> (pts, view, tx, dir_tx or None) as numpy, each [B, R'*S, 3]."""
    out = orc.network_inputs(case.oracle_cfg(), rays_o, position_tx, dirs, d_vals, direction_tx)
    return tuple(None if t is None else t.contiguous().numpy() for t in out)


# --------------------------------------------------------------------------
# the staged block of a HIP-graph replay with host-side poses (avr_amd.graph)
# --------------------------------------------------------------------------
def staged_block(rays_o, position_tx, direction_tx, u_azi):
    """[rays_o 3B | pos_tx 3B | dir_tx 3B | u_azi n_azi] fp32; the dir_tx
    slots are present (zero) when there is no direction_tx."""
    B = rays_o.size(0)
    blk = torch.zeros(9 * B + u_azi.numel(), dtype=torch.float32)
    blk[:3 * B] = rays_o.reshape(-1)
    blk[3 * B:6 * B] = position_tx.reshape(-1)
    if direction_tx is not None:
        blk[6 * B:9 * B] = direction_tx.reshape(-1)
    blk[9 * B:] = u_azi
    return blk


def unstage_block(blk, B, has_dir_tx):
    """Inverse of staged_block -> (rays_o, position_tx, direction_tx or None, u_azi)."""
    ro, tx, dtx = (blk[k * 3 * B:(k + 1) * 3 * B].view(B, 3) for k in range(3))
    return ro, tx, (dtx if has_dir_tx else None), blk[9 * B:]
