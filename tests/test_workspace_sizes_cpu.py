"""CPU: the workspace sizes and layouts the library reports are pinned.

Every `*_workspace` entry point and `avr_render_core_layout` is host-only
arithmetic (avr::Arena, csrc/common.h): the Python side allocates exactly what
they return and the launchers carve the same bytes, so a changed number is a
changed contract.  EXPECTED holds the values of the parent build: the library
built at the commit before avr::Arena, which carved every workspace by hand
(`align16` / `al` lambdas).  They were recorded from that library, not derived
from the code under test.

Shapes where a region's own size is no multiple of the alignment, so that a
wrong alignment moves the total (checked on the recorded numbers):
  criterion   align 16: at (1, 130) the frame adjoints Y take B * NY * 4 =
              34220 = 16 * 2138 + 12 bytes, at (3, 161) 125892 = 16 * 7868 + 4
  hash grid   align 256: the tables of P and of P + 1 ints cannot both be
              multiples of 256 bytes
  core layout align 256: edge_oddT (17 rays x 33 samples) has w and delay of
              2244 B per pose
avr_das_workspace has one fixed shape, and the regions of avr_metrics_workspace
(apart from the criterion workspace it embeds) and of avr_doa_das_workspace are
multiples of 16 bytes for every shape they accept (2 * B * K float2, 2 * B * n
floats with n even; double2 and 2 * ... doubles), so those pin the sizes only.
"""
import ctypes

import numpy as np
import pytest

from avr_amd import _lib
from avr_amd.encoding import level_layout
from avr_amd.workloads import MESHRIR, WORKLOADS

CRITERION = [(1, 130), (3, 161), (4, 801)]
METRICS = [(1, 258), (3, 320), (2, 12288)]
DOA_DAS = [(1, 512, 360), (5, 2048, 1024), (3, 510, 7)]  # 510: F = 256 bins, K = 7 directions
# (n_levels, log2_hashmap_size, base_resolution) of tests/test_gpu_hashgrid.py
HASHGRID = [(20, 18, 16), (8, 14, 16), (20, 16, 16), (20, 20, 16), (2, 21, 256)]
HASHGRID_N = [16384, 20000]
CORE = {
    "c1": (WORKLOADS["c1_meshrir_plumbing"].render, WORKLOADS["c1_meshrir_plumbing"].T),
    "edge_oddT_s4": (dict(MESHRIR, n_azi=5, n_ele=3, n_samples=33), 255),
}
CORE_B = [1, 3]

EXPECTED = {
    'criterion 1 130': 153760,
    'criterion 3 161': 566528,
    'criterion 4 801': 3619248,
    'das': 101184,
    'metrics 1 258': 157904,
    'metrics 3 320': 581936,
    'metrics 2 12288': 14171408,
    'doa_das 1 512 360': 163712,
    'doa_das 5 2048 1024': 6636800,
    'doa_das 3 510 7': 201984,
    'hashgrid 20 18 16 16384': 34729216,
    'hashgrid 20 18 16 20000': 42399232,
    'hashgrid 8 14 16 16384': 13647872,
    'hashgrid 8 14 16 20000': 16660224,
    'hashgrid 20 16 16 16384': 34245376,
    'hashgrid 20 16 16 20000': 41804800,
    'hashgrid 20 20 16 16384': 36557056,
    'hashgrid 20 20 16 20000': 44644864,
    'hashgrid 2 21 256 16384': 3981824,
    'hashgrid 2 21 256 20000': 4865024,
    'core c1 1': [0, 8192, 16384, 276480, 284672, 4, 4],
    'core c1 3': [0, 24576, 49152, 829440, 854016, 4, 4],
    'core edge_oddT_s4 1': [0, 2304, 4608, 71936, 80128, 2, 4],
    'core edge_oddT_s4 3': [0, 6912, 13824, 215808, 240384, 2, 4],
}


def _i64(lib, name, *args):
    out = ctypes.c_int64(-1)
    rc = getattr(lib, name)(*args, ctypes.byref(out))
    assert rc == 0, (name, args, lib.avr_last_error())
    return out.value


def measure(lib):
    """Every pinned number, keyed by entry point and shape."""
    got = {}
    for B, F in CRITERION:
        got[f"criterion {B} {F}"] = _i64(lib, "avr_criterion_workspace", B, F)
    got["das"] = _i64(lib, "avr_das_workspace")
    for B, n in METRICS:
        got[f"metrics {B} {n}"] = _i64(lib, "avr_metrics_workspace", B, n)
    for G, nfft, K in DOA_DAS:
        got[f"doa_das {G} {nfft} {K}"] = _i64(lib, "avr_doa_das_workspace", G, nfft, K)
    for L, log2, base in HASHGRID:
        off = np.ascontiguousarray(level_layout(L, log2, base)[0])
        for N in HASHGRID_N:
            got[f"hashgrid {L} {log2} {base} {N}"] = _i64(lib, "avr_hashgrid_bwd_workspace", N, L, off.ctypes.data)
    for name, (cfg, T) in CORE.items():
        p = _lib.render_params(cfg, T)
        for B in CORE_B:
            off = (ctypes.c_int64 * 5)()
            sp = (ctypes.c_int32 * 2)()
            rc = lib.avr_render_core_layout(ctypes.byref(p), B, _lib.DTYPE_F32, off, sp)
            assert rc == 0, lib.avr_last_error()
            got[f"core {name} {B}"] = list(off) + list(sp)  # w, delay, part, spart, bytes, n_split, k_split
    return got


@pytest.fixture(scope="module")
def got():
    with pytest.MonkeyPatch.context() as mp:  # the layout's split counts read the two tuning knobs
        mp.delenv("AVR_NSPLIT", raising=False)
        mp.delenv("AVR_KSPLIT", raising=False)
        return measure(_lib.load())


def test_every_case_is_pinned(got):
    assert sorted(got) == sorted(EXPECTED)
    assert len(got) == len(CRITERION) + 1 + len(METRICS) + len(DOA_DAS) + len(HASHGRID) * len(HASHGRID_N) \
        + len(CORE) * len(CORE_B)


@pytest.mark.parametrize("key", sorted(EXPECTED))
def test_workspace_size_is_the_recorded_one(got, key):
    assert got[key] == EXPECTED[key]
