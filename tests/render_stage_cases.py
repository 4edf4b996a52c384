"""Stage-level float64 references and case lists for the render core.

Importable without a GPU: numpy / torch-CPU float64 only, no call into the
HIP library.  Each reference consumes exactly the operands its kernel
consumes (the fp32 or 16-bit arrays upcast exactly, the device's own tables
copied to the host, integer delays) and evaluates the stage's definition in
float64.  The live window of row (b, r, s) is delay[b,r,s] <= t < T-1-shift[s].

`tests/test_render_stages_cpu.py` composes the references to the oracle and
checks the conditions on the case lists; `tests/test_gpu_render_stages.py`
runs every `avr_*` stage entry point against them.
"""
from __future__ import annotations

import math
import zlib
from dataclasses import dataclass

import numpy as np
import torch

from avr_amd.workloads import MESHRIR, RAF, SIMU
from oracle import avr_oracle as orc

U32 = 2.0 ** -24  # unit roundoff of fp32
BLOCKS = {"meshrir": MESHRIR, "raf": RAF, "simu": SIMU}


# --------------------------------------------------------------------------
# configs
# --------------------------------------------------------------------------
def render_cfg(block: str, S: int, T: int, n_azi: int = 5, n_ele: int = 1, shift_frac: float = 0.5):
    """A `render:` block of workloads.py with `far` chosen so the largest
    receiver shift is about shift_frac*T (check_config needs <= 1.5 T)."""
    r = dict(BLOCKS[block])
    r.update(n_azi=n_azi, n_ele=n_ele, n_samples=S)
    r["far"] = float(np.float32(shift_frac * T * r["speed"] / r["fs"]))
    return r


def host_shift(cfg: dict, T: int) -> np.ndarray:
    """shift[S] as the reference computes it (oracle.receiver_delay)."""
    c = orc.RenderConfig.from_kwargs(**cfg)
    _, sh = orc.receiver_delay(c, orc.depth_samples(c))
    return sh.numpy().astype(np.int64)


@dataclass(frozen=True)
class ReduceCase:
    S: int
    T: int
    dtype: str  # float32 | float16 | bfloat16
    R: int = 7
    n_splits: tuple = (1, 2, 4)
    vector: bool = True
    offset: int = 0  # elements the signal tensor is shifted off 16-byte alignment
    block: str = "meshrir"
    B: int = 2

    @property
    def id(self):
        return f"{self.S}x{self.T}-{self.dtype}-R{self.R}" + (f"-off{self.offset}" if self.offset else "")

    @property
    def vec(self):
        return 4 if self.dtype == "float32" else 8

    def cfg(self):
        return render_cfg(self.block, self.S, self.T, n_azi=self.R - 2, n_ele=1)


_F32_VEC = [(2, 2046), (2, 2050), (2, 4098), (2, 8194), (2, 12290), (2, 16384)]
_H_VEC = [(4, 8190), (4, 8194), (4, 16382)]
# both sides of every chunks-per-lane boundary of the vector path (1024 lanes
# of 4 or 8 elements): the launchers instantiate only the (chunks per lane,
# launch bound) pairs a shape can reach, and these shapes reach each of them
CPT_EDGES = (
    [ReduceCase(2, T, "float32", n_splits=(1, 4)) for T in (4096, 4100, 8192, 8196, 12288, 12292)]
    + [ReduceCase(4, T, d, n_splits=(1, 4)) for d in ("float16", "bfloat16") for T in (8192, 8200)]
)

# (a) forward, vector path: 512 / 1024 threads, 1-4 chunks per lane, column
# phases 0/2 (fp32) and 0/6/4/2 (16-bit); R = 7 with 1, 2, 4 splits (4-ray
# unrolled loop + remainder, a 1-ray split), R = 5 with 4 splits (empty last)
REDUCE_FWD_VECTOR = (
    [ReduceCase(S, T, "float32") for S, T in _F32_VEC]
    + [ReduceCase(S, T, d) for d in ("float16", "bfloat16") for S, T in _H_VEC]
    + [ReduceCase(2, 2050, "float32", R=5, n_splits=(4,)), ReduceCase(4, 8194, "float16", R=5, n_splits=(4,))]
    + CPT_EDGES
)
# (b) scalar path: S*T not a multiple of the vector width (1-4 chunks per
# lane), and one vector shape with the tensor one element off alignment
_SCALAR_T = (510, 1026, 2050, 3074)
REDUCE_SCALAR = (
    [ReduceCase(3, T, "float32", vector=False, n_splits=(1, 4)) for T in _SCALAR_T]
    + [ReduceCase(3, T, "bfloat16", vector=False, n_splits=(2,)) for T in _SCALAR_T]
    + [ReduceCase(2, 2050, "float32", vector=False, offset=1, n_splits=(2,))]
)
SCALAR_LIMIT = ReduceCase(3, 4098, "float32", vector=False, n_splits=(1,))  # 5 chunks per lane: refused
# (c) backward, vector path: the shapes of (a) plus column groups of 4 and 2
# with a ragged last group
REDUCE_BWD_VECTOR = (
    [ReduceCase(S, T, "float32") for S, T in _F32_VEC]
    + [ReduceCase(S, T, d) for d in ("float16", "bfloat16") for S, T in _H_VEC]
    + [ReduceCase(5, 254, "float32"), ReduceCase(5, 510, "float32"), ReduceCase(3, 1022, "float32")]
    + CPT_EDGES
)
ALL_REDUCE = REDUCE_FWD_VECTOR + REDUCE_SCALAR + REDUCE_BWD_VECTOR + [SCALAR_LIMIT]


@dataclass(frozen=True)
class DftCase:
    S: int
    T: int
    n_splits: tuple = (1,)
    k_splits: tuple = ()  # forced values besides the library's; "max" = ceil(T/64)
    block: str = "raf"
    B: int = 2
    fwd: bool = True  # backward-only cases (tile tails) set this False

    @property
    def id(self):
        return f"{self.S}x{self.T}"

    def cfg(self):
        return render_cfg(self.block, self.S, self.T)

    def forced_k(self):
        nkc = math.ceil(self.T / 64)
        return tuple(nkc if k == "max" else k for k in self.k_splits)


DFT_CASES = [
    DftCase(5, 130, n_splits=(1, 2, 4, 8, 16), k_splits=(1, 2, 3)),  # last slice of k_split 2 holds 2 samples
    DftCase(5, 200, k_splits=(3,)),          # chunk 128: the third slice starts past T (empty, writes zeros)
    DftCase(33, 255, k_splits=(1, "max")),   # odd T, F = 128, one-row second s-tile
    DftCase(33, 256, k_splits=(1, "max")),   # F = 129: one bin in the second 128-bin block
    DftCase(40, 1022, block="meshrir"),      # the ragged golden's S
    DftCase(257, 130, block="simu"),         # 9 s-tiles: XCD-ordered grid with 7 padding groups
    DftCase(33, 8200, k_splits=(1, "max")),  # > 64 KiB LDS launch
    DftCase(33, 16384, k_splits=(1, "max")),
]
DFT_BWD_EXTRA = ([DftCase(S, 130, fwd=False) for S in (15, 16, 17)]        # 16-row tiles
                 + [DftCase(5, T, fwd=False) for T in (63, 64, 65)])      # 64-t tiles
DFT_FWD_CASES = DFT_CASES
DFT_BWD_CASES = DFT_CASES + DFT_BWD_EXTRA

WEIGHT_S = (1, 2, 63, 64, 65, 1024, 1025, 4096, 4097, 8192)
WEIGHT_DTYPES = ("float32", "float16", "bfloat16")
WEIGHT_T, WEIGHT_R, WEIGHT_B = 254, 3, 2


def weights_cfg(S):
    return render_cfg("meshrir", S, WEIGHT_T, n_azi=1, n_ele=1)


TORCH_DTYPE = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}


# --------------------------------------------------------------------------
# synthesized operands
# --------------------------------------------------------------------------
def case_rng(*key):
    """A generator seeded by the case's name (stable across processes)."""
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def synth_delays(case: ReduceCase, shift: np.ndarray) -> np.ndarray:
    """int32 [B,R,S] in [0, T-1] (the reference's clamp).  Every column holds
    0, T-1, lim-1, lim, lim+1 (lim = T-1-shift[s]) and values at 16-byte chunk
    edges +-1 (literal multiples of the vector width, and the edges of the
    column's own alignment phase), so windows open and close on and next to
    chunk edges; rows with delay >= lim are empty."""
    B, R, S, T, vec = case.B, case.R, case.S, case.T, case.vec
    rng = case_rng("delay", case.id)
    slots = B * R
    d = rng.integers(0, T, size=(slots, S))
    early = rng.random((slots, S)) < 0.6  # most windows open in the first quarter
    d = np.where(early, rng.integers(0, max(1, T // 4), size=(slots, S)), d)
    for s in range(S):
        lim = T - 1 - int(shift[s])
        sp = [0, T - 1, lim - 1, lim, lim + 1]
        phase = (s * T) % vec  # element offset of the column's rows from a 16-byte boundary
        m = int(rng.integers(1, max(2, lim // vec)))
        edges = [m * vec - phase, (m // 2 + 1) * vec]  # the column's own chunk edge, a literal multiple
        for e in edges[: max(1, (slots - len(sp)) // 3)]:
            sp += [e - 1, e, e + 1]
        sp = np.clip(np.array(sp[:slots]), 0, T - 1)
        rows = rng.permutation(slots)[: len(sp)]
        d[rows, s] = sp
    return d.reshape(B, R, S).astype(np.int32)


def live_mask(delay, shift, T):
    """bool [B,R,S,T]: delay <= t < T-1-shift[s]."""
    t = np.arange(T)
    lim = (T - 1 - np.asarray(shift, np.int64))[None, None, :, None]
    return (t >= np.asarray(delay, np.int64)[..., None]) & (t < lim)


def synth_reduce_inputs(case: ReduceCase, shift):
    """(x [B,R,S,T] torch in the case's dtype, w [B,R,S] f32, delay int32,
    gz [B,S,T] f32).  Signal entries outside the live window are finite noise
    of magnitude 5 (never NaN: test_nonfinite_semantics pins that contract)."""
    B, R, S, T = case.B, case.R, case.S, case.T
    rng = case_rng("reduce", case.id)
    delay = synth_delays(case, shift)
    live = live_mask(delay, shift, T)
    x = rng.standard_normal((B, R, S, T)).astype(np.float32)
    noise = (5.0 * np.sign(rng.standard_normal((B, R, S, T))) * (0.5 + rng.random((B, R, S, T)))).astype(np.float32)
    x = np.where(live, x, noise)
    w = rng.uniform(-1.0, 1.0, (B, R, S)).astype(np.float32)
    gz = rng.standard_normal((B, S, T)).astype(np.float32)
    xt = torch.from_numpy(x).to(TORCH_DTYPE[case.dtype])
    return xt, w, delay, gz


def live_fraction_reduce(case: ReduceCase) -> float:
    shift = host_shift(case.cfg(), case.T)
    return float(live_mask(synth_delays(case, shift), shift, case.T).mean())


def live_fraction_dft(case: DftCase) -> float:
    shift = host_shift(case.cfg(), case.T)
    return float((np.arange(case.T)[None, :] < (case.T - 1 - shift)[:, None]).mean())


def synth_attn(S: int, dtype: str, far: float) -> torch.Tensor:
    """attn [B,R,S] in the storage dtype, scaled so that each ray's
    transmittance at the last sample, prod_{k<S-1} (exp(-attn_k gap_k) + 1e-6),
    lies in [0.05, 0.5] (S >= 2; a single sample has no factor)."""
    rng = case_rng("attn", S, dtype)
    u = rng.uniform(0.5, 1.5, (WEIGHT_B, WEIGHT_R, S))
    a = u * (1.6 / max(far, 1e-9))
    return torch.from_numpy(a.astype(np.float32)).to(TORCH_DTYPE[dtype])


def final_transmittance(attn: torch.Tensor, d_vals) -> np.ndarray:
    """[B,R]: the exclusive transmittance product at the last sample, float64."""
    a = attn.double().numpy()
    d = np.asarray(d_vals, np.float64)
    gaps = d[1:] - d[:-1]
    f = np.exp(-a[..., :-1] * gaps) + 1e-6
    return f.prod(-1)


# --------------------------------------------------------------------------
# references (float64)
# --------------------------------------------------------------------------
def ref_reduce_fwd(x, w, delay, shift, n_split, with_bound=False):
    """part[k,b,s,t] = sum over the rays of split k of w*x inside the live
    window; rps = ceil(R / n_split).  with_bound: also (sum |w*x| [live], rays
    of the split) for the fma-chain error bound."""
    x = np.asarray(x, np.float64)
    w = np.asarray(w, np.float64)
    B, R, S, T = x.shape
    live = live_mask(delay, shift, T)
    prod = np.where(live, w[..., None] * x, 0.0)
    rps = -(-R // n_split)
    part = np.zeros((n_split, B, S, T))
    mag = np.zeros((n_split, B, S, T))
    n_r = np.zeros(n_split, np.int64)
    for k in range(n_split):
        sl = slice(k * rps, min(R, (k + 1) * rps))
        part[k] = prod[:, sl].sum(1)
        mag[k] = np.abs(prod[:, sl]).sum(1)
        n_r[k] = max(0, sl.stop - sl.start)
    return (part, mag, n_r) if with_bound else part


def ref_reduce_bwd(x, gz, w, delay, shift, with_bound=False):
    """grad_x = w*[live]*gz, grad_w = sum_t [live]*gz*x."""
    x = np.asarray(x, np.float64)
    w = np.asarray(w, np.float64)
    gz = np.asarray(gz, np.float64)
    T = x.shape[-1]
    live = live_mask(delay, shift, T)
    g = np.where(live, gz[:, None], 0.0)
    grad_x = w[..., None] * g
    grad_w = (g * x).sum(-1)
    if with_bound:
        return grad_x, grad_w, np.abs(g * x).sum(-1), live.sum(-1)
    return grad_x, grad_w


def _pl_rows(pl, shift, T):
    t = np.arange(T)
    shift = np.asarray(shift, np.int64)
    rows = np.asarray(pl, np.float64)[shift[:, None] + t[None, :]]
    mask = t[None, :] < (T - 1 - shift)[:, None]
    return rows, mask


def ref_dft_fwd(part, pl, shift, phase):
    """out[b,f] (complex128) = sum_s phase[s,f] * rfft_t(z*pl[shift_s+t]*[t<T-1-shift_s]),
    z = sum_k part[k]."""
    z = np.asarray(part, np.float64).sum(0)
    T = z.shape[-1]
    rows, mask = _pl_rows(pl, shift, T)
    a = np.where(mask, z * rows, 0.0)
    return (np.fft.rfft(a, axis=-1) * np.asarray(phase, np.complex128)[None]).sum(1)


def ref_dft_bwd(g, pl, shift, phase, T):
    """gz[b,s,t]: the exact adjoint of ref_dft_fwd with respect to z for the
    real pairing <out, g> = sum Re(out)*Re(g) + Im(out)*Im(g)."""
    g = np.asarray(g, np.complex128)
    phase = np.asarray(phase, np.complex128)
    F = phase.shape[-1]
    H = g[:, None, :] * np.conj(phase)[None]  # [B,S,F]
    Hp = np.zeros(H.shape[:-1] + (T,), np.complex128)
    Hp[..., :F] = H
    da = np.fft.ifft(Hp, axis=-1).real * T  # sum_f Re(H e^{+2 pi i t f / T})
    rows, mask = _pl_rows(pl, shift, T)
    return np.where(mask, da * rows, 0.0)


def ref_irfft(spec):
    """torch c2r semantics: imaginary parts of DC and Nyquist ignored."""
    s = np.array(spec, np.complex128)
    n = 2 * (s.shape[-1] - 1)
    s[..., 0] = s[..., 0].real
    s[..., -1] = s[..., -1].real
    return np.fft.irfft(s, n=n, axis=-1)


def ref_irfft_bwd(g):
    """Adjoint of ref_irfft: interior bins doubled, zero imaginary gradient at
    DC and Nyquist, 1/n."""
    g = np.asarray(g, np.float64)
    n = g.shape[-1]
    r = np.fft.rfft(g, axis=-1)
    c = np.full(r.shape[-1], 2.0)
    c[0] = c[-1] = 1.0
    r = r * c / n
    r[..., 0] = r[..., 0].real
    r[..., -1] = r[..., -1].real
    return r


def ref_weights(attn, d_vals, grad_w=None, dtype=np.float64):
    """oracle.composite_weights restated in float64; with grad_w also the
    float64-autograd gradient for attn."""
    a = torch.as_tensor(np.asarray(attn, dtype)).clone().requires_grad_(grad_w is not None)
    d = torch.as_tensor(np.asarray(d_vals, dtype))
    gaps = torch.cat([d[1:] - d[:-1], torch.tensor([1e10], dtype=d.dtype)])
    alpha = 1.0 - torch.exp(-a * gaps)
    factors = torch.cat([torch.ones_like(alpha[..., :1]), 1.0 - alpha + 1e-6], -1)
    w = torch.cumprod(factors, -1)[..., :-1] * alpha
    if grad_w is None:
        return w.numpy()
    (w * torch.as_tensor(np.asarray(grad_w, dtype))).sum().backward()
    return w.detach().numpy(), a.grad.numpy()


def weights_yardstick(attn32, d_vals32, grad_w32):
    """oracle.composite_weights and its autograd in fp32, op for op the
    reference (which needs S >= 2: a single sample takes the same ops here)."""
    if np.shape(attn32)[-1] == 1:
        return ref_weights(attn32, d_vals32, grad_w32, dtype=np.float32)
    a = torch.as_tensor(np.asarray(attn32, np.float32)).clone().requires_grad_(True)
    w = orc.composite_weights(a, torch.as_tensor(np.asarray(d_vals32, np.float32)))
    (w * torch.as_tensor(np.asarray(grad_w32, np.float32))).sum().backward()
    return w.detach().numpy(), a.grad.numpy()


# --------------------------------------------------------------------------
# fp32 yardsticks of the DFT stages (the kernel's summation shape)
# --------------------------------------------------------------------------
def _tw32(T):
    a = 2.0 * np.pi * np.arange(T, dtype=np.float64) / T
    return np.cos(a).astype(np.float32), (-np.sin(a)).astype(np.float32)


def subset(n, count=64, seed=0):
    """All of range(n) when n <= 4096 samples' worth of work allows, else the
    first, the last and count-2 seeded indices (sorted)."""
    if n <= count:
        return np.arange(n)
    rng = np.random.default_rng(seed)
    mid = rng.choice(np.arange(1, n - 1), size=count - 2, replace=False)
    return np.sort(np.concatenate([[0, n - 1], mid]))


def yardstick_dft_fwd(part32, pl32, shift, phase32, k_split, bins):
    """out[b, bins] in float32 with the kernel's summation shape: a sequential
    chain over t within each k-slice, float32 twiddles rounded once from
    float64 cos/sin, slices added next, then a float32 complex multiply by
    phase, then the sum over s.  phase32: [S,F,2] float32."""
    part32 = np.asarray(part32, np.float32)
    K, B, S, T = part32.shape
    z = part32[0].copy()
    for k in range(1, K):
        z = z + part32[k]
    shift = np.asarray(shift, np.int64)
    t = np.arange(T)
    rows = np.asarray(pl32, np.float32)[shift[:, None] + t[None, :]]
    mask = t[None, :] < (T - 1 - shift)[:, None]
    a = np.where(mask, z * rows, np.float32(0)).astype(np.float32)  # [B,S,T]
    c32, s32 = _tw32(T)
    bins = np.asarray(bins, np.int64)
    nkc = -(-T // 64)
    kchunk = -(-nkc // k_split) * 64
    tot_re = np.zeros((B, S, len(bins)), np.float32)
    tot_im = np.zeros_like(tot_re)
    for k0 in range(0, T, kchunk):
        re = np.zeros_like(tot_re)
        im = np.zeros_like(tot_re)
        for tt in range(k0, min(T, k0 + kchunk)):
            idx = (tt * bins) % T
            col = a[:, :, tt, None]
            re += col * c32[idx]
            im += col * s32[idx]
        tot_re += re
        tot_im += im
    pr = np.asarray(phase32, np.float32)[:, bins, 0][None]
    pi = np.asarray(phase32, np.float32)[:, bins, 1][None]
    o_re = (tot_re * pr - tot_im * pi).astype(np.float32)
    o_im = (tot_re * pi + tot_im * pr).astype(np.float32)
    out_re = np.zeros((B, len(bins)), np.float32)
    out_im = np.zeros_like(out_re)
    for s in range(S):
        out_re += o_re[:, s]
        out_im += o_im[:, s]
    return out_re.astype(np.float64) + 1j * out_im.astype(np.float64)


def yardstick_dft_bwd(g32, pl32, shift, phase32, T, samples):
    """gz[b, s, samples] in float32: U, V formed in float32, a sequential chain
    over f with float32 twiddles, then the float32 path-loss product."""
    g32 = np.asarray(g32, np.float32)  # [B,F,2]
    ph = np.asarray(phase32, np.float32)
    S, F = ph.shape[:2]
    gr, gi = g32[:, None, :, 0], g32[:, None, :, 1]
    pc, ps = ph[None, :, :, 0], ph[None, :, :, 1]
    U = (gr * pc + gi * ps).astype(np.float32)  # [B,S,F]
    Vn = (-(gr * ps - gi * pc)).astype(np.float32)
    c32, s32 = _tw32(T)
    samples = np.asarray(samples, np.int64)
    acc = np.zeros((g32.shape[0], S, len(samples)), np.float32)
    for f in range(F):
        idx = (f * samples) % T
        acc += U[:, :, f, None] * c32[idx]
        acc += Vn[:, :, f, None] * s32[idx]
    shift = np.asarray(shift, np.int64)
    rows = np.asarray(pl32, np.float32)[shift[:, None] + samples[None, :]]
    mask = samples[None, :] < (T - 1 - shift)[:, None]
    return np.where(mask, acc * rows, np.float32(0)).astype(np.float64)


def rel_l2(a, b):
    a, b = np.asarray(a), np.asarray(b)
    nb = np.linalg.norm(b)
    d = np.linalg.norm(a - b)
    return float(d / nb) if nb > 0 else float(d)


def rel_max(a, b):
    a, b = np.asarray(a), np.asarray(b)
    mb = np.abs(b).max()
    d = np.abs(a - b).max()
    return float(d / mb) if mb > 0 else float(d)


DFT_FLOOR = 5e-7       # relative L2 floor of the DFT stages' bound
DFT_MARGIN = 4.0       # MFMA adds two products per step; the finalize order differs
DFT_CEILING = 2.5e-5   # the 1e-4 north star divided over the four float stages


def dft_bounds(e32):
    """(relative L2 bound, relative max-norm bound) for a measured e32."""
    l2 = max(DFT_MARGIN * e32, DFT_FLOOR)
    return min(l2, DFT_CEILING), min(4.0 * l2, DFT_CEILING)
