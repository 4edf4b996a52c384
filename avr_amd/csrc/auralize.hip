// Auralization: the reference's DoA evaluation chain in front of its
// estimators (whitenoise_bandpass_doa.py:93-117) on the GPU.
//
//   avr_conv_source   y[s,c,:] = np.convolve(x[s], h[c], "full"), all channels
//                     against a shared source as one GEMM with a Toeplitz
//                     operand on the exact-fp32 MFMA
//   avr_sosfiltfilt   scipy.signal.sosfiltfilt(sos, y, axis=-1), fp64,
//                     one thread per row
//
// and, beyond the reference, a source or listener that moves:
//
//   avr_conv_trajectory  the same GEMM per path point, each source sample
//                     played through the IR in force when it is emitted,
//                     crossfaded linearly between points
//
// DESIGN.md §18, §22.
#include "common.h"

namespace avr {
namespace {

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef float floatx4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------- source convolution
// Y[c, n] = sum_k H[c, k] * x[n - k] on the exact-fp32 MFMA: an fp32 FMA
// chain in ascending k, so a row depends only on its own h and x.
// R = 32: v_mfma_f32_32x32x2_f32, a workgroup owns 32 channels x kConvNB
// outputs, each of its 4 waves 4 tiles of 32 outputs.  R = 16 (C <= 16, one
// 8-microphone group): v_mfma_f32_16x16x4_f32, 16 channels, 8 tiles of 16
// outputs per wave, half the issued work.  Either way a wave's independent
// accumulators reach the MFMA issue rate from one wave per SIMD and an A
// fragment serves all its tiles.
// A = h tile, staged k-major ([k][R + 1]: the lanes of a row read
// consecutive words, the transposing writes spread over the banks).
// B is never materialised: lane l needs B[k = l / R][j = l % R] =
// x[base + j - k], one ds_read_b32 at consecutive addresses from a window
// of x in LDS (zeros outside [0, L)).
constexpr int kConvThreads = 256;
constexpr int kConvKc = 64;               // taps per LDS stage
constexpr int kConvGroups = kConvKc / 4;  // groups of 4 taps (8 MFMAs) per stage
constexpr int kConvWave = 128;            // outputs per wave
constexpr int kConvNB = 4 * kConvWave;    // outputs per workgroup (512)
constexpr int kConvWin = kConvNB + kConvKc - 1;
constexpr int kConvXLoads = (kConvWin + kConvThreads - 1) / kConvThreads;
constexpr int kConvFrag = 8;              // B fragments (= MFMAs) per group

template <int R>
__device__ __forceinline__ auto conv_mfma(float a, float b,
                                          std::conditional_t<R == 32, floatx16, floatx4> c) {
    if constexpr (R == 32)
        return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

template <int R>
__global__ __launch_bounds__(kConvThreads) void conv_source_kernel(
    int C, int Nh, int64_t L, int64_t N, const float* __restrict__ h, const float* __restrict__ x,
    float* __restrict__ y) {
    using Acc = std::conditional_t<R == 32, floatx16, floatx4>;
    constexpr int kRegs = R == 32 ? 16 : 4;     // accumulator registers per tile
    constexpr int kTiles = kConvWave / R;       // R-output tiles per wave (4 or 8)
    constexpr int kSteps = kConvFrag / kTiles;  // MFMA k-steps per group (2 or 1)
    constexpr int kPer = 4 / kSteps;            // taps per MFMA (2 or 4)
    __shared__ float As[kConvKc][R + 1];
    __shared__ float xs[kConvWin];
    const int64_t nb = (int64_t)blockIdx.x * kConvNB;
    const int c0 = blockIdx.y * R;
    const int s = blockIdx.z;
    const float* xrow = x + (int64_t)s * L;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int kq = lane / R, j = lane % R;  // this lane's tap within an MFMA, its row / column

    // taps that meet a sample of x for some output of this block:
    // n - k in [0, L)  =>  k in [nb - (L-1), nb + NB - 1]; whole stages, in
    // ascending order (a skipped stage would only have added +0 products)
    const int64_t klo = nb - (L - 1);
    const int k_begin = klo > 0 ? (int)(klo / kConvKc) * kConvKc : 0;
    const int k_end = (int)(nb + kConvNB < (int64_t)Nh ? nb + kConvNB : (int64_t)Nh);

    // A staging: thread owns tap k0 + (tid & 63) of rows (tid >> 6) + 4i
    constexpr int kARows = R / 4;
    const int col = threadIdx.x & 63, row0 = threadIdx.x >> 6;
    float araw[kARows], xraw[kConvXLoads];
    auto issue = [&](int k0) {
        const int k = k0 + col;
        const int kc = k < Nh ? k : Nh - 1;
#pragma unroll
        for (int i = 0; i < kARows; ++i) {
            const int c = c0 + row0 + 4 * i;
            const int cc = c < C ? c : C - 1;
            araw[i] = h[(int64_t)cc * Nh + kc];
        }
        // xs[i] = x[nb - k0 - (Kc-1) + i]
        const int64_t xbase = nb - k0 - (kConvKc - 1);
#pragma unroll
        for (int i = 0; i < kConvXLoads; ++i) {
            int64_t g = xbase + i * kConvThreads + (int)threadIdx.x;
            const bool ok = g >= 0 && g < L;
            g = g < 0 ? 0 : (g < L ? g : L - 1);
            const float v = xrow[g];
            xraw[i] = ok ? v : 0.0f;
        }
    };
    auto commit = [&](int k0) {
        const bool kok = k0 + col < Nh;
#pragma unroll
        for (int i = 0; i < kARows; ++i) {
            const bool ok = kok && (c0 + row0 + 4 * i) < C;
            As[col][row0 + 4 * i] = ok ? araw[i] : 0.0f;
        }
#pragma unroll
        for (int i = 0; i < kConvXLoads; ++i) {
            const int w = i * kConvThreads + (int)threadIdx.x;
            if (w < kConvWin) xs[w] = xraw[i];
        }
    };

    Acc acc[kTiles];
#pragma unroll
    for (int t = 0; t < kTiles; ++t)
#pragma unroll
        for (int i = 0; i < kRegs; ++i) acc[t][i] = 0.0f;

    if (k_begin < k_end) issue(k_begin);
    // window index of output (tile t, column j) at tap kk + kq:
    // (wave*128 + t*R + j) - (kk + kq) + (Kc - 1)
    const int bbase = wave * kConvWave + j - kq + (kConvKc - 1);
    float aq[3][kSteps], bq[3][kConvFrag];
    // fragments of group g (taps 4g .. 4g + 3), materialised in registers
    // of their own before any MFMA reads them
    auto fetch = [&](int g, float* af, float* bf) {
#pragma unroll
        for (int p = 0; p < kSteps; ++p) {
            const int kk = 4 * g + kPer * p;
            af[p] = As[kk + kq][j];
#pragma unroll
            for (int t = 0; t < kTiles; ++t) bf[p * kTiles + t] = xs[bbase + t * R - kk];
        }
#pragma unroll
        for (int i = 0; i < kConvFrag; ++i) asm volatile("" : "+v"(bf[i]));
#pragma unroll
        for (int p = 0; p < kSteps; ++p) asm volatile("" : "+v"(af[p]));
    };
    auto hold = [&](const float* af, const float* bf) {
#pragma unroll
        for (int i = 0; i < kConvFrag; ++i) keep_live(bf[i]);
#pragma unroll
        for (int p = 0; p < kSteps; ++p) keep_live(af[p]);
    };
    for (int k0 = k_begin; k0 < k_end; k0 += kConvKc) {
        __syncthreads();
        commit(k0);
        __syncthreads();
        if (k0 + kConvKc < k_end) issue(k0 + kConvKc);  // next stage's loads fly under the MFMAs
        // Fragments live in a ring of 3 slots, one slot per group of 4 taps
        // (8 MFMAs).  Group g + 1's reads are issued before group g's MFMAs
        // (their latency hides under them) and go into the slot of group
        // g - 2: the slot of group g - 1 is held until group g's MFMAs have
        // issued, so no operand register is refilled within a whole group of
        // MFMAs behind the one that read it.
        fetch(0, aq[0], bq[0]);
#pragma unroll
        for (int g = 0; g < kConvGroups; ++g) {
            if (g + 1 < kConvGroups) fetch(g + 1, aq[(g + 1) % 3], bq[(g + 1) % 3]);
#pragma unroll
            for (int p = 0; p < kSteps; ++p)
#pragma unroll
                for (int t = 0; t < kTiles; ++t)
                    acc[t] = conv_mfma<R>(aq[g % 3][p], bq[g % 3][p * kTiles + t], acc[t]);
            __builtin_amdgcn_sched_barrier(0);
            if (g >= 1) hold(aq[(g - 1) % 3], bq[(g - 1) % 3]);
        }
        mfma_queue_wait();
        hold(aq[(kConvGroups - 1) % 3], bq[(kConvGroups - 1) % 3]);
        hold(aq[(kConvGroups - 2) % 3], bq[(kConvGroups - 2) % 3]);
    }
    // accumulator register reg of a lane: column j, row (reg&3) + 8*(reg>>2)
    // + 4*kq (32x32) or 4*kq + reg (16x16); rows beyond C are never stored
#pragma unroll
    for (int t = 0; t < kTiles; ++t) {
        const int64_t n = nb + wave * kConvWave + t * R + j;
        if (n >= N) continue;
#pragma unroll
        for (int reg = 0; reg < kRegs; ++reg) {
            const int c = c0 + (R == 32 ? (reg & 3) + 8 * (reg >> 2) + 4 * kq : 4 * kq + reg);
            if (c < C) y[((int64_t)s * C + c) * N + n] = acc[t][reg];
        }
    }
}

// ------------------------------------------ time-varying source convolution
// Y[c, n] = sum_p sum_k H[p, c, k] * xw[p, n - k], xw[p, m] = w[p, m] x[m]:
// source sample m is played through the IR of the path point in force at
// emission time m, with a linear crossfade over the last `fade` samples of
// each hop.  conv_source_kernel's tiling, stages, fragment
// ring and MFMAs; a stage runs once per path point whose support meets the
// stage's window of x, the later point first: for one output the later point
// holds the smaller taps, so the non-zero products stay in ascending tap
// order, and a product with a zero xw leaves the fp32 FMA chain as it was.
// With one point, or with fade = 0 and equal IRs, the chain is
// conv_source_kernel's.
struct TrajArgs {
    int32_t P, C, Nh;
    int64_t L, N, hop, fade;
};

// point p sounds over source samples [traj_first(p), traj_end(p)); the last
// point holds to the end of x
__device__ __forceinline__ int64_t traj_first(const TrajArgs& a, int p) {
    return p > 0 ? (int64_t)p * a.hop - a.fade : 0;
}
__device__ __forceinline__ int64_t traj_end(const TrajArgs& a, int p) {
    return p + 1 < a.P ? ((int64_t)p + 1) * a.hop : a.L;
}
// w[p, m] for m in [0, L): u = fp32(2j + 1) / fp32(2 fade), one correctly
// rounded division (2j + 1 < 2^24 is exact), fading in over the `fade`
// samples before p's interval and out as 1 - u over the last `fade` of it
__device__ __forceinline__ float traj_weight(const TrajArgs& a, int p, int64_t m) {
    const int64_t lo = (int64_t)p * a.hop;
    const float den = (float)(2 * a.fade);
    if (p > 0 && m < lo) {
        const int64_t j = m - (lo - a.fade);
        return j >= 0 ? __fdiv_rn((float)(2 * j + 1), den) : 0.0f;
    }
    if (p + 1 < a.P) {
        const int64_t j = m - (lo + a.hop - a.fade);
        if (m >= lo + a.hop) return 0.0f;
        if (j >= 0) return 1.0f - __fdiv_rn((float)(2 * j + 1), den);
    }
    return 1.0f;
}

template <int R>
__global__ __launch_bounds__(kConvThreads) void conv_trajectory_kernel(
    TrajArgs a, const float* __restrict__ h, const float* __restrict__ x, float* __restrict__ y) {
    using Acc = std::conditional_t<R == 32, floatx16, floatx4>;
    constexpr int kRegs = R == 32 ? 16 : 4;
    constexpr int kTiles = kConvWave / R;
    constexpr int kSteps = kConvFrag / kTiles;
    constexpr int kPer = 4 / kSteps;
    __shared__ float As[kConvKc][R + 1];
    __shared__ float xs[kConvWin];
    const int C = a.C, Nh = a.Nh;
    const int64_t L = a.L, N = a.N;
    const int64_t nb = (int64_t)blockIdx.x * kConvNB;
    const int c0 = blockIdx.y * R;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int kq = lane / R, j = lane % R;

    // the stages of conv_source_kernel
    const int64_t klo = nb - (L - 1);
    const int k_begin = klo > 0 ? (int)(klo / kConvKc) * kConvKc : 0;
    const int k_end = (int)(nb + kConvNB < (int64_t)Nh ? nb + kConvNB : (int64_t)Nh);

    // A stage's window of x is [nb - k0 - (Kc-1), nb - k0 + NB - 1] cut to
    // [0, L); the points that sound in it are p_lo .. p_hi.  The window moves
    // down by Kc per stage, so both only ever step down: no division per stage.
    auto win_lo = [&](int k0) {
        const int64_t g = nb - k0 - (kConvKc - 1);
        return g > 0 ? g : (int64_t)0;
    };
    auto win_hi = [&](int k0) {
        const int64_t g = nb - k0 + (kConvNB - 1);
        return g < L ? g : L - 1;
    };
    int p_lo = 0, p_hi = 0;
    if (k_begin < k_end) {
        const int64_t last = a.P - 1;
        const int64_t ql = win_lo(k_begin) / a.hop, qh = (win_hi(k_begin) + a.fade) / a.hop;
        p_lo = (int)(ql < last ? ql : last);
        p_hi = (int)(qh < last ? qh : last);
    }
    auto settle = [&](int k0) {
        const int64_t lo = win_lo(k0), hi = win_hi(k0);
        while (p_hi > 0 && traj_first(a, p_hi) > hi) --p_hi;
        while (p_lo > 0 && traj_end(a, p_lo - 1) > lo) --p_lo;
    };

    constexpr int kARows = R / 4;
    const int col = threadIdx.x & 63, row0 = threadIdx.x >> 6;
    float araw[kARows], xraw[kConvXLoads];
    auto issue = [&](int k0, int p) {
        const int k = k0 + col;
        const int kc = k < Nh ? k : Nh - 1;
#pragma unroll
        for (int i = 0; i < kARows; ++i) {
            const int c = c0 + row0 + 4 * i;
            const int cc = c < C ? c : C - 1;
            araw[i] = h[((int64_t)p * C + cc) * Nh + kc];
        }
        // xs[i] = xw[p, nb - k0 - (Kc-1) + i]: the weight goes on here, once
        const int64_t xbase = nb - k0 - (kConvKc - 1);
#pragma unroll
        for (int i = 0; i < kConvXLoads; ++i) {
            int64_t g = xbase + i * kConvThreads + (int)threadIdx.x;
            const bool ok = g >= 0 && g < L;
            g = g < 0 ? 0 : (g < L ? g : L - 1);
            const float v = traj_weight(a, p, g) * x[g];
            xraw[i] = ok ? v : 0.0f;
        }
    };
    auto commit = [&](int k0) {
        const bool kok = k0 + col < Nh;
#pragma unroll
        for (int i = 0; i < kARows; ++i) {
            const bool ok = kok && (c0 + row0 + 4 * i) < C;
            As[col][row0 + 4 * i] = ok ? araw[i] : 0.0f;
        }
#pragma unroll
        for (int i = 0; i < kConvXLoads; ++i) {
            const int w = i * kConvThreads + (int)threadIdx.x;
            if (w < kConvWin) xs[w] = xraw[i];
        }
    };

    Acc acc[kTiles];
#pragma unroll
    for (int t = 0; t < kTiles; ++t)
#pragma unroll
        for (int i = 0; i < kRegs; ++i) acc[t][i] = 0.0f;

    const int bbase = wave * kConvWave + j - kq + (kConvKc - 1);
    float aq[3][kSteps], bq[3][kConvFrag];
    auto fetch = [&](int g, float* af, float* bf) {
#pragma unroll
        for (int p = 0; p < kSteps; ++p) {
            const int kk = 4 * g + kPer * p;
            af[p] = As[kk + kq][j];
#pragma unroll
            for (int t = 0; t < kTiles; ++t) bf[p * kTiles + t] = xs[bbase + t * R - kk];
        }
#pragma unroll
        for (int i = 0; i < kConvFrag; ++i) asm volatile("" : "+v"(bf[i]));
#pragma unroll
        for (int p = 0; p < kSteps; ++p) asm volatile("" : "+v"(af[p]));
    };
    auto hold = [&](const float* af, const float* bf) {
#pragma unroll
        for (int i = 0; i < kConvFrag; ++i) keep_live(bf[i]);
#pragma unroll
        for (int p = 0; p < kSteps; ++p) keep_live(af[p]);
    };

    // the (stage, point) pairs in order: stages ascending, points descending
    int k0 = k_begin, p = 0;
    bool more = k_begin < k_end;
    if (more) {
        settle(k0);
        p = p_hi;
        issue(k0, p);
    }
    while (more) {
        int k0n = k0, pn = p - 1;
        if (pn < p_lo) {
            k0n = k0 + kConvKc;
            more = k0n < k_end;
            if (more) {
                settle(k0n);
                pn = p_hi;
            }
        }
        __syncthreads();
        commit(k0);
        __syncthreads();
        if (more) issue(k0n, pn);  // the next pair's loads fly under the MFMAs
        // a wave whose own 128 outputs meet none of p's samples in this stage
        // would add +0 products only
        const int64_t wlo = nb + wave * kConvWave - k0 - (kConvKc - 1);
        if (traj_first(a, p) <= wlo + (kConvWave + kConvKc - 2) && traj_end(a, p) > wlo) {
            // the fragment ring of conv_source_kernel
            fetch(0, aq[0], bq[0]);
#pragma unroll
            for (int g = 0; g < kConvGroups; ++g) {
                if (g + 1 < kConvGroups) fetch(g + 1, aq[(g + 1) % 3], bq[(g + 1) % 3]);
#pragma unroll
                for (int s = 0; s < kSteps; ++s)
#pragma unroll
                    for (int t = 0; t < kTiles; ++t)
                        acc[t] = conv_mfma<R>(aq[g % 3][s], bq[g % 3][s * kTiles + t], acc[t]);
                __builtin_amdgcn_sched_barrier(0);
                if (g >= 1) hold(aq[(g - 1) % 3], bq[(g - 1) % 3]);
            }
            mfma_queue_wait();
            hold(aq[(kConvGroups - 1) % 3], bq[(kConvGroups - 1) % 3]);
            hold(aq[(kConvGroups - 2) % 3], bq[(kConvGroups - 2) % 3]);
        }
        k0 = k0n;
        p = pn;
    }
#pragma unroll
    for (int t = 0; t < kTiles; ++t) {
        const int64_t n = nb + wave * kConvWave + t * R + j;
        if (n >= N) continue;
#pragma unroll
        for (int reg = 0; reg < kRegs; ++reg) {
            const int c = c0 + (R == 32 ? (reg & 3) + 8 * (reg >> 2) + 4 * kq : 4 * kq + reg);
            if (c < C) y[((int64_t)c) * N + n] = acc[t][reg];
        }
    }
}

// ------------------------------------------------- zero-phase SOS filter
// scipy.signal.sosfiltfilt with its defaults: odd extension by padlen at
// both ends, a forward pass from zi * ext[0], a pass over the reversed
// result from zi * (its last sample), the extension cut off.  The
// recurrence (direct form II transposed, fp64, scipy's op order) is serial
// in time: one thread per row.  A workgroup is one wave that owns kSosRows
// rows; time is walked in tiles of 64 samples that all 64 lanes move
// between global memory and LDS (coalesced along time), the first kSosRows
// lanes run the recurrence on the tile in LDS.  The next tile's loads are
// issued before the recurrence and land under it.
constexpr int kSosRows = 16;
constexpr int kSosTile = 64;
constexpr int kSosMaxSections = 8;

struct SosArgs {
    int64_t rows, n;
    int32_t padlen, in_f64, out_f64;
    const double* sos;  // [NS][6], a0 == 1
    const double* zi;   // [NS][2]
    const void* y;
    void* out;
    double* ws;  // [rows][n + 2 padlen]
};

// sample i of the odd extension of row r (scipy odd_ext: computed in the
// input's own precision, then widened)
__device__ __forceinline__ double ext_at(const SosArgs& a, int64_t r, int64_t i) {
    const int64_t p = a.padlen, n = a.n;
    int64_t e, m;  // ext = 2*y[e] - y[m] outside, y[m] inside
    bool pad = true;
    if (i < p) {
        e = 0;
        m = p - i;
    } else if (i < p + n) {
        pad = false;
        e = 0;
        m = i - p;
    } else {
        e = n - 1;
        m = n - 2 - (i - p - n);
    }
    if (a.in_f64) {
        const double* y = static_cast<const double*>(a.y) + r * n;
        return pad ? 2.0 * y[e] - y[m] : y[m];
    }
    const float* y = static_cast<const float*>(a.y) + r * n;
    return pad ? (double)(2.0f * y[e] - y[m]) : (double)y[m];
}

template <int NS>
__global__ __launch_bounds__(64) void sosfiltfilt_kernel(SosArgs a) {
    __shared__ double tile[kSosRows][kSosTile + 1];
    const int lane = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * kSosRows;
    const int nrows = (int)(a.rows - r0 < kSosRows ? a.rows - r0 : kSosRows);
    const int64_t M = a.n + 2 * (int64_t)a.padlen;
    const int64_t ntiles = (M + kSosTile - 1) / kSosTile;

    double b0[NS], b1[NS], b2[NS], a1[NS], a2[NS], z0[NS], z1[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) {
        b0[q] = a.sos[q * 6 + 0];
        b1[q] = a.sos[q * 6 + 1];
        b2[q] = a.sos[q * 6 + 2];
        a1[q] = a.sos[q * 6 + 4];
        a2[q] = a.sos[q * 6 + 5];
    }
    auto start = [&](double first) {
#pragma unroll
        for (int q = 0; q < NS; ++q) {
            z0[q] = a.zi[q * 2 + 0] * first;
            z1[q] = a.zi[q * 2 + 1] * first;
        }
    };
    auto step = [&](double u) {
#pragma unroll
        for (int q = 0; q < NS; ++q) {
            const double v = b0[q] * u + z0[q];
            z0[q] = b1[q] * u - a1[q] * v + z1[q];
            z1[q] = b2[q] * u - a2[q] * v;
            u = v;
        }
        return u;
    };
    // this row's cnt samples of the tile, in time order.  (Reading 8 samples
    // ahead of the recurrence measured 4 % faster at 4 sections and spilled
    // at 5 and more: the chain of fp64 operations is the time, not the LDS.)
    auto run_tile = [&](int cnt) {
        for (int q = 0; q < cnt; ++q) tile[lane][q] = step(tile[lane][q]);
    };

    double nxt[kSosRows];
    // ---- forward over the extension: ws[r][i] = filtered ext[i]
    auto load_fwd = [&](int64_t t) {
        const int64_t i = t * kSosTile + lane;
#pragma unroll
        for (int r = 0; r < kSosRows; ++r)
            nxt[r] = (r < nrows && i < M) ? ext_at(a, r0 + r, i) : 0.0;
    };
    load_fwd(0);
    if (lane < nrows) start(ext_at(a, r0 + lane, 0));
    for (int64_t t = 0; t < ntiles; ++t) {
#pragma unroll
        for (int r = 0; r < kSosRows; ++r) tile[r][lane] = nxt[r];
        __syncthreads();
        if (t + 1 < ntiles) load_fwd(t + 1);
        if (lane < nrows) {
            const int cnt = (int)(M - t * kSosTile < kSosTile ? M - t * kSosTile : kSosTile);
            run_tile(cnt);
        }
        __syncthreads();
        const int64_t i = t * kSosTile + lane;
        if (i < M)
            for (int r = 0; r < nrows; ++r) a.ws[(r0 + r) * M + i] = tile[r][lane];
        __syncthreads();
    }
    // the workgroup reads back only what it wrote itself
    __threadfence_block();
    __syncthreads();

    // ---- backward: tile t covers reversed positions, read from ws back to
    // front; position q of the reversed signal is ws[M-1-q].  Outputs
    // ws index i in [padlen, padlen + n) go to out[i - padlen].
    auto load_bwd = [&](int64_t t) {
        const int64_t i = M - 1 - (t * kSosTile + lane);
#pragma unroll
        for (int r = 0; r < kSosRows; ++r) nxt[r] = (r < nrows && i >= 0) ? a.ws[(r0 + r) * M + i] : 0.0;
    };
    load_bwd(0);
    if (lane < nrows) start(a.ws[(r0 + lane) * M + M - 1]);
    for (int64_t t = 0; t < ntiles; ++t) {
#pragma unroll
        for (int r = 0; r < kSosRows; ++r) tile[r][lane] = nxt[r];
        __syncthreads();
        if (t + 1 < ntiles) load_bwd(t + 1);
        if (lane < nrows) {
            const int cnt = (int)(M - t * kSosTile < kSosTile ? M - t * kSosTile : kSosTile);
            run_tile(cnt);
        }
        __syncthreads();
        const int64_t o = M - 1 - (t * kSosTile + lane) - a.padlen;
        if (o >= 0 && o < a.n) {
            if (a.out_f64) {
                double* out = static_cast<double*>(a.out);
                for (int r = 0; r < nrows; ++r) out[(r0 + r) * a.n + o] = tile[r][lane];
            } else {
                float* out = static_cast<float*>(a.out);
                for (int r = 0; r < nrows; ++r) out[(r0 + r) * a.n + o] = (float)tile[r][lane];
            }
        }
        __syncthreads();
    }
}

int sos_shape(int64_t rows, int64_t n, int32_t n_sections, int32_t padlen) {
    AVR_REQUIRE(rows >= 1 && rows <= ((int64_t)1 << 31) - 1, "avr_sosfiltfilt: 1 <= rows < 2^31 required");
    AVR_REQUIRE(n_sections >= 1 && n_sections <= kSosMaxSections,
                "avr_sosfiltfilt: 1 <= n_sections <= 8 required");
    AVR_REQUIRE(padlen >= 0, "avr_sosfiltfilt: padlen must not be negative");
    AVR_REQUIRE(n > padlen && n >= 2, "avr_sosfiltfilt: n must be greater than padlen (and at least 2)");
    AVR_REQUIRE(n <= ((int64_t)1 << 40), "avr_sosfiltfilt: n too large");
    return 0;
}

}  // namespace
}  // namespace avr

using namespace avr;

extern "C" int avr_conv_source(int32_t S, int32_t C, int32_t Nh, int64_t L, const float* h,
                               const float* x, float* y, void* stream) {
    AVR_REQUIRE(S >= 1 && C >= 1 && Nh >= 1 && L >= 1, "avr_conv_source: S, C, Nh and L must be positive");
    AVR_REQUIRE(h && x && y, "avr_conv_source: null pointer");
    AVR_REQUIRE(S <= 65535, "avr_conv_source: at most 65535 sources");
    const int64_t N = L + Nh - 1;
    const int64_t nblk = (N + kConvNB - 1) / kConvNB;
    // one 8-microphone group (C <= 16) takes the 16-row tile: half the issued work
    const int R = C <= 16 ? 16 : 32;
    const int64_t ctiles = ((int64_t)C + R - 1) / R;
    AVR_REQUIRE(nblk <= 0x7fffffffLL, "avr_conv_source: output too long");
    AVR_REQUIRE(ctiles <= 65535, "avr_conv_source: at most 65535 * 32 channels");
    const dim3 grid((unsigned)nblk, (unsigned)ctiles, (unsigned)S);
    return launch("conv_source_kernel", R == 16 ? conv_source_kernel<16> : conv_source_kernel<32>, grid,
                  dim3(kConvThreads), 0, as_stream(stream), C, Nh, L, N, h, x, y);
}

extern "C" int avr_conv_trajectory(int32_t P, int32_t C, int32_t Nh, int64_t L, int64_t hop, int64_t fade,
                                   const float* h, const float* x, float* y, void* stream) {
    AVR_REQUIRE(P >= 1 && C >= 1 && Nh >= 1 && L >= 1 && hop >= 1,
                "avr_conv_trajectory: P, C, Nh, L and hop must be positive");
    AVR_REQUIRE(fade >= 0 && fade <= hop, "avr_conv_trajectory: 0 <= fade <= hop required");
    AVR_REQUIRE(fade < ((int64_t)1 << 23), "avr_conv_trajectory: fade must be below 2^23");
    AVR_REQUIRE(h && x && y, "avr_conv_trajectory: null pointer");
    AVR_REQUIRE(L <= ((int64_t)1 << 40), "avr_conv_trajectory: source too long");
    const int64_t N = L + Nh - 1;
    const int64_t nblk = (N + kConvNB - 1) / kConvNB;
    const int R = C <= 16 ? 16 : 32;
    const int64_t ctiles = ((int64_t)C + R - 1) / R;
    AVR_REQUIRE(nblk <= 0x7fffffffLL, "avr_conv_trajectory: output too long");
    AVR_REQUIRE(ctiles <= 65535, "avr_conv_trajectory: at most 65535 * 32 channels");
    // x ends before point 0 starts to fade: point 0 alone, at weight 1.  Any
    // other hop is below L + 2^23, so the kernel's p * hop stays far inside 64 bits.
    TrajArgs a{hop - fade >= L ? 1 : P, C, Nh, L, N, hop, fade};
    const dim3 grid((unsigned)nblk, (unsigned)ctiles);
    return launch("conv_trajectory_kernel", R == 16 ? conv_trajectory_kernel<16> : conv_trajectory_kernel<32>,
                  grid, dim3(kConvThreads), 0, as_stream(stream), a, h, x, y);
}

extern "C" int avr_sosfiltfilt_workspace(int64_t rows, int64_t n, int32_t n_sections, int32_t padlen,
                                         int64_t* bytes) {
    if (int e = sos_shape(rows, n, n_sections, padlen)) return e;
    AVR_REQUIRE(bytes, "avr_sosfiltfilt_workspace: null bytes");
    *bytes = rows * (n + 2 * (int64_t)padlen) * (int64_t)sizeof(double);
    return 0;
}

extern "C" int avr_sosfiltfilt(int64_t rows, int64_t n, int32_t n_sections, int32_t padlen,
                               const double* sos, const double* zi, const void* y, int32_t in_dtype,
                               void* out, int32_t out_dtype, void* workspace, int64_t workspace_bytes,
                               void* stream) {
    if (int e = sos_shape(rows, n, n_sections, padlen)) return e;
    AVR_REQUIRE(in_dtype == AVR_DTYPE_F32 || in_dtype == AVR_DTYPE_F64,
                "avr_sosfiltfilt: input must be fp32 or fp64");
    AVR_REQUIRE(out_dtype == AVR_DTYPE_F32 || out_dtype == AVR_DTYPE_F64,
                "avr_sosfiltfilt: output must be fp32 or fp64");
    AVR_REQUIRE(sos && zi && y && out && workspace, "avr_sosfiltfilt: null pointer");
    AVR_REQUIRE(workspace_bytes >= rows * (n + 2 * (int64_t)padlen) * (int64_t)sizeof(double),
                "avr_sosfiltfilt: workspace too small");
    AVR_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "avr_sosfiltfilt: workspace must be 8-byte aligned");
    SosArgs a{rows, n, padlen, in_dtype == AVR_DTYPE_F64, out_dtype == AVR_DTYPE_F64, sos, zi, y, out,
              static_cast<double*>(workspace)};
    const dim3 grid((unsigned)((rows + kSosRows - 1) / kSosRows)), block(64);
    hipStream_t st = as_stream(stream);
    switch (n_sections) {
#define AVR_SOS_CASE(NS) \
    case NS: return launch("sosfiltfilt_kernel", sosfiltfilt_kernel<NS>, grid, block, 0, st, a);
        AVR_SOS_CASE(1)
        AVR_SOS_CASE(2)
        AVR_SOS_CASE(3)
        AVR_SOS_CASE(4)
        AVR_SOS_CASE(5)
        AVR_SOS_CASE(6)
        AVR_SOS_CASE(7)
        AVR_SOS_CASE(8)
#undef AVR_SOS_CASE
    }
    return fail(AVR_E_ARG, "avr_sosfiltfilt: n_sections out of range");
}
