// metrics.hip — the validation metrics of the reference (utils/metric.py:8-136)
// on gfx950, for two batches of impulse responses ori, pred [B][n] fp32.
//
//   Angle     = mean|cos∠O - cos∠P| + mean|sin∠O - sin∠P| over the n-bin FFT  (:37)
//   Amplitude = mean(|a_o - a_p| / a_o), a = |FFT| summed over a `window`-bin
//               box, scipy.ndimage.convolve1d(mode='reflect')                  (:38-40)
//   Envelope  = mean(|env_o - env_p| / max_row env_o), env = |hilbert(x)|      (:43-45)
//   energy    = 10 log10 of the reversed cumulative sum of x^2 + 1e-9, minus
//               its first sample: both curves are outputs                      (:48-52)
//   T60, EDT  = per row from the curve (t60_EDT_cal, :77-136): nearest samples
//               to -10 / -5 / -25 dB, least-squares slope between the last two;
//               T60 = mean(|o - p| / o), EDT = mean|o - p|                     (:55-58)
//   C50       = mean|c_o - c_p|, c = 10 log10(early / late energy), split at
//               s50 = int(0.05 fs)                                             (:61-72)
//   multi_stft= auraloss MR-STFT, fft 512/256/128: the criterion's resolutions
//               0-2 (criterion.hip, launch_mr3)                                (:31-32)
//
// Launches: met_dft_kernel (dense real DFT of every row, bins 0..n/2, integer
// twiddle index (k t) mod n), met_hilbert_kernel (imaginary part of the
// analytic signal: a dense inverse transform of the one-sided spectrum, then
// the envelope), met_energy_kernel (one workgroup per row and signal: scan,
// curve, the three crossings, regression in double, C50), met_pair_kernel
// (one workgroup per row: angle, amplitude, envelope sums), the criterion's
// STFT kernel + crit_mr3_reduce_kernel, met_final_kernel (batch means, rows in
// order).  Every sum is in a fixed order: results repeat bitwise and a row's
// values do not depend on its batch.  All LDS is static, sized for n <= 12288.
#include <math.h>

#include "block.h"
#include "common.h"

using namespace avr;

namespace {

constexpr int kT = 256;         // lanes per workgroup, every kernel below
constexpr int kMaxN = 12288;    // the criterion's IR length limit
constexpr int kMinN = 256;      // n must exceed it (512-point STFT reflect pad)
constexpr int kMaxK = kMaxN / 2 + 1;
constexpr int kChunk = 1024;    // samples (or bins) staged in LDS per round
constexpr int kCols = AVR_METRICS_COLS;
constexpr int kLdsLimit = 64 * 1024;
static_assert(kChunk % 4 == 0, "the transforms walk four taps per round");

struct MetWs {
    void* mr;      // the criterion's workspace for the MR-STFT term
    float2* X;     // [2][B][n/2+1] half spectra, ori (0) then pred (1)
    float* env;    // [2][B][n] envelopes
    int64_t mr_bytes, bytes;
};

int check_shape(int B, int n) {
    AVR_REQUIRE(B >= 1 && B <= 256, "avr_metrics: 1 <= B <= 256 required");
    AVR_REQUIRE(n % 2 == 0, "avr_metrics: IR length n must be even");
    AVR_REQUIRE(n > kMinN && n <= kMaxN, "avr_metrics: IR length must satisfy 256 < n <= 12288");
    return 0;
}

int carve(int B, int n, void* base, MetWs* W) {
    int64_t mr = 0;
    if (int e = mr3_workspace(B, n, &mr)) return e;
    Arena A(base, 16);
    const int64_t K = n / 2 + 1;
    W->mr = A.take<char>(mr);
    W->mr_bytes = mr;
    W->X = A.take<float2>(2 * (int64_t)B * K);
    W->env = A.take<float>(2 * (int64_t)B * n);
    W->bytes = A.bytes();
    return 0;
}

// ------------------------------------------------------------ half spectrum
// X[k] = sum_t x[t] (cos - i sin)(2 pi k t / n), k = 0..n/2.  One lane per
// bin, the row staged through LDS kChunk samples at a time, four independent
// accumulators (taps t = u mod 4).  tw = avr_ir_twiddle(n): (cos, sin)(2 pi j/n).
__global__ __launch_bounds__(kT) void met_dft_kernel(int B, int n, const float* __restrict__ ori,
                                                     const float* __restrict__ pred,
                                                     const float2* __restrict__ tw,
                                                     float2* __restrict__ X) {
    __shared__ float xs[kChunk];
    const int tid = threadIdx.x;
    const int K = n / 2 + 1;
    const int row = blockIdx.y;  // s * B + b
    const int s = row >= B, b = row - s * B;
    const float* x = (s ? pred : ori) + (int64_t)b * n;
    const int k = blockIdx.x * kT + tid;
    const int kk = k < K ? k : 0;  // lanes past the last bin walk bin 0 and store nothing
    const int step = (int)(((int64_t)kk * 4) % n);
    int idx[4];
    float re[4], im[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        idx[u] = (kk * u) % n;
        re[u] = 0.f;
        im[u] = 0.f;
    }
    for (int t0 = 0; t0 < n; t0 += kChunk) {
        __syncthreads();
        for (int i = tid; i < kChunk; i += kT) xs[i] = t0 + i < n ? x[t0 + i] : 0.f;
        __syncthreads();
        const int len = min(kChunk, n - t0);
        for (int i = 0; i < len; i += 4) {  // the last round's missing taps are zeros
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float2 c = tw[idx[u]];  // idx < n always
                const float v = xs[i + u];
                re[u] = fmaf(v, c.x, re[u]);
                im[u] = fmaf(-v, c.y, im[u]);
                idx[u] += step;
                if (idx[u] >= n) idx[u] -= n;
            }
        }
    }
    if (k >= K) return;
    const float r = (re[0] + re[1]) + (re[2] + re[3]);
    float m = (im[0] + im[1]) + (im[2] + im[3]);
    if (k == 0 || k == K - 1) m = 0.f;  // a real signal's DC and Nyquist bins are real
    X[(int64_t)row * K + k] = make_float2(r, m);
}

// --------------------------------------------------------------- envelope
// scipy.signal.hilbert: the analytic signal is the inverse DFT of the
// one-sided spectrum (X[0], X[n/2] once, the bins between twice).  Its real
// part is x; its imaginary part is
//   h[t] = (1/n) sum_k w_k (Re X_k sin(2 pi k t/n) + Im X_k cos(2 pi k t/n)).
// One lane per sample, the weighted bins staged through LDS.
__global__ __launch_bounds__(kT) void met_hilbert_kernel(int B, int n, const float* __restrict__ ori,
                                                         const float* __restrict__ pred,
                                                         const float2* __restrict__ tw,
                                                         const float2* __restrict__ X,
                                                         float* __restrict__ env) {
    __shared__ float2 Xs[kChunk];
    const int tid = threadIdx.x;
    const int K = n / 2 + 1;
    const int row = blockIdx.y;
    const int s = row >= B, b = row - s * B;
    const float2* Xr = X + (int64_t)row * K;
    const int t = blockIdx.x * kT + tid;
    const int tt = t < n ? t : 0;
    const int step = (int)(((int64_t)tt * 4) % n);
    const float inv = 1.0f / (float)n;
    int idx[4];
    float h[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        idx[u] = (int)(((int64_t)tt * u) % n);
        h[u] = 0.f;
    }
    for (int k0 = 0; k0 < K; k0 += kChunk) {
        __syncthreads();
        for (int i = tid; i < kChunk; i += kT) {
            const int k = k0 + i;
            float2 v = make_float2(0.f, 0.f);
            if (k < K) {
                v = Xr[k];
                const float w = (k == 0 || k == K - 1) ? inv : 2.0f * inv;
                v.x *= w;
                v.y *= w;
            }
            Xs[i] = v;
        }
        __syncthreads();
        const int len = min(kChunk, K - k0);
        for (int i = 0; i < len; i += 4) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float2 c = tw[idx[u]];
                const float2 v = Xs[i + u];
                h[u] = fmaf(v.x, c.y, h[u]);
                h[u] = fmaf(v.y, c.x, h[u]);
                idx[u] += step;
                if (idx[u] >= n) idx[u] -= n;
            }
        }
    }
    if (t >= n) return;
    const float im = (h[0] + h[1]) + (h[2] + h[3]);
    const float xr = (s ? pred : ori)[(int64_t)b * n + t];
    env[(int64_t)row * n + t] = hypotf(xr, im);
}

// ---------------------------------------------------- energy curve, T60, EDT, C50
// One workgroup per (row, signal).  The reversed cumulative sum: lane i owns
// samples [i L, (i+1) L), sums them from the end, lane 0 turns the 256 segment
// totals into suffix offsets from the end, and each lane then walks its
// segment again from the end on top of its offset.
struct EnergyLds {
    float S[kMaxN];      // x, then the cumulative sum, then the curve
    float seg[kT];
    double red[4][kT];   // regression sums; C50 and nearest-sample scratch before that
};
struct Nearest {  // distance to a target level and the sample it is at
    float d;
    int t;
};
static_assert(sizeof(EnergyLds) <= kLdsLimit, "met_energy_kernel: LDS over 64 KB");
static_assert(sizeof(double) * 4 >= sizeof(Nearest) * 3 && sizeof(double) * 4 >= sizeof(float) * 2,
              "the scratch fits the double rows");

__global__ __launch_bounds__(kT) void met_energy_kernel(int B, int n, double fs, int s50,
                                                        const float* __restrict__ ori,
                                                        const float* __restrict__ pred,
                                                        float* __restrict__ rows,
                                                        float* __restrict__ ori_energy,
                                                        float* __restrict__ pred_energy) {
    __shared__ EnergyLds L;
    const int tid = threadIdx.x;
    const int b = blockIdx.x, s = blockIdx.y;
    const float* x = (s ? pred : ori) + (int64_t)b * n;
    float* out = (s ? pred_energy : ori_energy) + (int64_t)b * n;
    for (int i = tid; i < n; i += kT) L.S[i] = x[i];
    __syncthreads();
    const int seg_len = (n + kT - 1) / kT;
    const int lo = min(tid * seg_len, n), hi = min(lo + seg_len, n);
    float tot = 0.f, el[2] = {0.f, 0.f};
    for (int j = hi - 1; j >= lo; --j) {
        const float sq = L.S[j] * L.S[j];
        tot += sq + 1e-9f;
        el[j >= s50] += sq;
    }
    L.seg[tid] = tot;
    block_reduce<kT, 2>(reinterpret_cast<float(*)[kT]>(L.red), el, SumOp{});  // early, late energy
    if (tid == 0) {
        float run = 0.f;
        for (int i = kT - 1; i >= 0; --i) {
            const float t = L.seg[i];
            L.seg[i] = run;
            run += t;
        }
    }
    __syncthreads();
    float run = L.seg[tid];
    for (int j = hi - 1; j >= lo; --j) {
        run += L.S[j] * L.S[j] + 1e-9f;
        L.S[j] = run;
    }
    __syncthreads();
    // curve, and the first sample nearest each of -10, -5, -25 dB
    const float e0 = 10.0f * log10f(L.S[0]);
    __syncthreads();
    const float target[3] = {-10.0f, -5.0f, -25.0f};
    Nearest best[3] = {{INFINITY, n - 1}, {INFINITY, n - 1}, {INFINITY, n - 1}};
    for (int t = tid; t < n; t += kT) {
        const float e = 10.0f * log10f(L.S[t]) - e0;
        L.S[t] = e;
        out[t] = e;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float d = fabsf(e - target[c]);
            if (d < best[c].d) best[c] = Nearest{d, t};  // t ascends: the first minimum stays
        }
    }
    // the smallest distance over the lanes, the earliest sample among equals
    block_reduce<kT, 3>(reinterpret_cast<Nearest(*)[kT]>(L.red), best, [](Nearest a, Nearest b) {
        return (b.d < a.d || (b.d == a.d && b.t < a.t)) ? b : a;
    });
    const int i10 = min(max(best[0].t, 0), n - 1), i5 = min(max(best[1].t, 0), n - 1),
              i25 = min(max(best[2].t, 0), n - 1);
    // least squares of E[i5..i25] on u = t - i5 (stats.linregress on t / fs:
    // the slope per second is the slope per sample times fs)
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    for (int t = i5 + tid; t <= i25; t += kT) {
        const double u = (double)(t - i5), y = (double)L.S[t];
        a[0] += u;
        a[1] += y;
        a[2] += u * u;
        a[3] += u * y;
    }
    block_reduce<kT, 4>(L.red, a, SumOp{});
    if (tid == 0) {
        float t60 = NAN;
        if (i25 > i5) {
            const double N = (double)(i25 - i5 + 1);
            const double su = a[0], sy = a[1], suu = a[2], suy = a[3];
            const double slope = (N * suy - su * sy) / (N * suu - su * su) * fs;
            if (slope != 0.0) t60 = (float)(3.0 * (-20.0) / slope);
        }
        float* r = rows + (int64_t)b * kCols;
        r[0 + s] = t60;
        r[2 + s] = (float)((double)i10 / fs * 6.0);
        r[4 + s] = 10.0f * log10f(el[0] / el[1]);  // late = 0 gives inf, as the reference
    }
}

// ------------------------------------------------- angle, amplitude, envelope
// One workgroup per row, both signals' magnitudes in LDS.
struct PairLds {
    float mag[2][kMaxK];
    float red[3][kT];
};
static_assert(sizeof(PairLds) <= kLdsLimit, "met_pair_kernel: LDS over 64 KB");

__global__ __launch_bounds__(kT) void met_pair_kernel(int B, int n, int window,
                                                      const float2* __restrict__ X,
                                                      const float* __restrict__ env,
                                                      float* __restrict__ rows) {
    __shared__ PairLds L;
    const int tid = threadIdx.x;
    const int b = blockIdx.x;
    const int K = n / 2 + 1;
    const float2* Xo = X + (int64_t)b * K;
    const float2* Xp = X + ((int64_t)B + b) * K;
    float acc[3] = {0.f, 0.f, 0.f};
    // bins 0 and n/2 of the n-bin spectrum once, the others with their mirror
    // (conjugate: same cosine, negated sine, same absolute differences)
    for (int k = tid; k < K; k += kT) {
        const float2 o = Xo[k], p = Xp[k];
        L.mag[0][k] = hypotf(o.x, o.y);
        L.mag[1][k] = hypotf(p.x, p.y);
        const float to = atan2f(o.y, o.x), tp = atan2f(p.y, p.x);
        const float d = fabsf(cosf(to) - cosf(tp)) + fabsf(sinf(to) - sinf(tp));
        acc[0] += (k == 0 || k == K - 1) ? d : 2.0f * d;
    }
    __syncthreads();
    // convolve1d(|fft|, ones(window)), mode='reflect' (d c b a | a b c d | d c b a):
    // output i sums inputs i + window/2 - window + 1 .. i + window/2
    for (int i = tid; i < n; i += kT) {
        const int hi = i + window / 2, lo = hi - window + 1;
        float so = 0.f, sp = 0.f;
        for (int j = lo; j <= hi; ++j) {
            int jj = j < 0 ? -j - 1 : (j >= n ? 2 * n - 1 - j : j);  // in [0, n): window <= n
            jj = min(max(jj, 0), n - 1);
            const int h = min(jj, n - jj);  // full-spectrum bin -> half-spectrum bin, <= n/2
            so += L.mag[0][h];
            sp += L.mag[1][h];
        }
        acc[1] += fabsf(so - sp) / so;
    }
    const float* eo = env + (int64_t)b * n;
    const float* ep = env + ((int64_t)B + b) * n;
    float mx = 0.f;
    for (int t = tid; t < n; t += kT) mx = fmaxf(mx, eo[t]);
    mx = block_max<kT>(mx, L.red[0]);
    for (int t = tid; t < n; t += kT) acc[2] += fabsf(eo[t] - ep[t]) / mx;
    block_reduce<kT, 3>(L.red, acc, SumOp{});
    if (tid < 3) rows[(int64_t)b * kCols + 6 + tid] = acc[tid];
}

// means[0..5] = Angle, Amplitude, Envelope, T60, EDT, C50 over the rows in
// order (means[6], multi_stft, comes from crit_mr3_reduce_kernel)
__global__ void met_final_kernel(int B, int n, const float* __restrict__ rows,
                                 float* __restrict__ means) {
    const int c = threadIdx.x;
    if (c >= 6) return;
    float sum = 0.f;
    for (int b = 0; b < B; ++b) {
        const float* r = rows + (int64_t)b * kCols;
        if (c < 3)
            sum += r[6 + c];
        else if (c == 3)
            sum += fabsf(r[0] - r[1]) / r[0];
        else
            sum += fabsf(r[2 * (c - 3)] - r[2 * (c - 3) + 1]);
    }
    means[c] = c < 3 ? sum / ((float)B * (float)n) : sum / (float)B;
}

}  // namespace

extern "C" int avr_metrics_workspace(int32_t B, int32_t n, int64_t* bytes) {
    if (int e = check_shape(B, n)) return e;
    AVR_REQUIRE(bytes, "avr_metrics_workspace: null bytes");
    MetWs W{};
    if (int e = carve(B, n, nullptr, &W)) return e;
    *bytes = W.bytes;
    return 0;
}

extern "C" int avr_metrics(int32_t B, int32_t n, double fs, int32_t s50, int32_t window,
                           const float* ori, const float* pred, const float* ir_twiddle,
                           const float* win_table, const float* tw512, float* rows, float* means,
                           float* ori_energy, float* pred_energy, void* ws, int64_t ws_bytes,
                           void* stream) {
    if (int e = check_shape(B, n)) return e;
    AVR_REQUIRE(window >= 1 && window <= n, "avr_metrics: 1 <= window <= n required");
    AVR_REQUIRE(fs > 0.0, "avr_metrics: fs must be positive");
    AVR_REQUIRE(s50 >= 0, "avr_metrics: s50 must not be negative");
    AVR_REQUIRE(ori && pred && ir_twiddle && win_table && tw512 && rows && means && ori_energy &&
                    pred_energy && ws,
                "avr_metrics: null pointer");
    MetWs W{};
    if (int e = carve(B, n, ws, &W)) return e;
    AVR_REQUIRE(ws_bytes >= W.bytes, "avr_metrics: workspace too small");
    const int K = n / 2 + 1;
    const float2* tw = reinterpret_cast<const float2*>(ir_twiddle);
    hipStream_t st = as_stream(stream);
    if (int e = launch("met_dft_kernel", met_dft_kernel, dim3((K + kT - 1) / kT, 2 * B), dim3(kT), 0, st, B, n, ori,
                       pred, tw, W.X))
        return e;
    if (int e = launch("met_hilbert_kernel", met_hilbert_kernel, dim3((n + kT - 1) / kT, 2 * B), dim3(kT), 0, st, B,
                       n, ori, pred, tw, W.X, W.env))
        return e;
    if (int e = launch("met_energy_kernel", met_energy_kernel, dim3(B, 2), dim3(kT), 0, st, B, n, fs, s50, ori, pred,
                       rows, ori_energy, pred_energy))
        return e;
    if (int e = launch("met_pair_kernel", met_pair_kernel, dim3(B), dim3(kT), 0, st, B, n, window, W.X, W.env, rows))
        return e;
    // auraloss is called as (ori, pred): the criterion's argument order
    if (int e = launch_mr3(B, n, pred, ori, win_table, tw512, W.mr, W.mr_bytes, means + 6, stream))
        return e;
    return launch("met_final_kernel", met_final_kernel, dim3(1), dim3(64), 0, st, B, n, rows, means);
}
