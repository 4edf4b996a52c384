// doa.hip — direction-of-arrival evaluation on gfx950.
//
//   avr_doa_das          plot_eval.py:134-265 run_delay_and_sum_on_npz for all
//                        G groups of 8 microphones and for the predicted and
//                        the measured IRs together: three launches
//                          doa_das_spectrum_kernel  X = rfft(ir, n = n_fft), one
//                                                   workgroup per row, fp64
//                          doa_das_power_kernel     one workgroup per 16 bins
//                                                   and (signal, group): all K
//                                                   beams, normalised per bin
//                          doa_das_finish_kernel    one workgroup per group:
//                                                   power, argmax, soft-argmax,
//                                                   true_deg, the three errors
//                        The steering table is the reference's own (host torch
//                        ops, fp32); everything summed on the device is fp64 in
//                        a fixed order, so the result carries the rounding of
//                        the reference's inputs and none of its own.
//   avr_doa_frames       the frame-wise narrow-band estimators (SRP-PHAT,
//                        MUSIC and NormMUSIC for one source) on [G][8][n]
//                        signals: ONE launch, one workgroup per (group, frame):
//                        dense DFT over the wanted bins, 8x8 covariances,
//                        cyclic complex Jacobi (eight lanes per matrix),
//                        pseudo-spectrum over 360 directions, first argmax.
//                        fp32 arithmetic, fixed summation orders, no float
//                        atomics: bitwise repeatable and independent of the
//                        batch.
//   avr_doa_frame_stats  whitenoise_bandpass_doa.py:36-49 circ_stats_deg over
//                        the valid frames of each group, fp64.
#include <math.h>

#include "block.h"
#include "common.h"

using namespace avr;

namespace {

constexpr int kMics = 8;
constexpr int kThreads = 256;

// Python's float % 360 (numpy's remainder): the sign of the divisor
__device__ __forceinline__ double mod360(double a) {
    double r = fmod(a, 360.0);
    if (r != 0.0 && r < 0.0) r += 360.0;
    return r;
}
// plot_eval.py:15 angular_error_deg
__device__ __forceinline__ double ang_err(double a, double b) {
    const double d = fabs(a - b);
    return fmin(d, 360.0 - d);
}

// ------------------------------------------------------------- NormDAS
constexpr int kDasFTile = 16;
constexpr int kDasMaxNfft = 2048;
constexpr int kDasMaxDirs = 1024;

struct DasDoaWs {
    double2* X;     // [2][G][8][F]
    double* ppart;  // [2][G][tiles][K]
    int64_t bytes;
};

DasDoaWs das_carve(void* base, int64_t G, int F, int K) {
    DasDoaWs W{};
    Arena A(base, 16);
    const int tiles = (F + kDasFTile - 1) / kDasFTile;
    W.X = A.take<double2>(2 * G * kMics * F);
    W.ppart = A.take<double>(2 * G * tiles * K);
    W.bytes = A.bytes();
    return W;
}

// X[s][row][f] = sum_{t < min(n, nfft)} ir[row][t] e^{-2 pi i f t / nfft}
// tw[j] = (cos, -sin)(2 pi j / nfft) in fp64 (host table)
__global__ __launch_bounds__(kThreads) void doa_das_spectrum_kernel(
    int n, int nfft, int F, const float* __restrict__ pred, const float* __restrict__ ori,
    const double2* __restrict__ tw, double2* __restrict__ X) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double2* stw = reinterpret_cast<double2*>(smem);   // [nfft]
    float* x = reinterpret_cast<float*>(stw + nfft);   // [nfft]
    const int64_t row = blockIdx.x;
    const int s = blockIdx.y;
    const float* src = (s ? ori : pred) + row * n;
    const int L = min(n, nfft);
    for (int i = threadIdx.x; i < nfft; i += kThreads) {
        stw[i] = tw[i];
        x[i] = i < L ? src[i] : 0.f;
    }
    __syncthreads();
    double2* out = X + ((int64_t)s * gridDim.x + row) * F;
    for (int f = threadIdx.x; f < F; f += kThreads) {
        double re = 0.0, im = 0.0;
        int j = 0;
        for (int t = 0; t < L; ++t) {
            const double2 c = stw[j];
            const double v = (double)x[t];
            re = fma(v, c.x, re);
            im = fma(v, c.y, im);
            j += f;
            if (j >= nfft) j -= nfft;
        }
        out[f] = make_double2(re, im);
    }
}

// |beam|^2 for 16 bins x K directions of one (signal, group), normalised
// over the directions per bin, summed over the tile's bins.
__global__ __launch_bounds__(kThreads) void doa_das_power_kernel(
    int F, int K, const float2* __restrict__ steer, const double2* __restrict__ X,
    double* __restrict__ ppart) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double2* xs = reinterpret_cast<double2*>(smem);            // [8][16]
    double* inv = reinterpret_cast<double*>(xs + kMics * kDasFTile);  // [16]
    double* bp = inv + kDasFTile;                              // [K][17]
    const int tile = blockIdx.x;
    const int64_t sg = blockIdx.y;
    const int f0 = tile * kDasFTile;
    const int nf = min(kDasFTile, F - f0);
    for (int i = threadIdx.x; i < kMics * kDasFTile; i += kThreads) {
        const int m = i / kDasFTile, j = i % kDasFTile;
        xs[i] = j < nf ? X[(sg * kMics + m) * F + f0 + j] : make_double2(0.0, 0.0);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < K * kDasFTile; i += kThreads) {
        const int k = i / kDasFTile, j = i % kDasFTile;
        double re = 0.0, im = 0.0;
        if (j < nf) {
#pragma unroll
            for (int m = 0; m < kMics; ++m) {
                const double2 a = xs[m * kDasFTile + j];
                const float2 b = steer[((int64_t)k * kMics + m) * F + f0 + j];
                re += a.x * (double)b.x - a.y * (double)b.y;
                im += a.x * (double)b.y + a.y * (double)b.x;
            }
            re /= (double)kMics;
            im /= (double)kMics;
        }
        bp[k * (kDasFTile + 1) + j] = re * re + im * im;
    }
    __syncthreads();
    if (threadIdx.x < kDasFTile) {
        const int j = threadIdx.x;
        double sum = 0.0;
        for (int k = 0; k < K; ++k) sum += bp[k * (kDasFTile + 1) + j];
        inv[j] = sum + 1e-8;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < K; k += kThreads) {
        double p = 0.0;
        for (int j = 0; j < nf; ++j) p += bp[k * (kDasFTile + 1) + j] / inv[j];
        ppart[(sg * gridDim.x + tile) * K + k] = p;
    }
}

struct DasDoaOut {
    double soft, arg;
};

// power = sum of the tile partials; first argmax; softmax(beta power) angle
__device__ DasDoaOut das_doa_stats(const double* __restrict__ ppart, int tiles, int K,
                                   const float* __restrict__ angles, double beta, double* pw,
                                   double* red, int* redi) {
    double lmax = -INFINITY;
    for (int k = threadIdx.x; k < K; k += kThreads) {
        double p = 0.0;
        for (int t = 0; t < tiles; ++t) p += ppart[(int64_t)t * K + k];
        pw[k] = p;
        lmax = fmax(lmax, p);
    }
    const double mx = block_max<kThreads>(lmax, red);
    int first = 0x7fffffff;
    for (int k = threadIdx.x; k < K; k += kThreads)
        if (pw[k] == mx) {
            first = k;
            break;
        }
    const int idx = block_min<kThreads>(first, redi);
    double se = 0.0;
    for (int k = threadIdx.x; k < K; k += kThreads) se += exp(beta * pw[k] - beta * mx);
    const double sum = block_sum<kThreads>(se, red);
    double sa = 0.0;
    for (int k = threadIdx.x; k < K; k += kThreads)
        sa += exp(beta * pw[k] - beta * mx) / sum * (double)angles[k];
    const double soft = block_sum<kThreads>(sa, red);
    DasDoaOut o;
    o.soft = mod360(soft);
    o.arg = mod360((double)angles[idx < K ? idx : 0]);
    return o;
}

// ---- atan2 rounded once.  The reference's errors against true_deg are
// compared bit for bit, and the device library's atan2 is accurate to an ulp
// but does not always round as libm does (one group in thirteen differed in
// the last bit).  So: double-double arithmetic, atan(z) = atan(i/32) +
// atan((z - i/32) / (1 + z i/32)) with a table of atan(i/32) and the odd
// series for the small remainder, rounded to double at the very end.
struct dd {
    double hi, lo;
};
__device__ __forceinline__ dd quick_two_sum(double a, double b) {
    const double s = a + b;
    return dd{s, b - (s - a)};
}
__device__ __forceinline__ dd dd_add(dd x, dd y) {
    const double s = x.hi + y.hi;
    const double bb = s - x.hi;
    const double e = ((x.hi - (s - bb)) + (y.hi - bb)) + (x.lo + y.lo);
    return quick_two_sum(s, e);
}
__device__ __forceinline__ dd dd_mul_d(dd x, double b) {
    const double p = x.hi * b;
    const double e = fma(x.hi, b, -p) + x.lo * b;
    return quick_two_sum(p, e);
}
__device__ __forceinline__ dd dd_neg(dd x) { return dd{-x.hi, -x.lo}; }
__device__ dd dd_div(dd x, dd y) {
    const double q1 = x.hi / y.hi;
    dd r = dd_add(x, dd_neg(dd_add(dd_mul_d(dd{y.hi, 0.0}, q1), dd_mul_d(dd{y.lo, 0.0}, q1))));
    const double q2 = r.hi / y.hi;
    r = dd_add(r, dd_neg(dd_add(dd_mul_d(dd{y.hi, 0.0}, q2), dd_mul_d(dd{y.lo, 0.0}, q2))));
    const double q3 = r.hi / y.hi;
    return dd_add(quick_two_sum(q1, q2), dd{q3, 0.0});
}
__constant__ double kAtanTab[33][2] = {
    {0x0.0p+0, 0x0.0p+0},
    {0x1.ffd55bba97625p-6, -0x1.5ec431444912cp-60},
    {0x1.ff55bb72cfdeap-5, -0x1.c934d86d23f1dp-60},
    {0x1.7ee182602f10fp-4, -0x1.cfb654c0c3d98p-58},
    {0x1.fd5ba9aac2f6ep-4, -0x1.cd37686760c17p-59},
    {0x1.3d6eee8c6626cp-3, 0x1.61a3b0ce9281bp-57},
    {0x1.7b97b4bce5b02p-3, 0x1.347b0b4f881cap-58},
    {0x1.b90d7529260a2p-3, 0x1.17b10d2e0e5abp-61},
    {0x1.f5b75f92c80ddp-3, 0x1.8ab6e3cf7afbdp-57},
    {0x1.18bf5a30bf178p-2, 0x1.30ca4748b1bf9p-57},
    {0x1.362773707ebccp-2, -0x1.963a544b672d8p-57},
    {0x1.530ad9951cd4ap-2, -0x1.2566480884082p-57},
    {0x1.6f61941e4def1p-2, -0x1.c63aae6f6e918p-56},
    {0x1.8b24d394a1b25p-2, 0x1.b6d0ba3748fa8p-56},
    {0x1.a64eec3cc23fdp-2, -0x1.24dec1b50b7ffp-56},
    {0x1.c0db4c94ec9f0p-2, -0x1.cc1ce70934c34p-56},
    {0x1.dac670561bb4fp-2, 0x1.a2b7f222f65e2p-56},
    {0x1.f40dd0b541418p-2, -0x1.a3992dc382a23p-57},
    {0x1.0657e94db30d0p-1, -0x1.d5b495f6349e6p-56},
    {0x1.1255d9bfbd2a9p-1, -0x1.2bdaee1c0ee35p-58},
    {0x1.1e00babdefeb4p-1, -0x1.928df287a668fp-58},
    {0x1.2958e59308e31p-1, -0x1.09e73b0c6c087p-56},
    {0x1.345f01cce37bbp-1, 0x1.1021137c71102p-55},
    {0x1.3f13fb89e96f4p-1, 0x1.ecf8b492644f0p-56},
    {0x1.4978fa3269ee1p-1, 0x1.2419a87f2a458p-56},
    {0x1.538f57b89061fp-1, -0x1.1bb74abda520cp-55},
    {0x1.5d58987169b18p-1, 0x1.0028e4bc5e7cap-57},
    {0x1.66d663923e087p-1, -0x1.6ea6febe8bbbap-56},
    {0x1.700a7c5784634p-1, -0x1.8c34d25aadef6p-56},
    {0x1.78f6bbd5d315ep-1, 0x1.406a089803740p-55},
    {0x1.819d0b7158a4dp-1, -0x1.bf76229d3b917p-56},
    {0x1.89ff5ff57f1f8p-1, -0x1.55b9a5e177a1bp-55},
    {0x1.921fb54442d18p-1, 0x1.1a62633145c07p-55},
};
// atan of z in [0, 1]
__device__ dd atan_dd(dd z) {
    const int i = (int)rint(z.hi * 32.0);
    const double c = (double)i / 32.0;
    const dd t = dd_div(dd_add(z, dd{-c, 0.0}), dd_add(dd{1.0, 0.0}, dd_mul_d(z, c)));  // |t| <= 1/64
    const double u = t.hi, u2 = u * u;
    // t^3/3 - t^5/5 + ... - t^15/15 (below 1.3e-6 |t|: plain double is enough)
    const double p = u2 * u *
                     (1.0 / 3 - u2 * (1.0 / 5 - u2 * (1.0 / 7 - u2 * (1.0 / 9 - u2 * (1.0 / 11 - u2 * (1.0 / 13 - u2 / 15))))));
    return dd_add(dd{kAtanTab[i][0], kAtanTab[i][1]}, dd_add(t, dd{-p, 0.0}));
}
__device__ double atan2_once(double y, double x) {
    const double ax = fabs(x), ay = fabs(y);
    if (!(ax > 0.0 || ay > 0.0) || isinf(ax) || isinf(ay) || ax != ax || ay != ay) return atan2(y, x);
    const dd pi{0x1.921fb54442d18p+1, 0x1.1a62633145c07p-53}, half_pi{0x1.921fb54442d18p+0, 0x1.1a62633145c07p-54};
    dd a;
    if (ay <= ax)
        a = atan_dd(dd_div(dd{ay, 0.0}, dd{ax, 0.0}));
    else
        a = dd_add(half_pi, dd_neg(atan_dd(dd_div(dd{ax, 0.0}, dd{ay, 0.0}))));
    if (x < 0.0) a = dd_add(pi, dd_neg(a));
    return copysign(a.hi + a.lo, y);
}

// true_deg (plot_eval.py:179-187): the group's mean receiver position in xy
// (numpy's mean over 8 rows in the positions' own precision), its first
// transmitter row, atan2 in fp64.
template <typename T>
__device__ double true_deg_of(const T* __restrict__ rx, const T* __restrict__ tx, int64_t g) {
    T cx = (T)0, cy = (T)0;
    for (int m = 0; m < kMics; ++m) {
        cx = cx + rx[(g * kMics + m) * 3 + 0];
        cy = cy + rx[(g * kMics + m) * 3 + 1];
    }
    cx = cx / (T)kMics;
    cy = cy / (T)kMics;
    const T dx = tx[g * kMics * 3 + 0] - cx;
    const T dy = tx[g * kMics * 3 + 1] - cy;
    const double rad = atan2_once((double)dy, (double)dx);
    return mod360(rad * (180.0 / 3.14159265358979323846));
}

__global__ __launch_bounds__(kThreads) void doa_das_finish_kernel(
    int64_t G, int tiles, int K, const float* __restrict__ angles, double beta,
    const double* __restrict__ ppart, const void* __restrict__ rx, const void* __restrict__ tx,
    int pos_f64, double* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* red = reinterpret_cast<double*>(smem);  // [256]
    double* pw = red + kThreads;                    // [K]
    int* redi = reinterpret_cast<int*>(pw + K + (K & 1));  // [256]
    const int64_t g = blockIdx.x;
    const DasDoaOut p = das_doa_stats(ppart + (0 * G + g) * tiles * K, tiles, K, angles, beta, pw, red, redi);
    __syncthreads();
    const DasDoaOut o = das_doa_stats(ppart + (1 * G + g) * tiles * K, tiles, K, angles, beta, pw, red, redi);
    if (threadIdx.x == 0) {
        const double t = pos_f64 ? true_deg_of(static_cast<const double*>(rx), static_cast<const double*>(tx), g)
                                 : true_deg_of(static_cast<const float*>(rx), static_cast<const float*>(tx), g);
        // out[method][key][G]; method 0 soft-argmax, 1 argmax; keys true, pred,
        // gt, pred_vs_gt, pred_vs_true, gt_vs_true
        for (int meth = 0; meth < 2; ++meth) {
            const double pd = meth ? p.arg : p.soft, gd = meth ? o.arg : o.soft;
            double* q = out + (int64_t)meth * 6 * G + g;
            q[0 * G] = t;
            q[1 * G] = pd;
            q[2 * G] = gd;
            q[3 * G] = ang_err(pd, gd);
            q[4 * G] = ang_err(pd, t);
            q[5 * G] = ang_err(gd, t);
        }
    }
}

int das_doa_shape(int64_t G, int32_t n, int32_t nfft, int32_t K) {
    AVR_REQUIRE(G >= 1 && G <= 32767, "avr_doa_das: 1 <= G <= 32767 required");
    AVR_REQUIRE(n >= 1, "avr_doa_das: n must be positive");
    AVR_REQUIRE(nfft >= 2 && nfft <= kDasMaxNfft && nfft % 2 == 0,
                "avr_doa_das: n_fft must be even and in [2, 2048]");
    AVR_REQUIRE(K >= 1 && K <= kDasMaxDirs, "avr_doa_das: 1 <= directions <= 1024 required");
    return 0;
}

// ------------------------------------------------------- frame estimators
constexpr int kFrKC = 32;        // bins per chunk (= matrices per Jacobi batch)
constexpr int kFrDirs = 360;
constexpr int kFrSweeps = 8;     // converged after 6 on every scene tried
constexpr int kFrChains = 16;    // partial sums of the DFT
constexpr int kFrMat = 65;       // float2 stride of one 8x8 matrix in LDS
constexpr int kFrMaxNfft = 2048;

enum { kAlgoSrp = 0, kAlgoMusic = 1, kAlgoNormMusic = 2 };

struct FrArgs {
    const void* y;  // [G][8][n]
    int32_t y_f64;
    int64_t n, n_frames;
    int32_t L, H, nfft, hop, J, k_lo, K, algo;  // bins k_lo .. k_lo + K - 1
    float floor8;         // 8 * floor
    const float2* tw;     // [nfft] (cos, -sin)(2 pi j / nfft)
    const float* win;     // [nfft]
    const float2* steer;  // [K][8][360]
    int32_t* est;         // [G][n_frames]
    uint8_t* valid;       // [G][n_frames]
    float* spec;          // [G][n_frames][360] or null
};

inline size_t frames_lds(int nfft) {
    size_t b = 0;
    b += align_up((int64_t)nfft * sizeof(float2), 16);              // stw
    b += align_up((int64_t)kMics * nfft * sizeof(float), 16);       // wy
    b += kMics * kFrKC * sizeof(float2);                            // xs
    b += 2 * align_up((int64_t)kFrKC * kFrMat * sizeof(float2), 16);  // A, V
    b += kFrKC * 4 * sizeof(float4);                                // prm
    b += kFrKC * kMics * sizeof(float2);                            // ev
    b += kFrKC * sizeof(uint32_t);                                  // dmin
    b += align_up(kFrDirs * sizeof(float), 16);                     // P
    b += kThreads * sizeof(float) + kThreads * sizeof(int);         // red, redi
    return b;
}

__device__ __forceinline__ float ld_y(const FrArgs& a, int64_t off) {
    return a.y_f64 ? (float)static_cast<const double*>(a.y)[off] : static_cast<const float*>(a.y)[off];
}

// pair i of round r of the round-robin order on 8 indices (7 rounds of 4
// disjoint pairs), p < q
__device__ __forceinline__ void jacobi_pair(int r, int i, int& p, int& q) {
    int u, v;
    if (i == 0) {
        u = r;
        v = 7;
    } else {
        u = (r + i) % 7;
        v = (r + 7 - i) % 7;
    }
    p = min(u, v);
    q = max(u, v);
}

__device__ __forceinline__ float2 cmul(float2 a, float2 b) {
    return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
// a * conj(b)
__device__ __forceinline__ float2 cmulc(float2 a, float2 b) {
    return make_float2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y);
}

// One workgroup per (group, frame).  Bins are taken in chunks of 32; per
// chunk: (1) thread (mic m, bin k) transforms every snapshot's windowed
// segment (staged in LDS) at its bin and keeps row m of R_k in registers,
// (2) eight lanes per matrix run the Jacobi sweeps on R_k and V_k in LDS,
// (3) thread theta adds the chunk's bins to P[theta] in ascending bin order.
__global__ __launch_bounds__(kThreads) void doa_frames_kernel(FrArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* sp = smem;
    auto take = [&](size_t bytes) {
        unsigned char* r = sp;
        sp += (bytes + 15) & ~(size_t)15;
        return r;
    };
    float2* stw = reinterpret_cast<float2*>(take((size_t)a.nfft * sizeof(float2)));
    float* wy = reinterpret_cast<float*>(take((size_t)kMics * a.nfft * sizeof(float)));
    float2* xs = reinterpret_cast<float2*>(take(kMics * kFrKC * sizeof(float2)));
    float2* A = reinterpret_cast<float2*>(take(kFrKC * kFrMat * sizeof(float2)));
    float2* V = reinterpret_cast<float2*>(take(kFrKC * kFrMat * sizeof(float2)));
    float4* prm = reinterpret_cast<float4*>(take(kFrKC * 4 * sizeof(float4)));
    float2* ev = reinterpret_cast<float2*>(take(kFrKC * kMics * sizeof(float2)));
    uint32_t* dmin = reinterpret_cast<uint32_t*>(take(kFrKC * sizeof(uint32_t)));
    float* P = reinterpret_cast<float*>(take(kFrDirs * sizeof(float)));
    float* red = reinterpret_cast<float*>(take(kThreads * sizeof(float)));
    int* redi = reinterpret_cast<int*>(take(kThreads * sizeof(int)));

    const int tid = threadIdx.x;
    const int64_t fr = blockIdx.x;  // g * n_frames + i
    const int64_t g = fr / a.n_frames, i = fr % a.n_frames;
    const int64_t base = g * kMics * a.n + i * (int64_t)a.H;  // channel 0, sample 0 of the frame

    // a frame with a non-finite sample is invalid, and so is one too short
    // for a snapshot
    int nonfinite = 0;
    for (int idx = tid; idx < kMics * a.L; idx += kThreads) {
        const int m = idx / a.L, t = idx % a.L;
        const float v = ld_y(a, base + (int64_t)m * a.n + t);
        if (!(fabsf(v) <= 3.402823466e+38f)) nonfinite = 1;
    }
    const int bad = __syncthreads_or(nonfinite);
    if (bad || a.J < 1) {
        if (tid == 0) {
            a.est[fr] = -1;
            a.valid[fr] = 0;
        }
        if (a.spec)
            for (int th = tid; th < kFrDirs; th += kThreads) a.spec[fr * kFrDirs + th] = 0.f;
        return;
    }

    for (int j = tid; j < a.nfft; j += kThreads) stw[j] = a.tw[j];
    for (int th = tid; th < kFrDirs; th += kThreads) P[th] = 0.f;

    const int dm = tid >> 5, dk = tid & (kFrKC - 1);  // DFT role: mic, bin of the chunk
    const int jm = tid >> 3, jl = tid & 7;            // Jacobi role: matrix, lane
    const float fJ = (float)a.J;

    for (int k0 = 0; k0 < a.K; k0 += kFrKC) {
        const int nk = min(kFrKC, a.K - k0);
        // ---- (1) DFT at the chunk's bins and covariance
        const int bin = a.k_lo + k0 + (dk < nk ? dk : 0);
        float2 r[kMics];
#pragma unroll
        for (int q = 0; q < kMics; ++q) r[q] = make_float2(0.f, 0.f);
        for (int j = 0; j < a.J; ++j) {
            __syncthreads();  // wy, xs free (and A, ev of the chunk before)
            for (int idx = tid; idx < kMics * a.nfft; idx += kThreads) {
                const int m = idx / a.nfft, t = idx % a.nfft;
                wy[idx] = ld_y(a, base + (int64_t)m * a.n + (int64_t)j * a.hop + t) * a.win[t];
            }
            __syncthreads();
            // kFrChains interleaved partial sums (t mod 16: short fp32 chains),
            // added pairwise at the end
            float re[kFrChains], im[kFrChains];
#pragma unroll
            for (int u = 0; u < kFrChains; ++u) re[u] = im[u] = 0.f;
            const float* row = wy + dm * a.nfft;
            int ph = 0;  // (bin * t) mod nfft
            int t = 0;
            for (; t + kFrChains <= a.nfft; t += kFrChains) {
#pragma unroll
                for (int u = 0; u < kFrChains; ++u) {
                    const float2 c = stw[ph];
                    const float v = row[t + u];
                    re[u] = fmaf(v, c.x, re[u]);
                    im[u] = fmaf(v, c.y, im[u]);
                    ph += bin;
                    if (ph >= a.nfft) ph -= a.nfft;
                }
            }
            for (; t < a.nfft; ++t) {  // nfft mod 16 left-over samples
                const float2 c = stw[ph];
                const float v = row[t];
                re[0] = fmaf(v, c.x, re[0]);
                im[0] = fmaf(v, c.y, im[0]);
                ph += bin;
                if (ph >= a.nfft) ph -= a.nfft;
            }
#pragma unroll
            for (int w = kFrChains / 2; w > 0; w >>= 1)
#pragma unroll
                for (int u = 0; u < w; ++u) {
                    re[u] += re[u + w];
                    im[u] += im[u + w];
                }
            float2 x = make_float2(re[0], im[0]);
            if (a.algo == kAlgoSrp) {  // PHAT
                const float mod = fmaxf(hypotf(x.x, x.y), 1e-14f);
                x.x = x.x / mod;
                x.y = x.y / mod;
            }
            xs[dm * kFrKC + dk] = x;
            __syncthreads();
            // R[m][q] += x_m conj(x_q): products first, so R stays exactly Hermitian
#pragma unroll
            for (int q = 0; q < kMics; ++q) {
                const float2 d = cmulc(x, xs[q * kFrKC + dk]);
                r[q].x += d.x;
                r[q].y += d.y;
            }
        }
#pragma unroll
        for (int q = 0; q < kMics; ++q) {
            A[dk * kFrMat + dm * kMics + q] = make_float2(r[q].x / fJ, r[q].y / fJ);
            V[dk * kFrMat + dm * kMics + q] = make_float2(dm == q ? 1.f : 0.f, 0.f);
        }
        __syncthreads();

        if (a.algo != kAlgoSrp) {
            // ---- (2) cyclic Jacobi, round-robin order, a fixed number of sweeps.
            // Pair (p, q), c = A[p][q] = |c| w: J = [[cs, sn w], [-sn conj(w), cs]],
            // A <- J^H A J, V <- V J.
            float2* Am = A + jm * kFrMat;
            float2* Vm = V + jm * kFrMat;
            for (int sweep = 0; sweep < kFrSweeps; ++sweep) {
                for (int rnd = 0; rnd < 7; ++rnd) {
                    if (jl < 4) {
                        int p, q;
                        jacobi_pair(rnd, jl, p, q);
                        const float app = Am[p * kMics + p].x, aqq = Am[q * kMics + q].x;
                        const float2 c = Am[p * kMics + q];
                        const float mag = hypotf(c.x, c.y);
                        float4 pr = make_float4(1.f, 0.f, 0.f, 0.f);
                        if (mag > 1e-30f) {
                            const float tau = (aqq - app) / (2.f * mag);
                            const float tt = copysignf(1.f, tau) / (fabsf(tau) + sqrtf(1.f + tau * tau));
                            const float cs = 1.f / sqrtf(1.f + tt * tt);
                            const float sn = tt * cs;
                            pr = make_float4(cs, sn * (c.x / mag), sn * (c.y / mag), 0.f);
                        }
                        prm[jm * 4 + jl] = pr;
                    }
                    __syncthreads();
                    // columns p, q of row jl of A and V
#pragma unroll
                    for (int pi = 0; pi < 4; ++pi) {
                        int p, q;
                        jacobi_pair(rnd, pi, p, q);
                        const float4 pr = prm[jm * 4 + pi];
                        const float cs = pr.x;
                        const float2 s = make_float2(pr.y, pr.z);
                        const float2 ap = Am[jl * kMics + p], aq = Am[jl * kMics + q];
                        const float2 t1 = cmulc(aq, s), t2 = cmul(ap, s);
                        Am[jl * kMics + p] = make_float2(cs * ap.x - t1.x, cs * ap.y - t1.y);
                        Am[jl * kMics + q] = make_float2(t2.x + cs * aq.x, t2.y + cs * aq.y);
                        const float2 vp = Vm[jl * kMics + p], vq = Vm[jl * kMics + q];
                        const float2 u1 = cmulc(vq, s), u2 = cmul(vp, s);
                        Vm[jl * kMics + p] = make_float2(cs * vp.x - u1.x, cs * vp.y - u1.y);
                        Vm[jl * kMics + q] = make_float2(u2.x + cs * vq.x, u2.y + cs * vq.y);
                    }
                    __syncthreads();
                    // rows p, q of column jl of A
#pragma unroll
                    for (int pi = 0; pi < 4; ++pi) {
                        int p, q;
                        jacobi_pair(rnd, pi, p, q);
                        const float4 pr = prm[jm * 4 + pi];
                        const float cs = pr.x;
                        const float2 s = make_float2(pr.y, pr.z);
                        const float2 ap = Am[p * kMics + jl], aq = Am[q * kMics + jl];
                        const float2 t1 = cmul(s, aq), t2 = cmulc(ap, s);
                        Am[p * kMics + jl] = make_float2(cs * ap.x - t1.x, cs * ap.y - t1.y);
                        Am[q * kMics + jl] = make_float2(t2.x + cs * aq.x, t2.y + cs * aq.y);
                    }
                    __syncthreads();
                }
            }
            // unit eigenvector of the largest eigenvalue (first among equals)
            int best = 0;
            float bv = Am[0].x;
#pragma unroll
            for (int q = 1; q < kMics; ++q) {
                const float v = Am[q * kMics + q].x;
                if (v > bv) {
                    bv = v;
                    best = q;
                }
            }
            float n2 = 0.f;
#pragma unroll
            for (int q = 0; q < kMics; ++q) {
                const float2 e = Vm[q * kMics + best];
                n2 += e.x * e.x + e.y * e.y;
            }
            const float nrm = sqrtf(n2);
            const float2 e = Vm[jl * kMics + best];
            ev[jm * kMics + jl] = nrm > 0.f ? make_float2(e.x / nrm, e.y / nrm) : make_float2(jl == 0 ? 1.f : 0.f, 0.f);
            if (tid < kFrKC) dmin[tid] = 0x7f800000u;  // +inf
            __syncthreads();
        }

        // ---- (3) the chunk's bins into P[theta]
        if (a.algo == kAlgoSrp) {
            for (int th = tid; th < kFrDirs; th += kThreads) {
                float acc = P[th];
                for (int kk = 0; kk < nk; ++kk) {
                    const float2* Ak = A + kk * kFrMat;
                    float2 st[kMics];
#pragma unroll
                    for (int m = 0; m < kMics; ++m)
                        st[m] = a.steer[((int64_t)(k0 + kk) * kMics + m) * kFrDirs + th];
                    // a^H R a = sum_m R_mm + 2 sum_{m < q} Re(conj(a_m) R_mq a_q)
                    float dg = 0.f, off = 0.f;
#pragma unroll
                    for (int m = 0; m < kMics; ++m) {
                        dg += Ak[m * kMics + m].x;
#pragma unroll
                        for (int q = m + 1; q < kMics; ++q) {
                            const float2 z = cmulc(st[q], st[m]);  // a_q conj(a_m)
                            const float2 rr = Ak[m * kMics + q];
                            off += rr.x * z.x - rr.y * z.y;
                        }
                    }
                    acc += dg + 2.f * off;
                }
                P[th] = acc;
            }
        } else {
            // d(theta, k) = max(8 - |e^H a|^2, 8 floor); P_k = 1 / d
            auto dval = [&](int th, int kk) {
                float2 s = make_float2(0.f, 0.f);
#pragma unroll
                for (int m = 0; m < kMics; ++m) {
                    const float2 z = cmulc(a.steer[((int64_t)(k0 + kk) * kMics + m) * kFrDirs + th],
                                           ev[kk * kMics + m]);  // a_m conj(e_m)
                    s.x += z.x;
                    s.y += z.y;
                }
                return fmaxf(8.f - (s.x * s.x + s.y * s.y), a.floor8);
            };
            if (a.algo == kAlgoNormMusic) {
                // max over theta of P_k = 1 / min d: an integer minimum over
                // the bit patterns of positive floats (order-independent)
                for (int th = tid; th < kFrDirs; th += kThreads)
                    for (int kk = 0; kk < nk; ++kk) atomicMin(&dmin[kk], __float_as_uint(dval(th, kk)));
                __syncthreads();
            }
            for (int th = tid; th < kFrDirs; th += kThreads) {
                float acc = P[th];
                for (int kk = 0; kk < nk; ++kk) {
                    float pk = 1.f / dval(th, kk);
                    if (a.algo == kAlgoNormMusic) pk = pk / (1.f / __uint_as_float(dmin[kk]));
                    acc += pk;
                }
                P[th] = acc;
            }
        }
    }
    __syncthreads();

    // ---- mean over the bins, first argmax
    const float fK = (float)a.K;
    float bv = -INFINITY;
    for (int th = tid; th < kFrDirs; th += kThreads) {
        const float v = P[th] / fK;
        if (a.spec) a.spec[fr * kFrDirs + th] = v;
        P[th] = v;
        bv = fmaxf(bv, v);
    }
    const float mx = block_max<kThreads>(bv, red);
    int first = 0x7fffffff;
    for (int th = tid; th < kFrDirs; th += kThreads)
        if (P[th] == mx) {
            first = th;
            break;
        }
    const int idx = block_min<kThreads>(first, redi);
    if (tid == 0) {
        a.est[fr] = idx < kFrDirs ? idx : 0;
        a.valid[fr] = 1;
    }
}

int frames_shape(int64_t G, int64_t n, int32_t L, int32_t H, int64_t n_frames, int32_t nfft, int32_t hop,
                 int32_t k_lo, int32_t K, int32_t algo, float floor) {
    AVR_REQUIRE(G >= 1 && n >= 1 && L >= 1 && H >= 1, "avr_doa_frames: G, n, L and H must be positive");
    AVR_REQUIRE(n_frames >= 1 && L <= n && (n_frames - 1) * (int64_t)H + L <= n,
                "avr_doa_frames: frames must lie inside the signal ((n_frames - 1) H + L <= n)");
    AVR_REQUIRE(G * n_frames <= 0x7fffffffLL, "avr_doa_frames: G * n_frames must be below 2^31");
    AVR_REQUIRE(G * kMics <= ((int64_t)1 << 62) / n, "avr_doa_frames: signal too large");
    AVR_REQUIRE(nfft >= 2 && nfft <= kFrMaxNfft, "avr_doa_frames: nfft must be in [2, 2048]");
    AVR_REQUIRE(hop >= 1, "avr_doa_frames: hop must be positive");
    AVR_REQUIRE(k_lo >= 0 && K >= 1 && k_lo + (int64_t)K <= nfft / 2 + 1,
                "avr_doa_frames: bins must lie in [0, nfft / 2]");
    AVR_REQUIRE(algo >= kAlgoSrp && algo <= kAlgoNormMusic, "avr_doa_frames: unknown algorithm");
    AVR_REQUIRE(floor > 0.f && floor <= 1.f, "avr_doa_frames: floor must be in (0, 1]");
    return 0;
}

// ------------------------------------------------------------ statistics
// sqrt(c^2 + s^2) rounded once: the squares and their sum are kept as
// double-double, the square root is corrected by its exact residual.  (For a
// single angle R must come out as 1.0 where libm's hypot gives 1.0: the
// circular standard deviation sqrt(-2 log R) turns one ulp of R into 8.5e-7
// degrees.)
__device__ double hypot_once(double c, double s) {
    const double p = c * c, pe = fma(c, c, -p);
    const double q = s * s, qe = fma(s, s, -q);
    const double sh = p + q;
    if (!(sh > 0.0)) return 0.0;
    const double bb = sh - p;
    const double se = ((p - (sh - bb)) + (q - bb)) + (pe + qe);
    const double h = sqrt(sh);
    return h + (fma(-h, h, sh) + se) / (2.0 * h);
}

// circ_stats_deg over the valid frames of a group (fp64; fixed order: a
// thread's frames in ascending order, then a tree over the 256 threads).
// cs[d] = (cos, sin)(deg2rad(d)), d = 0..359, is a host table (numpy's own
// values, the reference's); an angle is taken modulo 360.
__global__ __launch_bounds__(kThreads) void doa_frame_stats_kernel(
    int64_t n_frames, const int32_t* __restrict__ est, const uint8_t* __restrict__ valid,
    const double2* __restrict__ cs, int64_t G, double* __restrict__ out, int64_t* __restrict__ n_valid) {
    __shared__ double red[kThreads];
    const int64_t g = blockIdx.x;
    const double kPi = 3.14159265358979323846;
    double c = 0.0, s = 0.0, cnt = 0.0;
    for (int64_t i = threadIdx.x; i < n_frames; i += kThreads) {
        if (!valid[g * n_frames + i]) continue;
        int d = est[g * n_frames + i] % 360;
        if (d < 0) d += 360;
        const double2 v = cs[d];
        c += v.x;
        s += v.y;
        cnt += 1.0;
    }
    const double C = block_sum<kThreads>(c, red), S = block_sum<kThreads>(s, red);
    const double N = block_sum<kThreads>(cnt, red);
    if (threadIdx.x == 0) {
        n_valid[g] = (int64_t)N;
        double mu = NAN, var = NAN, sd = NAN;
        if (N > 0.0) {
            mu = fmod(atan2(S, C) * (180.0 / kPi) + 360.0, 360.0);
            const double R = hypot_once(C, S) / N;
            var = 1.0 - R;
            sd = R > 0.0 ? sqrt(fmax(0.0, -2.0 * log(fmax(R, 1e-12)))) * (180.0 / kPi) : NAN;
        }
        out[0 * G + g] = mu;
        out[1 * G + g] = var;
        out[2 * G + g] = sd;
    }
}

}  // namespace

extern "C" int avr_doa_das_workspace(int64_t G, int32_t nfft, int32_t K, int64_t* bytes) {
    if (int e = das_doa_shape(G, 1, nfft, K)) return e;
    AVR_REQUIRE(bytes, "avr_doa_das_workspace: null bytes");
    *bytes = das_carve(nullptr, G, nfft / 2 + 1, K).bytes;
    return 0;
}

extern "C" int avr_doa_das(int64_t G, int32_t n, int32_t nfft, int32_t K, const float* pred_ir,
                           const float* ori_ir, const float* steer, const float* angles,
                           const double* tw, double beta, const void* position_rx,
                           const void* position_tx, int32_t pos_dtype, double* out, void* workspace,
                           int64_t workspace_bytes, void* stream) {
    if (int e = das_doa_shape(G, n, nfft, K)) return e;
    AVR_REQUIRE(pred_ir && ori_ir && steer && angles && tw && position_rx && position_tx && out && workspace,
                "avr_doa_das: null pointer");
    AVR_REQUIRE(pos_dtype == AVR_DTYPE_F32 || pos_dtype == AVR_DTYPE_F64,
                "avr_doa_das: positions must be fp32 or fp64");
    AVR_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "avr_doa_das: workspace must be 16-byte aligned");
    const int F = nfft / 2 + 1;
    const int tiles = (F + kDasFTile - 1) / kDasFTile;
    const DasDoaWs W = das_carve(workspace, G, F, K);
    AVR_REQUIRE(workspace_bytes >= W.bytes, "avr_doa_das: workspace too small");
    hipStream_t st = as_stream(stream);
    if (int e = launch("doa_das_spectrum_kernel", doa_das_spectrum_kernel, dim3((unsigned)(G * kMics), 2),
                       dim3(kThreads), (size_t)nfft * (sizeof(double2) + sizeof(float)), st, (int)n, (int)nfft, F,
                       pred_ir, ori_ir, reinterpret_cast<const double2*>(tw), W.X))
        return e;
    const size_t plds = kMics * kDasFTile * sizeof(double2) + kDasFTile * sizeof(double) +
                        (size_t)K * (kDasFTile + 1) * sizeof(double);
    if (int e = launch("doa_das_power_kernel", doa_das_power_kernel, dim3((unsigned)tiles, (unsigned)(2 * G)),
                       dim3(kThreads), plds, st, F, (int)K, reinterpret_cast<const float2*>(steer),
                       (const double2*)W.X, W.ppart))
        return e;
    const size_t flds = (size_t)(kThreads + K + (K & 1)) * sizeof(double) + kThreads * sizeof(int);
    return launch("doa_das_finish_kernel", doa_das_finish_kernel, dim3((unsigned)G), dim3(kThreads), flds, st, G,
                  tiles, (int)K, angles, beta, (const double*)W.ppart, position_rx, position_tx,
                  (int)(pos_dtype == AVR_DTYPE_F64), out);
}

extern "C" int avr_doa_frames(int64_t G, int64_t n, int32_t L, int32_t H, int64_t n_frames, int32_t nfft,
                              int32_t hop, int32_t k_lo, int32_t K, int32_t algo, float floor, const void* y,
                              int32_t y_dtype, const float* tw, const float* win, const float* steer,
                              int32_t* est, uint8_t* valid, float* spectrum, void* stream) {
    if (int e = frames_shape(G, n, L, H, n_frames, nfft, hop, k_lo, K, algo, floor)) return e;
    AVR_REQUIRE(y_dtype == AVR_DTYPE_F32 || y_dtype == AVR_DTYPE_F64, "avr_doa_frames: y must be fp32 or fp64");
    AVR_REQUIRE(y && tw && win && steer && est && valid, "avr_doa_frames: null pointer");
    FrArgs a{};
    a.y = y;
    a.y_f64 = y_dtype == AVR_DTYPE_F64;
    a.n = n;
    a.n_frames = n_frames;
    a.L = L;
    a.H = H;
    a.nfft = nfft;
    a.hop = hop;
    a.J = L >= nfft ? (L - nfft) / hop + 1 : 0;
    a.k_lo = k_lo;
    a.K = K;
    a.algo = algo;
    a.floor8 = 8.f * floor;
    a.tw = reinterpret_cast<const float2*>(tw);
    a.win = win;
    a.steer = reinterpret_cast<const float2*>(steer);
    a.est = est;
    a.valid = valid;
    a.spec = spectrum;
    return launch("doa_frames_kernel", doa_frames_kernel, dim3((unsigned)(G * n_frames)), dim3(kThreads),
                  frames_lds(nfft), as_stream(stream), a);
}

extern "C" int avr_doa_frame_stats(int64_t G, int64_t n_frames, const int32_t* est, const uint8_t* valid,
                                   const double* cos_sin, double* out, int64_t* n_valid, void* stream) {
    AVR_REQUIRE(G >= 1 && G <= 0x7fffffffLL && n_frames >= 0, "avr_doa_frame_stats: G >= 1 and n_frames >= 0 required");
    AVR_REQUIRE(out && n_valid && cos_sin && (n_frames == 0 || (est && valid)),
                "avr_doa_frame_stats: null pointer");
    return launch("doa_frame_stats_kernel", doa_frame_stats_kernel, dim3((unsigned)G), dim3(kThreads), 0,
                  as_stream(stream), n_frames, est, valid, reinterpret_cast<const double2*>(cos_sin), G, out, n_valid);
}
