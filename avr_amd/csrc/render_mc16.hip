// Binaural rendering for MI355X (gfx950): the ray reduction of up to 16
// receiver channels in one pass over the signal on the fp32 MFMA, and the
// per-bin complex decode of an ambisonic spectrum with its adjoint.
// DESIGN.md section 25.
#include "common.h"
#include "ray_stream.h"

using namespace avr;

namespace {

// part[k][b*C + c][s][t] = sum_{r in split k} fl(w[b,r,s]*g[b,c,r]) * [live] * x[b,r,s,t]
// for every c < C at once: ray_reduce_mc_fwd_kernel's sums as the product
// [16 channels x rays] x [rays x t] on v_mfma_f32_16x16x4_f32, whose result
// is a k-ordered fmaf chain; rays enter in ascending order, so a channel's
// element is the vector kernel's fmaf chain term for term.  The mask is
// applied to x (select, not multiply) where the vector kernel applies it to
// the weight: the products are the same for finite x.
//
// Lane l = (n = l & 15, q = l >> 4).  A wave owns a strip of 16 chunks of 16
// bytes; lane (n, q) loads chunk n of ray 4i + q of r-group i.
//   A = wg[c = n][ray 4i + q]       from the LDS slab, ray-major (a wave's
//                                   read is 256 contiguous bytes), rows >= C 0
//   B = element j of the chunk      into accumulator j (VEC of them)
//   D = acc[j][reg]: channel 4q + reg at the t of element j of chunk n
// The rays of a split are padded to whole batches with delay INT_MAX and zero
// products.  LDS: d_l[ld], then wg_l[ld][16].
//
// The B registers are rewritten every batch: all MFMAs of a batch issue,
// then mfma_queue_wait(), and the operands are held across it (DESIGN.md
// section 15a).
template <typename Tin>
__global__ __launch_bounds__(64 * kMc16Waves) void ray_reduce_mc16_fwd_kernel(
    avr_render_params pp, const Tin* __restrict__ sig, const float* __restrict__ w,
    const int32_t* __restrict__ delay, const float* __restrict__ gain, int64_t gain_b_stride, int C,
    float* __restrict__ part, int B, int R, int S, int T, int rays_per_split, int ld) {
    constexpr int VEC = Vec16<Tin>::N;
    constexpr int U = kMc16Batch<VEC>;
    extern __shared__ float lds_mc16[];
    const int split = blockIdx.x, s = blockIdx.y, b = blockIdx.z;
    const int r0 = split * rays_per_split;
    const int nr = max(0, min(R, r0 + rays_per_split) - r0);
    const int nrp = (nr + 4 * U - 1) / (4 * U) * (4 * U);  // <= ld
    int* d_l = reinterpret_cast<int*>(lds_mc16);
    float* wg_l = lds_mc16 + ld;
    const float* gb = gain + (int64_t)b * gain_b_stride + r0;
    for (int i = threadIdx.x; i < nrp; i += blockDim.x)
        d_l[i] = i < nr ? delay[((int64_t)b * R + r0 + i) * S + s] : 0x7fffffff;
    for (int i = threadIdx.x; i < nrp * kMaxChannels; i += blockDim.x) {
        const int c = i / nrp, rr = i - c * nrp;
        float v = 0.0f;
        if (c < C && rr < nr) v = w[((int64_t)b * R + r0 + rr) * S + s] * gb[(int64_t)c * R + rr];
        wg_l[rr * kMaxChannels + c] = v;
    }
    __syncthreads();

    const int64_t row0 = (((int64_t)b * R + r0) * S + s) * (int64_t)T;
    const int phase = (int)(row0 % VEC);
    const int nchunks = (T + phase + VEC - 1) / VEC;
    const int64_t row_stride = (int64_t)S * T;
    const int lim = tail_limit(pp, s);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    const int n = lane & 15, q = lane >> 4;
    // byte offset of this lane's ray within an r-group's four rows, and the
    // bytes four rows span up to the end of the last one's chunks
    const uint32_t qoff = (uint32_t)q * (uint32_t)(row_stride * (int64_t)sizeof(Tin));
    const uint32_t span = 3u * (uint32_t)(row_stride * (int64_t)sizeof(Tin)) + (uint32_t)nchunks * 16u;
    float* pout = part + ((((int64_t)split * B + b) * C) * S + s) * (int64_t)T;

    for (int strip = wave; strip * 16 < nchunks; strip += nwaves) {
        const int j = strip * 16 + n;  // this lane's chunk
        int tk[VEC], tm[VEC], tmax = -1;
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const int e = j * VEC + k - phase;
            tk[k] = (e >= 0 && e < T) ? e : -1;
            tm[k] = tk[k] < lim ? tk[k] : -1;
            tmax = max(tmax, tm[k]);
        }
        if (j >= nchunks) tmax = -1;
        f32x4 acc[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[k] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

        for (int g0 = 0; g0 * 4 < nrp; g0 += U) {
            int d[U];
            bool need[U], any = false;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                d[u] = d_l[4 * (g0 + u) + q];
                need[u] = tmax >= d[u];  // padded rays: never
                any |= need[u];
            }
            // a batch that is dead for the whole wave adds only zeros
            if (!__any(any)) continue;
            float a[U], x[U][VEC];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                a[u] = wg_l[(4 * (g0 + u) + q) * kMaxChannels + n];
                // the r-group's first row is wave-uniform; a lane that needs
                // its chunk lies inside the tensor (rr < nr, j < nchunks),
                // every other lane reads zeros without touching memory
                const Tin* rowg = sig + (row0 - phase + (int64_t)(4 * (g0 + u)) * row_stride);
                load16_masked(rowg, span, need[u] ? qoff + (uint32_t)j * 16u : kSkip, x[u]);
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int k = 0; k < VEC; ++k) x[u][k] = tm[k] >= d[u] ? x[u][k] : 0.0f;
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int k = 0; k < VEC; ++k)
                    acc[k] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], x[u][k], acc[k], 0, 0, 0);
            mfma_queue_wait();
#pragma unroll
            for (int u = 0; u < U; ++u) {
                keep_live(a[u]);
#pragma unroll
                for (int k = 0; k < VEC; ++k) keep_live(x[u][k]);
            }
        }
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int c = 4 * q + reg;
            if (c < C) {
                float* pc = pout + (int64_t)c * S * T;
#pragma unroll
                for (int k = 0; k < VEC; ++k)
                    if (tk[k] >= 0 && j < nchunks) pc[tk[k]] = acc[k][reg];
            }
        }
    }
}

// out[b,e,f] = sum_k dec[e,k,f] * amb[b,k,f]: one thread per (b, e, f)
__global__ __launch_bounds__(256) void sh_decode_fwd_kernel(int B, int E, int K, int F,
                                                             const float2* __restrict__ dec,
                                                             const float2* __restrict__ amb,
                                                             float2* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)B * E * F) return;
    const int f = (int)(i % F), e = (int)(i / F % E), b = (int)(i / F / E);
    float re = 0.0f, im = 0.0f;
    for (int k = 0; k < K; ++k) {
        const float2 d = dec[((int64_t)e * K + k) * F + f], a = amb[((int64_t)b * K + k) * F + f];
        re = fmaf(-d.y, a.y, fmaf(d.x, a.x, re));
        im = fmaf(d.y, a.x, fmaf(d.x, a.y, im));
    }
    out[i] = make_float2(re, im);
}

// grad_amb[b,k,f] = sum_e conj(dec[e,k,f]) * grad_out[b,e,f]: one thread per (b, k, f)
__global__ __launch_bounds__(256) void sh_decode_bwd_kernel(int B, int E, int K, int F,
                                                             const float2* __restrict__ dec,
                                                             const float2* __restrict__ go,
                                                             float2* __restrict__ ga) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)B * K * F) return;
    const int f = (int)(i % F), k = (int)(i / F % K), b = (int)(i / F / K);
    float re = 0.0f, im = 0.0f;
    for (int e = 0; e < E; ++e) {
        const float2 d = dec[((int64_t)e * K + k) * F + f], g = go[((int64_t)b * E + e) * F + f];
        re = fmaf(d.y, g.y, fmaf(d.x, g.x, re));
        im = fmaf(-d.y, g.x, fmaf(d.x, g.y, im));
    }
    ga[i] = make_float2(re, im);
}

int sh_decode_args(const char* what, int B, int E, int K, int F, const void* a, const void* b, const void* c,
                   int64_t threads) {
    if (!(B >= 1 && E >= 1 && F >= 1 && a && b && c)) return fail(AVR_E_ARG, std::string(what) + ": bad args");
    if (!(K >= 1 && K <= kMaxChannels)) return fail(AVR_E_ARG, std::string(what) + ": K must be 1..16");
    if ((threads + 255) / 256 > 0x7fffffffLL) return fail(AVR_E_ARG, std::string(what) + ": too many elements");
    return 0;
}

}  // namespace

extern "C" int32_t avr_reduce_mc16_max_rays(void) { return mc16_max_rays(); }

extern "C" int avr_ray_reduce_mc16_fwd(const avr_render_params* p, int32_t B, int32_t C, const void* signal,
                                       int32_t sig_dtype, const float* w, const int32_t* delay,
                                       const float* gain, int64_t gain_b_stride, int32_t n_split, float* part,
                                       void* stream) {
    if (int e = validate_render_params(p)) return e;
    AVR_REQUIRE(B >= 1 && signal && w && delay && gain && part, "avr_ray_reduce_mc16_fwd: null pointer");
    AVR_REQUIRE(C >= 1 && C <= kMaxChannels, "avr_ray_reduce_mc16_fwd: C must be 1..16");
    const int R = n_rays(*p), S = p->n_samples, T = p->T;
    AVR_REQUIRE(gain_b_stride == 0 || gain_b_stride == (int64_t)C * R,
                "avr_ray_reduce_mc16_fwd: gain_b_stride must be 0 ([C,R]) or C*R ([B,C,R])");
    AVR_REQUIRE(n_split >= 1 && n_split <= R, "avr_ray_reduce_mc16_fwd: n_split out of range");
    const int rps = (R + n_split - 1) / n_split;
    AVR_REQUIRE(rps <= mc16_max_rays(), "avr_ray_reduce_mc16_fwd: too many rays per split (raise n_split)");
    const int64_t row = (int64_t)S * T;
    return dispatch_dtype<AVR_DTYPE_F32, AVR_DTYPE_F16, AVR_DTYPE_BF16>(
        sig_dtype, "avr_ray_reduce_mc16_fwd", [&](auto tag) {
            using Tin = typename decltype(tag)::type;
            constexpr int VEC = Vec16<Tin>::N;
            if (!vector_ok<Tin>(row, signal))
                return fail(AVR_E_CONFIG, "avr_ray_reduce_mc16_fwd: needs the 16-byte form (signal 16-byte "
                                          "aligned, S*T a multiple of the vector)");
            // a lane addresses the four rows of an r-group with a 32-bit byte offset
            // (the masked lanes' kSkip must stay past the four rows' span)
            if (4 * row * (int64_t)sizeof(Tin) >= 0x7fff0000LL)
                return fail(AVR_E_CONFIG, "avr_ray_reduce_mc16_fwd: S*T too large for this build");
            const int nstrips = ((T + VEC - 1 + VEC - 1) / VEC + 15) / 16;  // at the largest phase
            const int ld = mc16_padded(rps);
            const dim3 grid(n_split, S, B), block(64 * min(kMc16Waves, nstrips));
            return launch("avr_ray_reduce_mc16_fwd", ray_reduce_mc16_fwd_kernel<Tin>, grid, block,
                          (size_t)ld * kMc16RayBytes, as_stream(stream), *p, (const Tin*)signal, w, delay, gain,
                          (int64_t)gain_b_stride, (int)C, part, (int)B, R, S, T, rps, ld);
        });
}

extern "C" int avr_sh_decode_fwd(int32_t B, int32_t E, int32_t K, int32_t F, const float* dec, const float* amb,
                                 float* out, void* stream) {
    const int64_t n = (int64_t)B * E * F;
    if (int e = sh_decode_args("avr_sh_decode_fwd", B, E, K, F, dec, amb, out, n)) return e;
    return launch("avr_sh_decode_fwd", sh_decode_fwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                  as_stream(stream), (int)B, (int)E, (int)K, (int)F, reinterpret_cast<const float2*>(dec),
                  reinterpret_cast<const float2*>(amb), reinterpret_cast<float2*>(out));
}

extern "C" int avr_sh_decode_bwd(int32_t B, int32_t E, int32_t K, int32_t F, const float* dec,
                                 const float* grad_out, float* grad_amb, void* stream) {
    const int64_t n = (int64_t)B * K * F;
    if (int e = sh_decode_args("avr_sh_decode_bwd", B, E, K, F, dec, grad_out, grad_amb, n)) return e;
    return launch("avr_sh_decode_bwd", sh_decode_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                  as_stream(stream), (int)B, (int)E, (int)K, (int)F, reinterpret_cast<const float2*>(dec),
                  reinterpret_cast<const float2*>(grad_out), reinterpret_cast<float2*>(grad_amb));
}
