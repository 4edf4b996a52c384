// Per-pose bias + ReLU of the channel-embedding ("add" / injection) networks
// (model.py:55-61 of the reference: h = layer(x) + emb[ch]; x = relu(h)).
//
//   out[r][:] = round_T(relu(float(y[r][:]) + table[idx[r / rows_per_group]][:]))   (forward)
//   g[r][:]   = out[r][:] <= 0 ? 0 : gy[r][:]                                        (backward)
//   g_table[c][:] = sum over groups with idx == c of the group's rows of g          (backward)
//
// y is the layer's output in the MLP dtype T (tcnn's 16-bit output, or fp32),
// table the fp32 [C, W] embedding, idx one int64 channel per group (pose) of
// rows_per_group consecutive rows.  The sum and the ReLU run in fp32 and the
// result is rounded to T once, the promotion order of the reference's torch
// ops.  ReLU is torch's: NaN stays NaN, +inf stays.  A group whose index is
// outside [0, C) reads nothing from the table: its rows become NaN, and it
// adds nothing to g_table.
//
// One 16-byte vector per lane and row (8 x 16-bit or 4 x fp32); element
// offsets are 64-bit (N * W passes 2^31 at the reference's batch 16).
//
// The table gradient has no atomics: the backward pass, which writes g, also
// writes the fp32 column sums of each chunk of kChunk rows of a group into a
// workspace [G * chunks_per_group][W]; a second launch sums, for every
// channel, the chunks of its groups (groups ascending, chunks ascending) and
// stores each g_table element once.  The result is the same bits every run.
#include "common.h"

using namespace avr;

namespace {

constexpr int kThreads = 256;
constexpr int kFwdIters = 8;   // rows per lane of the forward (loads in flight)
constexpr int kBwdIters = 4;   // rows per lane and round of the backward
constexpr int kChunk = 512;    // rows per column-partial of the backward
constexpr int kSumCols = 16;   // table_sum_kernel: columns x lanes = kThreads
constexpr int kSumLanes = 16;

// A block is (row lanes) x (column units of 16 bytes): cw = 2^cw_log2 <= 64
// units side by side, 256 / cw rows at a time; blockIdx.y walks the column
// slabs of rows wider than cw units.
struct Tile {
    int upr;      // 16-byte units per row
    int cw_log2;
    int slabs;
};

Tile tile_of(int W, int vec) {
    Tile t;
    t.upr = W / vec;
    t.cw_log2 = 0;
    while ((1 << t.cw_log2) < t.upr && t.cw_log2 < 6) ++t.cw_log2;
    t.slabs = (t.upr + (1 << t.cw_log2) - 1) >> t.cw_log2;
    return t;
}

template <typename T>
__global__ __launch_bounds__(kThreads) void bias_relu_fwd_kernel(uint32_t N, int W, uint32_t rpg, int C, int upr,
                                                                 int cw_log2, const T* __restrict__ y,
                                                                 const float* __restrict__ table,
                                                                 const int64_t* __restrict__ idx,
                                                                 T* __restrict__ out) {
    using V = Vec16<T>;
    const int cw = 1 << cw_log2, rl = kThreads >> cw_log2;
    const int c = (int)blockIdx.y * cw + ((int)threadIdx.x & (cw - 1));
    const bool col_ok = c < upr;
    const int64_t col = (int64_t)(col_ok ? c : 0) * V::N;
    const uint32_t row0 = blockIdx.x * (uint32_t)(rl * kFwdIters) + (threadIdx.x >> cw_log2);
    // every load of the lane first (clamped rows: no load behind a branch)
    typename V::raw v[kFwdIters];
#pragma unroll
    for (int it = 0; it < kFwdIters; ++it) {
        const uint32_t row = min(row0 + (uint32_t)(it * rl), N - 1u);
        v[it] = *reinterpret_cast<const typename V::raw*>(y + (int64_t)row * W + col);
    }
#pragma unroll
    for (int it = 0; it < kFwdIters; ++it) {
        const uint32_t row = row0 + (uint32_t)(it * rl);
        if (row >= N || !col_ok) continue;
        const int64_t ch = idx[row / rpg];
        float f[V::N];
        V::cvt(v[it], f);
        if (ch >= 0 && ch < (int64_t)C) {
            const float* e = table + ch * W + col;
#pragma unroll
            for (int k = 0; k < V::N; k += 4) {
                const f32x4 t = *reinterpret_cast<const f32x4*>(e + k);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float s = f[k + i] + t[i];
                    f[k + i] = s <= 0.0f ? 0.0f : s;  // NaN <= 0 is false: NaN stays
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < V::N; ++k) f[k] = __builtin_nanf("");
        }
        store16(out + (int64_t)row * W + col, f);
    }
}

// blockIdx.x = group * cpg + chunk: rows [chunk * kChunk, +kChunk) of the group
template <typename T>
__global__ __launch_bounds__(kThreads) void bias_relu_bwd_kernel(int W, uint32_t rpg, uint32_t cpg, int upr,
                                                                 int cw_log2, const T* __restrict__ gy,
                                                                 const T* __restrict__ out, T* __restrict__ g,
                                                                 float* __restrict__ ws) {
    using V = Vec16<T>;
    __shared__ float part[kThreads * V::N];  // [row lane][cw * V::N]
    const int cw = 1 << cw_log2, rl = kThreads >> cw_log2;
    const int cu = (int)threadIdx.x & (cw - 1), r_in = (int)(threadIdx.x >> cw_log2);
    const int c = (int)blockIdx.y * cw + cu;
    const bool col_ok = c < upr;
    const uint32_t grp = blockIdx.x / cpg, chunk = blockIdx.x - grp * cpg;
    const uint32_t first = chunk * (uint32_t)kChunk;
    const uint32_t rows = min((uint32_t)kChunk, rpg - first);
    const int64_t base = ((int64_t)grp * rpg + first) * W + (int64_t)(col_ok ? c : 0) * V::N;
    float acc[V::N];
#pragma unroll
    for (int k = 0; k < V::N; ++k) acc[k] = 0.0f;
    // lane r_in sums rows r_in, r_in + rl, ... of the chunk in that order
    for (uint32_t i0 = 0; i0 < rows; i0 += (uint32_t)(kBwdIters * rl)) {
        typename V::raw a[kBwdIters], b[kBwdIters];
#pragma unroll
        for (int u = 0; u < kBwdIters; ++u) {
            const int64_t off = base + (int64_t)min(i0 + (uint32_t)(u * rl + r_in), rows - 1u) * W;
            a[u] = *reinterpret_cast<const typename V::raw*>(gy + off);
            b[u] = *reinterpret_cast<const typename V::raw*>(out + off);
        }
#pragma unroll
        for (int u = 0; u < kBwdIters; ++u) {
            const uint32_t i = i0 + (uint32_t)(u * rl + r_in);
            if (i >= rows || !col_ok) continue;
            float fa[V::N], fb[V::N];
            V::cvt(a[u], fa);
            V::cvt(b[u], fb);
#pragma unroll
            for (int k = 0; k < V::N; ++k) {
                fa[k] = fb[k] <= 0.0f ? 0.0f : fa[k];  // threshold_backward(gy, out, 0)
                acc[k] += fa[k];
            }
            store16(g + base + (int64_t)i * W, fa);
        }
    }
    const int slab_w = cw * V::N;
#pragma unroll
    for (int k = 0; k < V::N; ++k) part[r_in * slab_w + cu * V::N + k] = acc[k];
    __syncthreads();
    for (int e = (int)threadIdx.x; e < slab_w; e += kThreads) {
        float s = 0.0f;
        for (int r = 0; r < rl; ++r) s += part[r * slab_w + e];
        const int column = (int)blockIdx.y * slab_w + e;
        if (column < W) ws[(int64_t)blockIdx.x * W + column] = s;
    }
}

// g_table[c][col] = the chunk partials of the groups with idx == c.  Lane p
// of kSumLanes takes the p-th contiguous share of the (group, chunk) list in
// ascending order; the lanes are then added in ascending order.
__global__ __launch_bounds__(kThreads) void table_sum_kernel(int W, uint32_t G, uint32_t cpg,
                                                             const int64_t* __restrict__ idx,
                                                             const float* __restrict__ ws,
                                                             float* __restrict__ g_table) {
    __shared__ float part[kSumLanes][kSumCols];
    const int lc = (int)threadIdx.x % kSumCols, p = (int)threadIdx.x / kSumCols;
    const int col = (int)blockIdx.x * kSumCols + lc;
    const int64_t c = blockIdx.y;
    const uint64_t total = (uint64_t)G * cpg;
    uint64_t t = total * (uint64_t)p / kSumLanes;
    const uint64_t t1 = total * (uint64_t)(p + 1) / kSumLanes;
    float acc = 0.0f;
    if (col < W && t < t1) {
        uint32_t grp = (uint32_t)(t / cpg);
        while (t < t1) {
            const uint64_t gend = min(t1, (uint64_t)(grp + 1) * cpg);
            if (idx[grp] == c) {
#pragma unroll 4
                for (uint64_t q = t; q < gend; ++q) acc += ws[q * (uint64_t)W + col];
            }
            t = gend;
            ++grp;
        }
    }
    part[p][lc] = acc;
    __syncthreads();
    if (p == 0 && col < W) {
        float s = 0.0f;
        for (int q = 0; q < kSumLanes; ++q) s += part[q][lc];
        g_table[c * W + col] = s;
    }
}

bool dtype_ok(int d) { return d == AVR_DTYPE_F32 || d == AVR_DTYPE_F16 || d == AVR_DTYPE_BF16; }
bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

// the shape every entry point accepts; nullptr when it does, else what is wrong
const char* shape_error(int64_t N, int32_t W, int64_t rpg) {
    if (N <= 0 || N >= (int64_t(1) << 31)) return "N must be in [1, 2^31)";
    if (rpg <= 0 || N % rpg != 0) return "rows_per_group must divide N";
    if (W % 8 != 0 || W < 8 || W > 1024) return "W must be a multiple of 8 in [8, 1024]";
    return nullptr;
}

int64_t chunks_per_group(int64_t rpg) { return (rpg + kChunk - 1) / kChunk; }

int64_t bytes_needed(int64_t N, int32_t W, int64_t rpg) {
    return (N / rpg) * chunks_per_group(rpg) * W * (int64_t)sizeof(float);
}

}  // namespace

extern "C" int avr_group_bias_relu_fwd(int64_t N, int32_t W, int64_t rows_per_group, int32_t C, const void* y,
                                       int32_t dtype, const float* table, const int64_t* idx, void* out,
                                       void* stream) {
    AVR_REQUIRE(y && table && idx && out, "avr_group_bias_relu_fwd: null pointer");
    if (const char* e = shape_error(N, W, rows_per_group))
        return fail(AVR_E_ARG, std::string("avr_group_bias_relu_fwd: ") + e);
    AVR_REQUIRE(C > 0 && C <= 65535, "avr_group_bias_relu_fwd: C must be in [1, 65535]");
    AVR_REQUIRE(dtype_ok(dtype), "avr_group_bias_relu_fwd: unknown dtype");
    AVR_REQUIRE(aligned16(y) && aligned16(table) && aligned16(out),
                "avr_group_bias_relu_fwd: y, table and out must be 16-byte aligned");
    return dispatch_dtype<AVR_DTYPE_F32, AVR_DTYPE_F16, AVR_DTYPE_BF16>(
        dtype, "avr_group_bias_relu_fwd", [&](auto tag) {
            using T = typename decltype(tag)::type;
            const Tile t = tile_of(W, Vec16<T>::N);
            const int rows = (kThreads >> t.cw_log2) * kFwdIters;
            return launch("avr_group_bias_relu_fwd", bias_relu_fwd_kernel<T>,
                          dim3((unsigned)((N + rows - 1) / rows), (unsigned)t.slabs), dim3(kThreads), 0,
                          as_stream(stream), (uint32_t)N, W, (uint32_t)rows_per_group, C, t.upr, t.cw_log2,
                          static_cast<const T*>(y), table, idx, static_cast<T*>(out));
        });
}

extern "C" int avr_group_bias_relu_workspace(int64_t N, int32_t W, int64_t rows_per_group, int64_t* bytes) {
    AVR_REQUIRE(bytes != nullptr, "avr_group_bias_relu_workspace: null pointer");
    if (const char* e = shape_error(N, W, rows_per_group))
        return fail(AVR_E_ARG, std::string("avr_group_bias_relu_workspace: ") + e);
    *bytes = bytes_needed(N, W, rows_per_group);
    return 0;
}

extern "C" int avr_group_bias_relu_bwd(int64_t N, int32_t W, int64_t rows_per_group, int32_t C, const void* gy,
                                       const void* out, int32_t dtype, const int64_t* idx, void* g,
                                       void* workspace, int64_t workspace_bytes, float* g_table, void* stream) {
    AVR_REQUIRE(gy && out && idx && g && workspace && g_table, "avr_group_bias_relu_bwd: null pointer");
    if (const char* e = shape_error(N, W, rows_per_group))
        return fail(AVR_E_ARG, std::string("avr_group_bias_relu_bwd: ") + e);
    AVR_REQUIRE(C > 0 && C <= 65535, "avr_group_bias_relu_bwd: C must be in [1, 65535]");
    AVR_REQUIRE(dtype_ok(dtype), "avr_group_bias_relu_bwd: unknown dtype");
    AVR_REQUIRE(workspace_bytes >= bytes_needed(N, W, rows_per_group),
                "avr_group_bias_relu_bwd: workspace too small (avr_group_bias_relu_workspace)");
    AVR_REQUIRE(aligned16(gy) && aligned16(out) && aligned16(g),
                "avr_group_bias_relu_bwd: gy, out and g must be 16-byte aligned");
    AVR_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 4 == 0 && reinterpret_cast<uintptr_t>(g_table) % 4 == 0,
                "avr_group_bias_relu_bwd: workspace and g_table must be 4-byte aligned");
    hipStream_t st = as_stream(stream);
    float* ws = static_cast<float*>(workspace);
    const int64_t G = N / rows_per_group, cpg = chunks_per_group(rows_per_group);
    const char* what = "avr_group_bias_relu_bwd";
    if (int e = dispatch_dtype<AVR_DTYPE_F32, AVR_DTYPE_F16, AVR_DTYPE_BF16>(dtype, what, [&](auto tag) {
            using T = typename decltype(tag)::type;
            const Tile t = tile_of(W, Vec16<T>::N);
            return launch(what, bias_relu_bwd_kernel<T>, dim3((unsigned)(G * cpg), (unsigned)t.slabs), dim3(kThreads),
                          0, st, W, (uint32_t)rows_per_group, (uint32_t)cpg, t.upr, t.cw_log2,
                          static_cast<const T*>(gy), static_cast<const T*>(out), static_cast<T*>(g), ws);
        }))
        return e;
    return launch(what, table_sum_kernel, dim3((unsigned)((W + kSumCols - 1) / kSumCols), (unsigned)C),
                  dim3(kThreads), 0, st, W, (uint32_t)G, (uint32_t)cpg, idx, ws, g_table);
}
