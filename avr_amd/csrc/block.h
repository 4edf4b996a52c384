// Workgroup-wide device helpers: the one fixed-order block reduction of the
// loss, metric and DoA kernels (criterion.hip, das.hip, metrics.hip, doa.hip),
// and the LDS-only barrier of the width-512 GEMMs.
//
// Those kernels promise "every sum in a fixed order, bitwise repeatable,
// batch-independent".  For a sum over a workgroup the order is the one written
// here and nowhere else: lane tid's value is entry tid of an LDS row, and the
// row is folded in halves, entry tid taking op(entry tid, entry tid + st) for
// st = THREADS/2, THREADS/4, ..., 1.
//
// Out of scope: optim.hip's shuffle block_sum (other order, lane 0 only); head/hashgrid's DPP wave scans (hot, one user).
#pragma once

#include <hip/hip_runtime.h>

namespace avr {

// Workgroup barrier that waits for the LDS traffic only: global loads and
// stores in flight are not waited for (__syncthreads would drain them; the
// compiler waits for a load where its registers are used); "memory" keeps LDS
// accesses on their side.  head.hip keeps its own, built from the waitcnt and
// barrier builtins: another instruction sequence to the scheduler, and hot.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

struct SumOp {
    template <typename T>
    __device__ T operator()(T a, T b) const { return a + b; }
};
struct MaxOp {  // fmaxf / fmax: a NaN operand loses to a number
    __device__ float operator()(float a, float b) const { return fmaxf(a, b); }
    __device__ double operator()(double a, double b) const { return fmax(a, b); }
};
struct MinOp {
    __device__ int operator()(int a, int b) const { return min(a, b); }
};

// v[c] <- the reduction of column c over the workgroup's THREADS lanes, in
// every lane.  red is [N][THREADS] of LDS.  A barrier before the first store
// and one after the last read: safe wherever it is called (by all lanes) and
// whatever red aliases.
template <int THREADS, int N, typename T, typename Op>
__device__ __forceinline__ void block_reduce(T (*red)[THREADS], T* v, Op op) {
    static_assert(THREADS >= 2 && (THREADS & (THREADS - 1)) == 0, "block_reduce folds in halves");
    const int tid = threadIdx.x;
    __syncthreads();
#pragma unroll
    for (int c = 0; c < N; ++c) red[c][tid] = v[c];
    __syncthreads();
    for (int st = THREADS / 2; st > 0; st >>= 1) {
        if (tid < st) {
#pragma unroll
            for (int c = 0; c < N; ++c) red[c][tid] = op(red[c][tid], red[c][tid + st]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int c = 0; c < N; ++c) v[c] = red[c][0];
    __syncthreads();
}

// one value per lane, red = THREADS entries of LDS
template <int THREADS, typename T, typename Op>
__device__ __forceinline__ T block_reduce1(T v, T* red, Op op) {
    block_reduce<THREADS, 1>(reinterpret_cast<T(*)[THREADS]>(red), &v, op);
    return v;
}
template <int THREADS, typename T>
__device__ __forceinline__ T block_sum(T v, T* red) { return block_reduce1<THREADS>(v, red, SumOp{}); }
template <int THREADS, typename T>
__device__ __forceinline__ T block_max(T v, T* red) { return block_reduce1<THREADS>(v, red, MaxOp{}); }
template <int THREADS>
__device__ __forceinline__ int block_min(int v, int* red) { return block_reduce1<THREADS>(v, red, MinOp{}); }

}  // namespace avr
