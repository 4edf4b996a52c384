// The ray stream, host side: what the launchers of the four ray-reduction
// kernels share (render_fwd.hip: ray_reduce_fwd / ray_reduce_mc_fwd,
// render_bwd.hip: their adjoints).  One workgroup per (ray split, column
// group, b) walks the rays of its split and reads each ray's (super-)row once
// with 16-byte loads.  Here: the block-shape rule, the dispatch over the
// (chunks per lane, launch bound) pairs that can occur, the vector-form
// predicate and the shared constants.  The kernels keep their own device
// code: a shared device scaffold was measured and cost registers and time
// (DESIGN.md section 21).
#pragma once

#include "common.h"

namespace avr {

constexpr int kMaxStreamThreads = 1024;
constexpr int kMaxGroupRays = 4096;  // G * rays per split (LDS: 8 or 12 bytes each of w/delay[/dot])
// Rows in flight per lane of the streaming reduction (non-temporal loads):
// the best of the sweeps (profiles/r01_tune*; 8 rows was slower).
constexpr int kReduceRows = 4;

// C receiver channels run in blocks of 4, then 2, then 1
constexpr int kMaxChannels = 16;
constexpr int mc_block(int left) { return left >= 4 ? 4 : left >= 2 ? 2 : 1; }

// The one-pass form of up to 16 channels (render_mc16.hip): a wave takes a
// strip of 16 chunks and walks the rays in batches of kMc16Batch groups of 4
// (the k of v_mfma_f32_16x16x4_f32); at most kMc16Waves waves per workgroup
// loop over the strips of a row.  Its LDS slab holds a delay and 16 products
// w*g per ray, the rays padded to whole batches, and may use a CU's 160 KiB.
constexpr int kMc16Waves = 8;
template <int VEC>
constexpr int kMc16Batch = VEC == 4 ? 8 : 4;
constexpr int kMc16RayBytes = 4 + 4 * kMaxChannels;
constexpr int kMc16RayPad = 32;  // 4 * the largest kMc16Batch
constexpr int mc16_max_rays() { return (int)(160 * 1024 / kMc16RayBytes) / kMc16RayPad * kMc16RayPad; }
constexpr int mc16_padded(int rays) { return ((rays < 1 ? 1 : rays) + kMc16RayPad - 1) & ~(kMc16RayPad - 1); }

// The 16-byte vector form needs every signal-shaped tensor 16-byte aligned
// and rows of one (b, s) column at one alignment phase: S*T % VEC == 0.
template <typename Tin, typename... Ptr>
bool vector_ok(int64_t row, const Ptr*... ptrs) {
    bool ok = row % Vec16<Tin>::N == 0;
    ((ok = reinterpret_cast<uintptr_t>(ptrs) % 16 == 0 && ok), ...);
    return ok;
}

struct StreamShape {
    int cpt, threads;
};

// Chunks per lane and block size for super-rows of G columns: the largest
// alignment phase of a group start (s0 a multiple of G; S*T % VEC == 0, so
// the phases repeat after VEC groups), the chunks of such a row, the fewest
// chunks per lane that fit kMaxStreamThreads lanes, whole waves.
template <int VEC>
StreamShape stream_shape(int S, int T, int G) {
    int max_phase = 0;
    for (int s0 = 0; s0 < S && s0 < VEC * G; s0 += G) max_phase = max(max_phase, (int)(((int64_t)s0 * T) % VEC));
    const int nch = (G * T + max_phase + VEC - 1) / VEC;
    StreamShape sh{1, 0};
    while ((nch + sh.cpt - 1) / sh.cpt > kMaxStreamThreads) ++sh.cpt;
    sh.threads = max(64, ((nch + sh.cpt - 1) / sh.cpt + 63) / 64 * 64);
    return sh;
}

// fn(chunks per lane, launch bound) as integral constants for one shape of
// stream_shape().  The bound is 512 threads (256 VGPRs per lane) or 1024
// (128).  Only the pairs that can occur are instantiated:
//  - cpt >= 2 is chosen only when nch > 1024*(cpt-1); then ceil(nch/cpt) >=
//    513, the block has at least 576 threads and the 512 bound is never taken;
//  - MAXCPT is the largest cpt the caller's kernel family is built for.
//    With T <= 16384 a 16-bit vector row has at most 2049 chunks (3 per
//    lane) and a G > 1 super-row of the backward at most 513 (1 per lane),
//    so nothing more can occur there.  A 4-byte vector row can reach 4097
//    chunks and an element-wise row 16384: those families are built up to
//    4 per lane, and a row of more than 4096 chunks is refused at run time
//    ("T too long"), as before.
// So a family has MAXCPT + 1 kernels instead of 8.  Anything else is
// AVR_E_CONFIG: never a fall-through to a kernel of another shape.
template <int MAXCPT, typename F>
int dispatch_stream(int cpt, int threads, const char* what, F&& fn) {
    using std::integral_constant;
    if (cpt == 1 && threads <= 512) return fn(integral_constant<int, 1>{}, integral_constant<int, 512>{});
    if (threads > 512 && threads <= kMaxStreamThreads) {
        if (cpt == 1) return fn(integral_constant<int, 1>{}, integral_constant<int, 1024>{});
        if constexpr (MAXCPT >= 2)
            if (cpt == 2) return fn(integral_constant<int, 2>{}, integral_constant<int, 1024>{});
        if constexpr (MAXCPT >= 3)
            if (cpt == 3) return fn(integral_constant<int, 3>{}, integral_constant<int, 1024>{});
        if constexpr (MAXCPT >= 4)
            if (cpt == 4) return fn(integral_constant<int, 4>{}, integral_constant<int, 1024>{});
    }
    return fail(AVR_E_CONFIG, std::string(what) + ": T too long for this build");
}
// largest chunks per lane of a G = 1 kernel family (see dispatch_stream)
template <typename Tin, bool VECTOR>
constexpr int kStreamMaxCpt = (VECTOR && Vec16<Tin>::N == 8) ? 3 : 4;

}  // namespace avr
