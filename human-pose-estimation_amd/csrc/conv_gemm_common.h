// conv_gemm_common.h -- pieces shared by the implicit-GEMM kernels: the A-row addressing and the k-slab walk of the implicit GEMM (all four:
// conv_gemm.hip, conv_gemm_f32s.hip, conv_gemm_bf16.hip, conv_gemm_bf16_p8.hip) and the fp32 epilogue (BN scale/shift, residual, ReLU, row
// stores; conv_gemm.hip, conv_gemm_f32s.hip, conv_stream_f32s.hip).  Everything here is in an anonymous namespace.
#pragma once
#include <hip/hip_runtime.h>

#include "hpe_internal.h"

#define BK 32

namespace {

// Per-thread description of one staged A row: element offset of its first k element (+ this thread's
// 16-B chunk) and, for the 3x3 conv, a 9-bit mask of the taps that fall inside the image.  Offsets are in elements of the kernel's
// type (fp32 or bf16).  c * CHUNK is the element offset of the thread's 16-B chunk inside the 128-B slab row, chunk = 0..7 (the callers form
// it as (lane & 7) ^ swizzle).  Two conventions, because where the multiply is written decides the instruction order hipcc emits and the
// device code of every kernel is kept as it was: the fp32 kernels pass chunk * 4 (c = 0, 4, .., 28) with CHUNK = 1, the bf16 kernels the
// chunk itself with CHUNK = 8.  PRECONDITION of the stem branch: c * CHUNK < 32 in fp32 (one kernel row per slab), < 64 in bf16 (two).
struct RowAddr {
    int base;
    unsigned mask;
};

template <int MODE, int CHUNK = 1>
__device__ __forceinline__ RowAddr make_row(const GemmArgs& p, int m, int c) {
    RowAddr r;
    r.mask = 0x1ffu;
    if (m >= p.M) m = p.M - 1;  // tail rows: read a valid row, the store guard drops the result
    if (MODE == GEMM_DENSE || MODE == GEMM_DUAL) {
        r.base = m * p.lda + c * CHUNK;
    } else {
        const int hw = p.Ho * p.Wo;
        const int b = m / hw;
        const int rem = m - b * hw;
        const int ho = rem / p.Wo;
        const int wo = rem - ho * p.Wo;
        if (MODE == GEMM_STRIDED) {
            r.base = ((b * p.Hi + ho * p.stride) * p.Wi + wo * p.stride) * p.Cin + c * CHUNK;
        } else if (MODE == GEMM_CONV3) {
            r.base = ((b * p.Hi + ho) * p.Wi + wo) * p.Cin + c * CHUNK;
            unsigned mk = 0;
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int dh = tap / 3 - 1, dw = tap % 3 - 1;
                if ((unsigned)(ho + dh) < (unsigned)p.Hi && (unsigned)(wo + dw) < (unsigned)p.Wi) mk |= 1u << tap;
            }
            r.mask = mk;
        } else {  // GEMM_STEM: padded input [B,Hi,Wi,4], 8 pixels x 4 ch = 32 elements per kernel row: a 32-float slab is one row (c < 32, so
                  // c >> 5 is 0: see the precondition above), a 64-bf16 slab two
            r.base = ((b * p.Hi + 2 * ho + (c * CHUNK >> 5)) * p.Wi + 2 * wo) * 4 + (c * CHUNK & 31);
        }
    }
    return r;
}

// Wave-uniform position of a k-slab inside the (kh, kw, cin) axis; advanced once per slab with scalar ops.  slab_advance -- SLAB: elements
// per k-slab (BK floats, or 64 bf16); STEM_ROWS: kernel rows of the stem's padded input per slab.  slab_seek (split-K) is fp32's alone.
struct SlabPos {
    int off;   // element offset added to every row base
    int tap;   // CONV3: kh*3+kw
    int cs;    // CONV3: cin slab inside the tap
};

template <int MODE, int SLAB = BK, int STEM_ROWS = 1>
__device__ __forceinline__ void slab_advance(const GemmArgs& p, SlabPos& sp) {
    if (MODE == GEMM_DENSE || MODE == GEMM_STRIDED || MODE == GEMM_DUAL) {
        sp.off += SLAB;
    } else if (MODE == GEMM_CONV3) {
        sp.cs += 1;
        sp.off += SLAB;
        if (sp.cs == p.cin_slabs) {
            sp.cs = 0;
            sp.tap += 1;
            const int kh = sp.tap / 3;
            sp.off = ((kh - 1) * p.Wi + (sp.tap - kh * 3 - 1)) * p.Cin;
        }
    } else {
        sp.off += STEM_ROWS * p.Wi * 4;
    }
}

template <int MODE>
__device__ __forceinline__ SlabPos slab_first(const GemmArgs& p) {
    SlabPos sp;
    sp.tap = 0;
    sp.cs = 0;
    sp.off = (MODE == GEMM_CONV3) ? (-p.Wi - 1) * p.Cin : 0;
    return sp;
}

template <int MODE>
__device__ __forceinline__ SlabPos slab_seek(const GemmArgs& p, int slab) {
    SlabPos sp;
    sp.tap = 0;
    sp.cs = 0;
    if (MODE == GEMM_DENSE || MODE == GEMM_STRIDED || MODE == GEMM_DUAL) {
        sp.off = slab * BK;
    } else if (MODE == GEMM_CONV3) {
        sp.tap = slab / p.cin_slabs;
        sp.cs = slab - sp.tap * p.cin_slabs;
        const int kh = sp.tap / 3;
        sp.off = ((kh - 1) * p.Wi + (sp.tap - kh * 3 - 1)) * p.Cin + sp.cs * BK;
    } else {
        sp.off = slab * p.Wi * 4;
    }
    return sp;
}

// Epilogue shared by the fp32 DMA kernel, the split-bf16 kernel (conv_gemm_f32s.hip) and the split-K fix-up kernel: BN scale/shift in registers, transpose through LDS,
// rows leave as 16 B per lane with the residual read the same way.
// The residual of an identity block is read here for the LAST time (the block input is dead after the add): -DHPE_F32_RES_NT reads it with
// the non-temporal policy (A/B knob of round 4; the bf16 chain kernel gained 1-2 % from the same idea).
#ifdef HPE_F32_RES_NT
#define HPE_RES_LOAD(ptr) __builtin_nontemporal_load(ptr)
#else
#define HPE_RES_LOAD(ptr) (*(ptr))
#endif
// rpre (use_pre): the residual vectors of this thread's rows, loaded by the caller before its main loop (else they are read here)
// STREAM: the caller is a persistent workgroup with the LDS-DMA of its next tile in flight (conv_stream_f32s.hip), and nothing here may wait
// for that: scale / shift of the lane's one column come in sc0 / sh0, loaded once (a load issued here would queue behind the DMA), and the
// barrier between transpose and row stores is an s_barrier behind this wave's LDS traffic alone (__syncthreads() is also a fence, which
// hipcc turns into vmcnt(0)); the caller has the vmcnt wait of that barrier in front of the call.  false: every one-tile kernel.
// THE STREAM CALLER COUNTS THIS FUNCTION'S VECTOR-MEMORY OPERATIONS in its s_waitcnt vmcnt(n): with STREAM, use_pre or p.res == nullptr, and a
// full tile (m0 + BM <= M, n0 + BN <= N) every thread issues exactly BM / RPP row stores and nothing else that vmcnt counts.  A load added
// to that path, or a store made conditional, makes the caller's count too large and lets it read a tile that has not landed: change
// NPASS / the wait_counts<> of conv_stream_f32s.hip with it (fewer operations than counted is the unsafe direction, more only waits longer)
template <int BM, int BN, int WM, int WN, bool STREAM = false, int NP>
__device__ __forceinline__ void conv_epilogue(const GemmArgs& p, float* lds, f32x16 (&acc)[BM / WM / 32][BN / WN / 32], int m0, int n0, int t,
                                              int lane, int wm, int wn, const f32x4 (&rpre)[NP], bool use_pre, float sc0 = 0.f, float sh0 = 0.f) {
    static_assert(!STREAM || BN / WN == 32, "STREAM: one column per lane");
    constexpr int MT = BM / WM / 32;
    constexpr int NT = BN / WN / 32;
    constexpr int NTHR = 64 * WM * WN;
    constexpr int EP = BN + 4;
    {
        const int col_l = lane & 31;
        const int row_l = 4 * (lane >> 5);
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int cl = (wn * NT + j) * 32 + col_l;
            const int n = n0 + cl;
            const bool n_ok = n < p.N;
            const float sc = STREAM ? sc0 : n_ok ? p.scale[n] : 0.f;
            const float sh = STREAM ? sh0 : n_ok ? p.shift[n] : 0.f;
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                const int rl = (wm * MT + i) * 32 + row_l;
#pragma unroll
                for (int e = 0; e < 16; ++e) lds[(rl + (e & 3) + 8 * (e >> 2)) * EP + cl] = acc[i][j][e] * sc + sh;
            }
        }
    }
    if constexpr (STREAM) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    else __syncthreads();
    {
        constexpr int TPR = BN / 4;
        constexpr int RPP = NTHR / TPR;
        const int r = t / TPR;
        const int c4 = (t - r * TPR) * 4;
        const int n = n0 + c4;
        const bool full = (n + 3) < p.N;
#pragma unroll
        for (int pass = 0; pass < BM / RPP; ++pass) {
            const int row = pass * RPP + r;
            const int m = m0 + row;
            if (m >= p.M || n >= p.N) continue;
            f32x4 v = *reinterpret_cast<const f32x4*>(&lds[row * EP + c4]);
            if (full) {
                if (use_pre) v += rpre[pass < NP ? pass : 0];
                else if (p.res) v += HPE_RES_LOAD(reinterpret_cast<const f32x4*>(p.res + (size_t)m * p.ldres + n));
                if (p.relu) {
                    v.x = fmaxf(v.x, 0.f);
                    v.y = fmaxf(v.y, 0.f);
                    v.z = fmaxf(v.z, 0.f);
                    v.w = fmaxf(v.w, 0.f);
                }
                if (p.y_slab8)
                    *reinterpret_cast<f32x4*>(p.y + ((size_t)(n >> 3) * p.M + m) * 8 + (n & 7)) = v;
                else
                    *reinterpret_cast<f32x4*>(p.y + (size_t)m * p.ldy + n) = v;
            } else {
                const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (n + u < p.N) {
                        float o = vv[u];
                        if (p.res) o += p.res[(size_t)m * p.ldres + n + u];
                        if (p.relu) o = fmaxf(o, 0.f);
                        p.y[(size_t)m * p.ldy + n + u] = o;
                    }
                }
            }
        }
    }
}

}  // namespace
