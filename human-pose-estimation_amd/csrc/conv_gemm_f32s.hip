// conv_gemm_f32s.hip -- the fp32 1x1 / strided / dual-source implicit GEMM of conv_gemm.hip on the bf16 matrix cores, fp32-exact.
//
// Both operands are split exactly into three bf16 pieces and the six products a_i w_j with i + j <= 2 are summed in fp32 (bf16_split.h:
// the derivation and the error bound): 6 x 32 = 192 cycles per 32x32x16 block against 8 x 64 = 512 on the fp32 MFMA.
//
//   * weights: split once on the host (hpe_finalize), three bf16 planes per weight row: piece j of Wt[n][k] at w + n * ldw + j * w_piece + k
//   * activations: LDS-DMA'd as fp32 exactly as in conv_gemm_f32_dma_kernel and split per wave in registers after the fragment read.
//     The wave grid is WN = 1 wide on the 4-wave tiles (each wave owns 32 rows x all 128 columns), so every A element is split by exactly
//     one wave of the workgroup; the 8-wave 128x128 tile (WN = 2) splits each element twice but issues the epilogue of the identity-block
//     expand layers (row stores + residual loads) from twice the waves, which those layers need.
//   * staging per slab (32 k): A [BM][32] fp32 (128-B rows, chunk swizzle c ^ ((r >> 1) & 7) as in conv_gemm.hip), then the three W pieces,
//     each [BN][32] bf16 (64-B rows, 4 chunks, swizzle c ^ ((r >> 2) & 3): a 16-lane ds_read_b128 group then covers 16 distinct 16-B slots
//     of the 256-B bank row).  Double buffered, one barrier per slab, the vmcnt wait written out in front of it (lds_dma.h).
//   * k labelling of one 16-deep MFMA step q: lane l supplies row l & 31, k = 16 q + 8 (l >> 5) .. + 7 -- for A the two logical fp32
//     chunks 4q + 2(l >> 5) + {0, 1}, for W the logical bf16 chunk 2q + (l >> 5); both in natural k order.
//   * two fp32 accumulators: a0 w0 alone in one, the five cross terms (2^-8 smaller and below) in the other, added once after the k loop.
//     The leading accumulator then takes one rounding per 16 k (the fp32 MFMA: one per 2 k); with all six products in one accumulator
//     the per-layer error against fp64 reached 1.6-1.8x the fp32 kernel's on two layers.
//   * summation order fixed by the program (no atomics): bitwise repeatable.
//   * epilogue, XCD-aware tile remap and NHWC layouts: those of conv_gemm_f32_dma_kernel (conv_gemm_common.h).
// Whole-tile launches only: small grids (split-K) stay on the fp32 kernel; the planner (hpe_api.hip) decides.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "bf16_split.h"
#include "conv_gemm_common.h"
#include "gemm_contract.h"
#include "hpe_internal.h"
#include "lds_dma.h"

namespace {

template <int MODE, int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(64 * WM * WN, 2) void conv_gemm_f32s_dma_kernel(GemmArgs p) {
    constexpr int MT = BM / WM / 32;
    constexpr int NT = BN / WN / 32;
    constexpr int NW = WM * WN;         // waves per workgroup (4 or 8)
    constexpr int NTHR = 64 * NW;
    constexpr int AP = BM / (8 * NW);   // DMA instructions per wave for the A rows of one slab (8 fp32 rows of 128 B each)
    constexpr int BP = BN / (16 * NW);  // ... per W piece (16 bf16 rows of 64 B each)
    constexpr int A_BYTES = BM * BK * 4;
    constexpr int W_BYTES = BN * BK * 2;  // one piece
    constexpr int BUF = A_BYTES + 3 * W_BYTES;  // bytes per staging buffer
    constexpr int EPB = BM * (BN + 4) * 4;      // epilogue transpose tile
    constexpr int LDS_BYTES = (2 * BUF > EPB) ? 2 * BUF : EPB;
    static_assert(NW == 4 || NW == 8, "4 or 8 waves per workgroup");
    static_assert(AP >= 1 && BP >= 1, "tile too small for the wave count");
    static_assert(MODE == GEMM_DENSE || MODE == GEMM_STRIDED || MODE == GEMM_DUAL, "1x1 layers only");

    __shared__ __attribute__((aligned(16))) float lds[LDS_BYTES / 4];
    char* const ldsb = reinterpret_cast<char*>(lds);

    // XCD-aware bijective remap: blocks b, b+8, ... (one XCD) walk consecutive tiles
    const int total = p.n_mtiles * p.n_ntiles;
    const int bid = blockIdx.x;
    const int tile = xcd_remap(bid, total);
    const int mtile = tile / p.n_ntiles;
    const int ntile = tile - mtile * p.n_ntiles;
    const int m0 = mtile * BM;
    const int n0 = ntile * BN;

    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wm = wave / WN;
    const int wn = wave - wm * WN;

    // ---- DMA sources.  A: instruction i of wave w fills rows (NW i + w) * 8 + (lane >> 3), LDS chunk lane & 7 (as conv_gemm.hip).
    //      W piece j: instruction i of wave w fills rows (NW i + w) * 16 + (lane >> 2), LDS chunk lane & 3.
    RowAddr arow[AP];
    int arow2[MODE == GEMM_DUAL ? AP : 1];
#pragma unroll
    for (int i = 0; i < AP; ++i) {
        const int r = (NW * i + wave) * 8 + (lane >> 3);
        const int lc = (lane & 7) ^ ((r >> 1) & 7);  // 0..7: make_row's stem branch needs lc * 4 < 32
        arow[i] = make_row<MODE>(p, m0 + r, lc * 4);
        if (MODE == GEMM_DUAL) arow2[i] = make_row<GEMM_STRIDED>(p, m0 + r, lc * 4).base;
    }
    const __bf16* const w16 = reinterpret_cast<const __bf16*>(p.w);
    const __bf16* wsrc[BP];
#pragma unroll
    for (int i = 0; i < BP; ++i) {
        const int r = (NW * i + wave) * 16 + (lane >> 2);
        const int lc = (lane & 3) ^ ((r >> 2) & 3);
        wsrc[i] = w16 + (size_t)(n0 + r) * p.ldw + lc * 8;
    }

    // ---- fragment read offsets (bytes inside a buffer) and swizzles
    int a_row[MT], a_x[MT], b_row[NT], b_x[NT];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        const int r = (wm * MT + i) * 32 + (lane & 31);
        a_row[i] = r * (BK * 4);
        a_x[i] = (r >> 1) & 7;
    }
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int r = (wn * NT + j) * 32 + (lane & 31);
        b_row[j] = A_BYTES + r * (BK * 2);
        b_x[j] = (r >> 2) & 3;
    }
    const int hi = lane >> 5;

    f32x16 acc[MT][NT], acx[MT][NT];  // a0 w0 / the cross terms
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = acx[i][j][e] = 0.f;

    // residual rows of the epilogue fetched before the main loop on the 8-wave tiles (the rule of conv_gemm_f32_dma_kernel)
    constexpr int R_TPR = BN / 4, R_RPP = NTHR / R_TPR, R_NPASS = BM / R_RPP;
    constexpr bool R_PRE = (NW == 8) && R_NPASS <= 4;
    f32x4 rpre[R_PRE ? R_NPASS : 1];
    bool r_pre = false;
    if constexpr (R_PRE) {
        const int rr_ = t / R_TPR;
        const int n = n0 + (t - rr_ * R_TPR) * 4;
        r_pre = p.res != nullptr && p.res_prefetch && (n + 3) < p.N;
        if (r_pre) {
#pragma unroll
            for (int pass = 0; pass < R_NPASS; ++pass) {
                const int m = m0 + pass * R_RPP + rr_;
                rpre[pass] = HPE_RES_LOAD(reinterpret_cast<const f32x4*>(p.res + (size_t)(m < p.M ? m : p.M - 1) * p.ldres + n));
            }
        }
    }

    auto issue_dma = [&](int slab, int buf) {
#pragma unroll
        for (int i = 0; i < AP; ++i) {
            const float* src;
            if (MODE == GEMM_DUAL)  // wave-uniform choice of the source by the slab index
                src = slab < p.k1_slabs ? p.x + (arow[i].base + slab * BK) : p.x2 + (arow2[i] + (slab - p.k1_slabs) * BK);
            else
                src = p.x + (arow[i].base + slab * BK);
            dma16(src, ldsb + buf + (NW * i + wave) * 1024);
        }
#pragma unroll
        for (int pc = 0; pc < 3; ++pc)
#pragma unroll
            for (int i = 0; i < BP; ++i)
                dma16(wsrc[i] + (size_t)pc * p.w_piece + slab * BK, ldsb + buf + A_BYTES + pc * W_BYTES + (NW * i + wave) * 1024);
    };

    const int S = p.K / BK;
    issue_dma(0, 0);
    wait_counts<0>();  // slab 0 has landed
    __syncthreads();

    for (int s = 0; s < S; ++s) {
        const int cur = (s & 1) * BUF;
        if (s + 1 < S) issue_dma(s + 1, BUF - cur);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            bf16x8 a0[MT], a1[MT], a2[MT], w0[NT], w1[NT], w2[NT];
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                const int lc = 4 * q + 2 * hi;
                const f32x4 lo = *reinterpret_cast<const f32x4*>(ldsb + cur + a_row[i] + ((lc ^ a_x[i]) << 4));
                const f32x4 up = *reinterpret_cast<const f32x4*>(ldsb + cur + a_row[i] + (((lc + 1) ^ a_x[i]) << 4));
                bf16_split3_cast<8>([&](int e) { return e < 4 ? lo[e] : up[e - 4]; }, a0[i], a1[i], a2[i]);
            }
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int off = cur + b_row[j] + (((2 * q + hi) ^ b_x[j]) << 4);
                w0[j] = *reinterpret_cast<const bf16x8*>(ldsb + off);
                w1[j] = *reinterpret_cast<const bf16x8*>(ldsb + off + W_BYTES);
                w2[j] = *reinterpret_cast<const bf16x8*>(ldsb + off + 2 * W_BYTES);
            }
            // cross terms smallest first
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    acx[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2[i], w0[j], acx[i][j], 0, 0, 0);
                    acx[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1[i], w1[j], acx[i][j], 0, 0, 0);
                    acx[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0[i], w2[j], acx[i][j], 0, 0, 0);
                    acx[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1[i], w0[j], acx[i][j], 0, 0, 0);
                    acx[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0[i], w1[j], acx[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0[i], w0[j], acc[i][j], 0, 0, 0);
                }
        }
        wait_counts<0>();  // this wave's part of slab s + 1 has landed
        __syncthreads();
    }

#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] += acx[i][j];
    conv_epilogue<BM, BN, WM, WN>(p, lds, acc, m0, n0, t, lane, wm, wn, rpre, R_PRE && r_pre);
}

template <int MODE, int TILE>
hipError_t launch_cfg(GemmArgs& p, hipStream_t st) {
    constexpr TileShape T = tile_shape(GEMM_K_F32S, TILE);
    constexpr int BM = T.bm, BN = T.bn, WM = T.wm, WN = T.wn;
    p.n_mtiles = (p.M + BM - 1) / BM;
    p.n_ntiles = (p.N + BN - 1) / BN;
    p.split_k = 1;
    p.res_prefetch = 1;
    hipLaunchKernelGGL((conv_gemm_f32s_dma_kernel<MODE, BM, BN, WM, WN>), dim3(p.n_mtiles * p.n_ntiles), dim3(64 * WM * WN), 0, st, p);
    return hipGetLastError();
}

template <int MODE>
hipError_t launch_mode(GemmArgs& p, int tile, hipStream_t st) {
    switch (tile) {
        case TILE_128x128: return launch_cfg<MODE, TILE_128x128>(p, st);
        case TILE_128x128_W8: return launch_cfg<MODE, TILE_128x128_W8>(p, st);
        case TILE_256x128_W8: return launch_cfg<MODE, TILE_256x128_W8>(p, st);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace

hipError_t hpe_launch_gemm_f32s(GemmArgs p, int mode, int tile, hipStream_t st) {
    if (gemm_contract(p, mode, tile, GEMM_K_F32S)) return hipErrorInvalidValue;
    switch (mode) {
        case GEMM_DENSE: return launch_mode<GEMM_DENSE>(p, tile, st);
        case GEMM_STRIDED: return launch_mode<GEMM_STRIDED>(p, tile, st);
        case GEMM_DUAL: return launch_mode<GEMM_DUAL>(p, tile, st);
        default: return hipErrorInvalidValue;
    }
}
