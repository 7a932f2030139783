// conv_gemm.hip -- fp32 implicit-GEMM convolution / dense layer on the gfx950 matrix cores.
//
// Computes  Y[m][n] = act( (sum_k A[m][k] * Wt[n][k]) * scale[n] + shift[n] + R[m][n] )
//   m : output pixel (b, ho, wo) flattened (NHWC)            -- or the image index for Dense layers
//   n : output channel
//   k : (kh, kw, cin) flattened with cin fastest (NHWC / HWIO order)
// which covers every conv of the Keras ResNet-50 v1 the reference instantiates
// (reference: src/models.py:35-41) with BatchNorm folded into (scale, shift), the residual add + ReLU of
// the bottleneck fused in the epilogue, and the three Dense layers of RegressionNetwork
// (reference: src/models.py:60-74; y = x @ kernel + bias is the scale == 1 case).
//
// conv_gemm_f32_dma_kernel is LDS-DMA staged: global_load_lds_dwordx4 writes the k-slabs straight into LDS, bank spread by an XOR
// swizzle on the per-lane source address.  (Rounds 1-4 also carried a register-staged kernel -- global_load_dwordx4 -> VGPR ->
// ds_write_b128, padded LDS pitch -- for A/B runs and the schedule ablations of DESIGN.md §4; no configuration selected it and it was
// removed.)
//
// CDNA4 mapping
//   * v_mfma_f32_32x32x2_f32: exact-fp32 matrix FMA (64 FLOP/clk/SIMD = the fp32 roofline, 157.3 TF).
//     Lane l supplies A[row = l&31][k = l>>5] and B[k = l>>5][col = l&31].
//   * A (activations) and W (weights, pre-packed [n][k] on the host at load time) are both staged in LDS
//     as [row][32 k] slabs (one 128-B line per row): one ds_read_b128 per lane then feeds FOUR MFMAs
//     (lanes 0-31 hold k = 8g..8g+3, lanes 32-63 hold k = 8g+4..8g+7 -- k is only a summation label,
//     A and B use the same labelling); the 16-lane b128 groups are bank-conflict-free (source-side XOR swizzle).
//   * double buffered: the loads of slab s+1 are in flight while slab s is multiplied; one barrier per slab.
//   * 64-wide waves in a WM x WN grid, each wave owns an (MT*32) x (NT*32) accumulator block; 4 or 8 waves.
//   * epilogue: BN scale/shift in registers, transpose through the (free) staging LDS, 16 B/lane row stores with the
//     residual read the same way.
//   * blockIdx -> tile mapping is XCD-aware: the N-tiles that share an A row-panel are consecutive
//     on ONE XCD (blocks b, b+8, ... share an L2), so the panel is fetched from HBM once.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "conv_gemm_common.h"
#include "gemm_contract.h"
#include "hpe_internal.h"
#include "lds_dma.h"

namespace {

// ---------------------------------------------------------------------------------------------------------
// LDS-DMA staged variant: `global_load_lds_dwordx4` writes each 16-B chunk straight into LDS (no VGPR round trip,
// no ds_write).  A wave-instruction fills 1 KiB = 8 unpadded 128-B rows; the bank spread that a padded pitch would give
// comes from an XOR swizzle applied on the per-lane SOURCE address instead:
// LDS chunk c of row r holds logical chunk c ^ ((r >> 1) & 7), and the fragment read applies the same XOR, which
// makes every 16-lane ds_read_b128 group hit 16 distinct 16-B slots of the 256-B bank row.
template <int MODE, int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(64 * WM * WN, (WM * WN) / 2) void conv_gemm_f32_dma_kernel(GemmArgs p) {
    constexpr int MT = BM / WM / 32;
    constexpr int NT = BN / WN / 32;
    constexpr int NW = WM * WN;        // waves per workgroup (4 or 8)
    constexpr int NTHR = 64 * NW;
    constexpr int AP = BM / (8 * NW);  // DMA instructions per wave for the A rows of one slab
    constexpr int BP = BN / (8 * NW);
    constexpr int EP = BN + 4;
    constexpr int BUF = (BM + BN) * BK;  // floats per staging buffer (unpadded rows)
    constexpr int LDS_FLOATS = (2 * BUF > BM * EP) ? 2 * BUF : BM * EP;
    static_assert(NW == 4 || NW == 8, "4 or 8 waves per workgroup");
    static_assert(AP >= 1 && BP >= 1, "tile too small for the wave count");

    __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];

    // Small grids (small batches, the Dense layers) are cut along K: workgroup bid owns K-slice bid % split_k of tile
    // bid / split_k, stores raw accumulators, and conv_gemm_fixup_kernel reduces the slices (fixed order) and runs the
    // epilogue.  split_k == 1: whole tiles with the XCD-aware bijective remap.
    const int total = p.n_mtiles * p.n_ntiles;
    const int bid = blockIdx.x;
    int tile, ks0 = 0, ks1 = p.K / BK, part = -1;
    if (p.split_k > 1) {
        tile = bid / p.split_k;
        part = bid - tile * p.split_k;
        const int S = p.K / BK;
        ks0 = (int)((long)part * S / p.split_k);
        ks1 = (int)((long)(part + 1) * S / p.split_k);
    } else {
        tile = xcd_remap(bid, total);
    }
    const int mtile = tile / p.n_ntiles;
    const int ntile = tile - mtile * p.n_ntiles;
    const int m0 = mtile * BM;
    const int n0 = ntile * BN;

    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wm = wave / WN;
    const int wn = wave - wm * WN;

    // ---- DMA sources: instruction i of wave w fills rows (4i + w) * 8 + (lane >> 3), LDS chunk lane & 7
    const int drow = lane >> 3;
    RowAddr arow[AP];
    int arow2[MODE == GEMM_DUAL ? AP : 1];  // GEMM_DUAL: the same rows in the second (strided) source
    const float* wsrc[BP];
#pragma unroll
    for (int i = 0; i < AP; ++i) {
        const int r = (NW * i + wave) * 8 + drow;
        const int lc = (lane & 7) ^ ((r >> 1) & 7);  // 0..7: make_row's stem branch needs lc * 4 < 32
        arow[i] = make_row<MODE>(p, m0 + r, lc * 4);
        if (MODE == GEMM_DUAL) arow2[i] = make_row<GEMM_STRIDED>(p, m0 + r, lc * 4).base;
    }
#pragma unroll
    for (int i = 0; i < BP; ++i) {
        const int r = (NW * i + wave) * 8 + drow;
        const int lc = (lane & 7) ^ ((r >> 1) & 7);
        wsrc[i] = p.w + (size_t)(n0 + r) * p.ldw + lc * 4;
    }

    // ---- fragment read offsets: row r of the wave tile, logical chunk 2g + (lane >> 5)
    int a_row[MT], b_row[NT], a_x[MT], b_x[NT];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        const int r = (wm * MT + i) * 32 + (lane & 31);
        a_row[i] = r * BK;
        a_x[i] = (r >> 1) & 7;
    }
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int r = (wn * NT + j) * 32 + (lane & 31);
        b_row[j] = (BM + r) * BK;
        b_x[j] = (r >> 1) & 7;
    }
    const int hi = lane >> 5;

    f32x16 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    // Residual rows of the epilogue, fetched NOW (8-wave tiles = the identity-block expand layers, which are all epilogue: 4 x 16 B per
    // thread): their HBM latency runs beside the operand DMA and the MFMAs instead of after the LDS transpose.
    constexpr int R_TPR = BN / 4, R_RPP = NTHR / R_TPR, R_NPASS = BM / R_RPP;
    constexpr bool R_PRE = (NW == 8) && R_NPASS <= 4;
    f32x4 rpre[R_PRE ? R_NPASS : 1];
    bool r_pre = false;
    if constexpr (R_PRE) {
        const int rr_ = t / R_TPR;
        const int n = n0 + (t - rr_ * R_TPR) * 4;
        r_pre = p.res != nullptr && p.res_prefetch && part < 0 && (n + 3) < p.N;
        if (r_pre) {
#pragma unroll
            for (int pass = 0; pass < R_NPASS; ++pass) {
                const int m = m0 + pass * R_RPP + rr_;
                rpre[pass] = HPE_RES_LOAD(reinterpret_cast<const f32x4*>(p.res + (size_t)(m < p.M ? m : p.M - 1) * p.ldres + n));
            }
        }
    }

    SlabPos sp = slab_seek<MODE>(p, ks0);

    auto issue_dma = [&](int slab, int buf) {
#pragma unroll
        for (int i = 0; i < AP; ++i) {
            const float* src;
            if (MODE == GEMM_CONV3) {
                const bool ok = (arow[i].mask >> sp.tap) & 1u;
                src = ok ? (p.x + (arow[i].base + sp.off)) : p.zero;
            } else if (MODE == GEMM_DUAL) {
                // wave-uniform choice of the source by the absolute slab index (also right inside a split-K slice)
                src = slab < p.k1_slabs ? p.x + (arow[i].base + slab * BK) : p.x2 + (arow2[i] + (slab - p.k1_slabs) * BK);
            } else {
                src = p.x + (arow[i].base + sp.off);
            }
            dma16(src, lds + buf + (NW * i + wave) * 8 * BK);
        }
#pragma unroll
        for (int i = 0; i < BP; ++i) dma16(wsrc[i] + slab * BK, lds + buf + (BM + (NW * i + wave) * 8) * BK);
    };

    issue_dma(ks0, 0);
    wait_counts<0>();  // written out in front of every barrier that publishes DMA'd data (lds_dma.h): slab ks0 has landed
    __syncthreads();

    for (int s = ks0; s < ks1; ++s) {
        const int cur = ((s - ks0) & 1) * BUF;
        if (s + 1 < ks1) {
            slab_advance<MODE>(p, sp);
            issue_dma(s + 1, BUF - cur);
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f32x4 fa[MT], fb[NT];
            const int lc = 2 * g + hi;
#pragma unroll
            for (int i = 0; i < MT; ++i) fa[i] = *reinterpret_cast<const f32x4*>(&lds[cur + a_row[i] + ((lc ^ a_x[i]) << 2)]);
#pragma unroll
            for (int j = 0; j < NT; ++j) fb[j] = *reinterpret_cast<const f32x4*>(&lds[cur + b_row[j] + ((lc ^ b_x[j]) << 2)]);
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int j = 0; j < NT; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i][ks], fb[j][ks], acc[i][j], 0, 0, 0);
        }
        wait_counts<0>();  // this wave's part of slab s + 1 has landed
        __syncthreads();
    }

    if (part >= 0) {
        // split-K slice: raw accumulators -> workspace [tile][slice][register quad][thread] (16 B per lane, coalesced)
        f32x4* dst = reinterpret_cast<f32x4*>(p.partial) + (size_t)(tile * p.split_k + part) * (MT * NT * 4 * NTHR) + t;
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int qd = 0; qd < 4; ++qd) {
                    f32x4 v = {acc[i][j][4 * qd], acc[i][j][4 * qd + 1], acc[i][j][4 * qd + 2], acc[i][j][4 * qd + 3]};
                    dst[((i * NT + j) * 4 + qd) * NTHR] = v;
                }
        return;
    }
    conv_epilogue<BM, BN, WM, WN>(p, lds, acc, m0, n0, t, lane, wm, wn, rpre, R_PRE && r_pre);
}

// Reduces the K-slices of every tile (fixed order -> bitwise reproducible) and runs the normal epilogue.
template <int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(64 * WM * WN) void conv_gemm_fixup_kernel(GemmArgs p) {
    constexpr int MT = BM / WM / 32;
    constexpr int NT = BN / WN / 32;
    constexpr int NTHR = 64 * WM * WN;
    constexpr int EP = BN + 4;
    __shared__ __attribute__((aligned(16))) float lds[BM * EP];
    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wm = wave / WN;
    const int wn = wave - wm * WN;
    const int tile = blockIdx.x;
    const int mtile = tile / p.n_ntiles;
    const int ntile = tile - mtile * p.n_ntiles;
    f32x16 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    const f32x4* src = reinterpret_cast<const f32x4*>(p.partial) + (size_t)tile * p.split_k * (MT * NT * 4 * NTHR) + t;
    for (int part = 0; part < p.split_k; ++part) {
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int qd = 0; qd < 4; ++qd) {
                    const f32x4 v = src[(size_t)part * (MT * NT * 4 * NTHR) + ((i * NT + j) * 4 + qd) * NTHR];
                    acc[i][j][4 * qd] += v.x;
                    acc[i][j][4 * qd + 1] += v.y;
                    acc[i][j][4 * qd + 2] += v.z;
                    acc[i][j][4 * qd + 3] += v.w;
                }
    }
    const f32x4 no_pre[1] = {{0.f, 0.f, 0.f, 0.f}};
    conv_epilogue<BM, BN, WM, WN>(p, lds, acc, mtile * BM, ntile * BN, t, lane, wm, wn, no_pre, false);
}

template <int MODE, int TILE>
hipError_t launch_cfg(GemmArgs& p, int splitk_min_slabs, hipStream_t st) {
    constexpr TileShape T = tile_shape(GEMM_K_F32, TILE);
    constexpr int BM = T.bm, BN = T.bn, WM = T.wm, WN = T.wn;
    p.n_mtiles = (p.M + BM - 1) / BM;
    p.n_ntiles = (p.N + BN - 1) / BN;
    const int grid = p.n_mtiles * p.n_ntiles;
    p.split_k = 1;
    if constexpr (WM * WN == 8) {
        p.res_prefetch = 1;
        hipLaunchKernelGGL((conv_gemm_f32_dma_kernel<MODE, BM, BN, WM, WN>), dim3(grid), dim3(512), 0, st, p);
        return hipGetLastError();
    } else {
        // latency-bound small grids: cut K so that about one workgroup per CU runs, splitk_min_slabs (>= 2, plan option) slabs per slice
        const int S = p.K / BK;
        if (p.partial && grid < 128 && S >= 2 * splitk_min_slabs) {
            int sk = 256 / grid;
            if (sk > S / splitk_min_slabs) sk = S / splitk_min_slabs;
            if (sk > 16) sk = 16;
            while (sk > 1 && (size_t)grid * sk * BM * BN > p.partial_floats) --sk;
            if (sk > 1) p.split_k = sk;
        }
        hipLaunchKernelGGL((conv_gemm_f32_dma_kernel<MODE, BM, BN, WM, WN>), dim3(grid * p.split_k), dim3(256), 0, st, p);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess || p.split_k == 1) return e;
        hipLaunchKernelGGL((conv_gemm_fixup_kernel<BM, BN, WM, WN>), dim3(grid), dim3(256), 0, st, p);
        return hipGetLastError();
    }
}

// the one place that instantiates the kernels: a tile id is a shape only through tile_shape (gemm_contract.h)
template <int MODE>
hipError_t launch_mode(GemmArgs& p, int tile, int splitk_min_slabs, hipStream_t st) {
    switch (tile) {
        case TILE_128x128: return launch_cfg<MODE, TILE_128x128>(p, splitk_min_slabs, st);
        case TILE_128x64: return launch_cfg<MODE, TILE_128x64>(p, splitk_min_slabs, st);
        case TILE_64x64: return launch_cfg<MODE, TILE_64x64>(p, splitk_min_slabs, st);
        case TILE_64x128: return launch_cfg<MODE, TILE_64x128>(p, splitk_min_slabs, st);
        case TILE_128x128_W8: return launch_cfg<MODE, TILE_128x128_W8>(p, splitk_min_slabs, st);
        case TILE_128x64_W8: return launch_cfg<MODE, TILE_128x64_W8>(p, splitk_min_slabs, st);
        case TILE_256x128_W8: return launch_cfg<MODE, TILE_256x128_W8>(p, splitk_min_slabs, st);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace

hipError_t hpe_launch_gemm(GemmArgs p, int mode, int tile, int splitk_min_slabs, hipStream_t st, int* split_k_out) {
    p.split_k = 0;
    hipError_t e = hipErrorInvalidValue;
    if (splitk_min_slabs >= 2 && !gemm_contract(p, mode, tile, GEMM_K_F32)) {
        switch (mode) {
            case GEMM_DENSE: e = launch_mode<GEMM_DENSE>(p, tile, splitk_min_slabs, st); break;
            case GEMM_STRIDED: e = launch_mode<GEMM_STRIDED>(p, tile, splitk_min_slabs, st); break;
            case GEMM_CONV3: e = launch_mode<GEMM_CONV3>(p, tile, splitk_min_slabs, st); break;
            case GEMM_STEM: e = launch_mode<GEMM_STEM>(p, tile, splitk_min_slabs, st); break;
            case GEMM_DUAL: e = launch_mode<GEMM_DUAL>(p, tile, splitk_min_slabs, st); break;
        }
    }
    if (split_k_out) *split_k_out = p.split_k;  // 0: rejected before a launcher ran
    return e;
}
