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
// Two kernels share the tiling and the epilogue:
//   conv_gemm_f32_dma_kernel  (default)  LDS-DMA staged: global_load_lds_dwordx4 writes the k-slabs straight into LDS,
//                                        bank spread by an XOR swizzle on the per-lane source address.
//   conv_gemm_f32_kernel      (HPE_STAGE=reg, kept for A/B and for the schedule ablations of DESIGN.md §4)
//                                        register staged: global_load_dwordx4 -> VGPR -> ds_write_b128, padded LDS pitch.
//
// CDNA4 mapping
//   * v_mfma_f32_32x32x2_f32: exact-fp32 matrix FMA (64 FLOP/clk/SIMD = the fp32 roofline, 157.3 TF).
//     Lane l supplies A[row = l&31][k = l>>5] and B[k = l>>5][col = l&31].
//   * A (activations) and W (weights, pre-packed [n][k] on the host at load time) are both staged in LDS
//     as [row][32 k] slabs (one 128-B line per row): one ds_read_b128 per lane then feeds FOUR MFMAs
//     (lanes 0-31 hold k = 8g..8g+3, lanes 32-63 hold k = 8g+4..8g+7 -- k is only a summation label,
//     A and B use the same labelling); the 16-lane b128 groups are bank-conflict-free (36-float pitch in the
//     register-staged kernel, source-side XOR swizzle in the DMA kernel).
//   * double buffered: the loads of slab s+1 are in flight while slab s is multiplied; one barrier per slab.
//   * 64-wide waves in a WM x WN grid, each wave owns an (MT*32) x (NT*32) accumulator block; 4 or 8 waves.
//   * epilogue: BN scale/shift in registers, transpose through the (free) staging LDS, 16 B/lane row stores with the
//     residual read the same way.
//   * blockIdx -> tile mapping is XCD-aware: the N-tiles that share an A row-panel are consecutive
//     on ONE XCD (blocks b, b+8, ... share an L2), so the panel is fetched from HBM once.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "conv_gemm_common.h"
#include "hpe_internal.h"

#define LDS_PITCH 36  // floats; 144 B row pitch -> conflict-free ds_read_b128 (see header comment)

namespace {

template <int MODE>
__device__ __forceinline__ f32x4 load_a(const GemmArgs& p, const RowAddr& r, const SlabPos& sp) {
    if (MODE == GEMM_CONV3) {
        // branch-free: out-of-image taps read the (always valid) centre pixel and are zeroed by a select
        const bool ok = (r.mask >> sp.tap) & 1u;
        f32x4 v = *reinterpret_cast<const f32x4*>(p.x + (r.base + (ok ? sp.off : sp.cs * BK)));
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        return ok ? v : z;
    }
    return *reinterpret_cast<const f32x4*>(p.x + (r.base + sp.off));
}

template <int MODE, int BM, int BN, int WM, int WN, int SCHED>
__global__ __launch_bounds__(256, 2) void conv_gemm_f32_kernel(GemmArgs p) {
    constexpr int MT = BM / WM / 32;
    constexpr int NT = BN / WN / 32;
    constexpr int AP = BM / 32;  // A rows staged per thread
    constexpr int BP = BN / 32;  // W rows staged per thread
    constexpr int EP = BN + 4;   // epilogue LDS pitch (floats)
    static_assert(WM * WN == 4, "4 waves per workgroup");
    static_assert(MT >= 1 && NT >= 1, "tile too small");
    static_assert(BM * EP <= 2 * (BM + BN) * LDS_PITCH, "epilogue tile must fit the staging LDS");

    __shared__ __attribute__((aligned(16))) float lds[2 * (BM + BN) * LDS_PITCH];
    constexpr int BUF = (BM + BN) * LDS_PITCH;

    // XCD-aware bijective remap: blocks b, b+8, ... (one XCD) walk consecutive tiles.
    const int total = p.n_mtiles * p.n_ntiles;
    const int bid = blockIdx.x;
    const int xcd = bid & 7;
    const int q = total >> 3, rr = total & 7;
    const int swz = (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + (bid >> 3);
    const int mtile = swz / p.n_ntiles;
    const int ntile = swz - mtile * p.n_ntiles;
    const int m0 = mtile * BM;
    const int n0 = ntile * BN;

    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wm = wave / WN;
    const int wn = wave - wm * WN;

    // ---- staging addresses: thread t stages 16 B (k chunk t&7) of rows (t>>3) + 32*i
    const int kc4 = (t & 7) * 4;
    const int srow = t >> 3;
    RowAddr arow[AP];
#pragma unroll
    for (int i = 0; i < AP; ++i) arow[i] = make_row<MODE>(p, m0 + srow + 32 * i, kc4);
    const float* wptr = p.w + (size_t)(n0 + srow) * p.ldw + kc4;
    const int lds_st = srow * LDS_PITCH + kc4;

    // ---- fragment read offsets (floats) inside a buffer
    const int frag = (lane & 31) * LDS_PITCH + 4 * (lane >> 5);
    const int a_off = (wm * MT * 32) * LDS_PITCH + frag;
    const int b_off = (BM + wn * NT * 32) * LDS_PITCH + frag;

    f32x16 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    f32x4 ra[AP], rb[BP];
    const int S = p.K / BK;
    SlabPos sp = slab_first<MODE>(p);

    auto load_slab = [&](int slab) {
#pragma unroll
        for (int i = 0; i < AP; ++i) ra[i] = load_a<MODE>(p, arow[i], sp);
#pragma unroll
        for (int i = 0; i < BP; ++i) rb[i] = *reinterpret_cast<const f32x4*>(wptr + (size_t)(32 * i) * p.ldw + slab * BK);
    };
    auto store_slab = [&](int buf) {
#pragma unroll
        for (int i = 0; i < AP; ++i) *reinterpret_cast<f32x4*>(&lds[buf + lds_st + 32 * i * LDS_PITCH]) = ra[i];
#pragma unroll
        for (int i = 0; i < BP; ++i) *reinterpret_cast<f32x4*>(&lds[buf + lds_st + (BM + 32 * i) * LDS_PITCH]) = rb[i];
    };
    auto mma_groups = [&](int buf, int g0, int g1) {
        const float* A = &lds[buf + a_off];
        const float* B = &lds[buf + b_off];
#pragma unroll
        for (int g = g0; g < g1; ++g) {
            f32x4 fa[MT], fb[NT];
#pragma unroll
            for (int i = 0; i < MT; ++i) fa[i] = *reinterpret_cast<const f32x4*>(A + i * 32 * LDS_PITCH + g * 8);
#pragma unroll
            for (int j = 0; j < NT; ++j) fb[j] = *reinterpret_cast<const f32x4*>(B + j * 32 * LDS_PITCH + g * 8);
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int j = 0; j < NT; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i][ks], fb[j][ks], acc[i][j], 0, 0, 0);
        }
    };

    // Software pipeline (register staged, LDS double buffered, one barrier per slab):
    //   iteration s multiplies LDS[s&1]; in the MIDDLE of its MFMA stream it retires the registers that hold
    //   slab s+1 into LDS[(s+1)&1] (free since the barrier that ended iteration s-1) and immediately re-issues
    //   the global loads of slab s+2 into the same registers, so every global load has a full iteration to land
    //   and the LDS writes issue in the shadow of the 64-cycle MFMAs.
#ifdef HPE_ABLATION
    unsigned long long t_clk0 = 0, t_rt0 = 0;
    if (p.dbg) {
        t_clk0 = __builtin_amdgcn_s_memtime();
        t_rt0 = __builtin_amdgcn_s_memrealtime();
    }
#endif
    load_slab(0);
    store_slab(0);
    if (S > 1) {
        slab_advance<MODE>(p, sp);
        load_slab(1);
    }
    __syncthreads();

    if (SCHED == 8 || SCHED == 9) {
        // Fully interleaved steady state, one basic block per slab.  LDS operations keep their source order
        // (the compiler must assume the staging writes alias the fragment reads), so the source is written in
        // the order we want them issued: per k-group g (16*MT*NT/4 MFMAs) -> prefetch the fragments of g+1,
        // multiply g, retire 1/4 of the staged registers into the other LDS buffer and re-issue their global
        // loads.  sched_group_barrier then pins the MFMAs between those memory instructions so that each
        // VMEM / DS issue sits in the shadow of a 64-cycle MFMA.
        constexpr int QA = AP / 4 > 0 ? AP / 4 : 1;  // staged A rows retired per k-group
        constexpr int QB = BP / 4 > 0 ? BP / 4 : 1;
        constexpr int GA = AP / QA, GB = BP / QB;    // groups that retire A / B rows (4, or 2 for 64-row tiles)
        constexpr int MPG = 4 * MT * NT;             // MFMAs per k-group
        int s = 0;
        for (; s + 2 < S; ++s) {
            const int cur = (s & 1) * BUF;
            const int nxt = BUF - cur;
            const float* A = &lds[cur + a_off];
            const float* B = &lds[cur + b_off];
            slab_advance<MODE>(p, sp);
            f32x4 fa[2][MT], fb[2][NT];
#pragma unroll
            for (int i = 0; i < MT; ++i) fa[0][i] = *reinterpret_cast<const f32x4*>(A + i * 32 * LDS_PITCH);
#pragma unroll
            for (int j = 0; j < NT; ++j) fb[0][j] = *reinterpret_cast<const f32x4*>(B + j * 32 * LDS_PITCH);
#define HPE_KGROUP(G)                                                                                                  \
    {                                                                                                                  \
        if (G < 3) {                                                                                                   \
            _Pragma("unroll") for (int i = 0; i < MT; ++i) fa[(G + 1) & 1][i] =                                        \
                *reinterpret_cast<const f32x4*>(A + i * 32 * LDS_PITCH + (G + 1) * 8);                                 \
            _Pragma("unroll") for (int j = 0; j < NT; ++j) fb[(G + 1) & 1][j] =                                        \
                *reinterpret_cast<const f32x4*>(B + j * 32 * LDS_PITCH + (G + 1) * 8);                                 \
        }                                                                                                              \
        _Pragma("unroll") for (int ks = 0; ks < 4; ++ks) _Pragma("unroll") for (int i = 0; i < MT; ++i)                \
            _Pragma("unroll") for (int j = 0; j < NT; ++j) acc[i][j] =                                                 \
                __builtin_amdgcn_mfma_f32_32x32x2f32(fa[G & 1][i][ks], fb[G & 1][j][ks], acc[i][j], 0, 0, 0);          \
        if (G < GA) {                                                                                                  \
            _Pragma("unroll") for (int q = 0; q < QA; ++q) {                                                           \
                const int i = G * QA + q;                                                                              \
                *reinterpret_cast<f32x4*>(&lds[nxt + lds_st + 32 * i * LDS_PITCH]) = ra[i];                            \
                ra[i] = load_a<MODE>(p, arow[i], sp);                                                                  \
            }                                                                                                          \
        }                                                                                                              \
        if (G < GB) {                                                                                                  \
            _Pragma("unroll") for (int q = 0; q < QB; ++q) {                                                           \
                const int i = G * QB + q;                                                                              \
                *reinterpret_cast<f32x4*>(&lds[nxt + lds_st + (BM + 32 * i) * LDS_PITCH]) = rb[i];                     \
                rb[i] = *reinterpret_cast<const f32x4*>(wptr + (size_t)(32 * i) * p.ldw + (s + 2) * BK);               \
            }                                                                                                          \
        }                                                                                                              \
        if (SCHED == 9) {                                                                                              \
            constexpr int NST = (G < GA ? QA : 0) + (G < GB ? QB : 0);                                                 \
            if (G < 3) __builtin_amdgcn_sched_group_barrier(0x100, MT + NT, 0);                                        \
            if constexpr (NST == 0) {                                                                                  \
                __builtin_amdgcn_sched_group_barrier(0x008, MPG, 0);                                                   \
            } else {                                                                                                   \
                _Pragma("unroll") for (int q = 0; q < NST; ++q) {                                                      \
                    __builtin_amdgcn_sched_group_barrier(0x008, MPG / NST, 0);                                         \
                    __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);                                                 \
                    __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);                                                 \
                }                                                                                                      \
            }                                                                                                          \
        }                                                                                                              \
    }
            HPE_KGROUP(0)
            HPE_KGROUP(1)
            HPE_KGROUP(2)
            HPE_KGROUP(3)
#undef HPE_KGROUP
            __syncthreads();
        }
        for (; s < S; ++s) {
            const int cur = (s & 1) * BUF;
            mma_groups(cur, 0, 2);
            if (s + 1 < S) store_slab(BUF - cur);
            mma_groups(cur, 2, 4);
            __syncthreads();
        }
    } else
    for (int s = 0; s < S; ++s) {
        const int cur = (s & 1) * BUF;
        if (SCHED == 0) {
            mma_groups(cur, 0, 2);
            if (s + 1 < S) {
                store_slab(BUF - cur);
                if (s + 2 < S) {
                    slab_advance<MODE>(p, sp);
                    load_slab(s + 2);
                }
            }
            mma_groups(cur, 2, 4);
        } else if (SCHED == 1) {
            mma_groups(cur, 0, 2);
            __builtin_amdgcn_sched_barrier(0);
            if (s + 1 < S) {
                store_slab(BUF - cur);
                __builtin_amdgcn_sched_barrier(0);
                if (s + 2 < S) {
                    slab_advance<MODE>(p, sp);
                    load_slab(s + 2);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            mma_groups(cur, 2, 4);
        } else if (SCHED == 6) {  // ablation: global loads, no LDS writes
            if (s + 2 < S) {
                slab_advance<MODE>(p, sp);
                load_slab(s + 2);
            }
            mma_groups(cur, 0, 4);
#pragma unroll
            for (int i = 0; i < AP; ++i) asm volatile("" ::"v"(ra[i]));
#pragma unroll
            for (int i = 0; i < BP; ++i) asm volatile("" ::"v"(rb[i]));
        } else if (SCHED == 7) {  // ablation: LDS writes, no global loads
            mma_groups(cur, 0, 2);
            if (s + 1 < S) store_slab(BUF - cur);
            mma_groups(cur, 2, 4);
        } else if (SCHED == 3) {  // ablation: no global loads / LDS writes in the loop (wrong results)
            mma_groups(cur, 0, 4);
        } else if (SCHED == 4) {  // ablation: 3 + no barrier
            mma_groups(0, 0, 4);
            continue;
        } else if (SCHED == 5) {  // ablation: MFMA only, operands fixed in registers
            f32x4 fa[MT], fb[NT];
#pragma unroll
            for (int i = 0; i < MT; ++i) fa[i] = ra[i % AP];
#pragma unroll
            for (int j = 0; j < NT; ++j) fb[j] = rb[j % BP];
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int ks = 0; ks < 4; ++ks)
#pragma unroll
                    for (int i = 0; i < MT; ++i)
#pragma unroll
                        for (int j = 0; j < NT; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i][ks], fb[j][ks], acc[i][j], 0, 0, 0);
            continue;
        } else {
            mma_groups(cur, 0, 1);
            __builtin_amdgcn_sched_barrier(0);
            if (s + 1 < S) store_slab(BUF - cur);
            mma_groups(cur, 1, 2);
            __builtin_amdgcn_sched_barrier(0);
            if (s + 2 < S) {
                slab_advance<MODE>(p, sp);
                load_slab(s + 2);
            }
            mma_groups(cur, 2, 3);
            __builtin_amdgcn_sched_barrier(0);
            mma_groups(cur, 3, 4);
        }
        __syncthreads();
    }

#ifdef HPE_ABLATION
    if (p.dbg && t == 0) {
        p.dbg[2 * bid] = __builtin_amdgcn_s_memtime() - t_clk0;
        p.dbg[2 * bid + 1] = __builtin_amdgcn_s_memrealtime() - t_rt0;
    }
#endif
    // ---- epilogue.  C/D layout of the 32x32 MFMA: col = lane&31, row = (e&3) + 8*(e>>2) + 4*(lane>>5).
    // BN-scale/shift is applied in registers, the tile is transposed through LDS (the staging buffers are
    // free after the last barrier) and leaves as full rows: 16 B per lane, BN*4 contiguous bytes per row,
    // with the residual read the same way.
    {
        const int col_l = lane & 31;
        const int row_l = 4 * (lane >> 5);
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int cl = (wn * NT + j) * 32 + col_l;
            const int n = n0 + cl;
            const bool n_ok = n < p.N;
            const float sc = n_ok ? p.scale[n] : 0.f;
            const float sh = n_ok ? p.shift[n] : 0.f;
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                const int rl = (wm * MT + i) * 32 + row_l;
#pragma unroll
                for (int e = 0; e < 16; ++e) lds[(rl + (e & 3) + 8 * (e >> 2)) * EP + cl] = acc[i][j][e] * sc + sh;
            }
        }
    }
    __syncthreads();
    {
        constexpr int TPR = BN / 4;     // threads per output row
        constexpr int RPP = 256 / TPR;  // rows per pass
        const int r = t / TPR;
        const int c4 = (t - r * TPR) * 4;
        const int n = n0 + c4;
        const bool full = (n + 3) < p.N;
#pragma unroll 4
        for (int pass = 0; pass < BM / RPP; ++pass) {
            const int row = pass * RPP + r;
            const int m = m0 + row;
            if (m >= p.M || n >= p.N) continue;
            f32x4 v = *reinterpret_cast<const f32x4*>(&lds[row * EP + c4]);
            if (full) {
                if (p.res) v += *reinterpret_cast<const f32x4*>(p.res + (size_t)m * p.ldres + n);
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

// ---------------------------------------------------------------------------------------------------------
// LDS-DMA staged variant: `global_load_lds_dwordx4` writes each 16-B chunk straight into LDS (no VGPR round trip,
// no ds_write).  A wave-instruction fills 1 KiB = 8 unpadded 128-B rows; the bank spread the padded pitch gave the
// register-staged kernel comes from an XOR swizzle applied on the per-lane SOURCE address instead:
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
        const int xcd = bid & 7;
        const int q = total >> 3, rr = total & 7;
        tile = (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + (bid >> 3);
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
        const int lc = (lane & 7) ^ ((r >> 1) & 7);
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
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                             (__attribute__((address_space(3))) void*)(lds + buf + (NW * i + wave) * 8 * BK), 16, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < BP; ++i) {
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(wsrc[i] + slab * BK),
                                             (__attribute__((address_space(3))) void*)(lds + buf + (BM + (NW * i + wave) * 8) * BK), 16, 0,
                                             0);
        }
    };

    issue_dma(ks0, 0);
    // The wait for the LDS-DMA is WRITTEN OUT in front of every barrier that publishes DMA'd data (here and at the end of the loop body):
    // __syncthreads() alone is a workgroup fence + s_barrier, and whether hipcc adds a vmcnt wait to it depends on the control flow around
    // the DMA issue (round 3: conv_wino4.hip got lgkmcnt only and raced).  tools/isa_lint.py / tests/test_isa_lint.py check the ISA.
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
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
        __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): this wave's part of slab s + 1 has landed (see above)
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

// environment knobs of the launcher: read once, in a thread-safe function-local static initialiser
int stage_variant() {
    static const int v = [] {
        const char* e = getenv("HPE_STAGE");
        return (e && e[0] == 'r') ? 0 : 1;  // "reg" = register staged, default = LDS-DMA
    }();
    return v;
}

int sched_variant() {
    static const int v = [] {
        const char* e = getenv("HPE_SCHED");
        const int x = e ? atoi(e) : 0;
        return (x < 0 || x > 9) ? 0 : x;
    }();
    return v;
}

int splitk_enabled() {
    static const int v = [] {
        const char* e = getenv("HPE_SPLITK");
        return e ? atoi(e) : 1;
    }();
    return v;
}

template <int MODE, int BM, int BN, int WM, int WN>
hipError_t launch_cfg(GemmArgs& p, hipStream_t st) {
    p.n_mtiles = (p.M + BM - 1) / BM;
    p.n_ntiles = (p.N + BN - 1) / BN;
    const int grid = p.n_mtiles * p.n_ntiles;
    p.split_k = 1;
    if constexpr (WM * WN == 8) {
        static const int res_prefetch = [] {
            const char* e = getenv("HPE_RES_PREFETCH");
            return e ? atoi(e) : 1;
        }();
        p.res_prefetch = res_prefetch;
        hipLaunchKernelGGL((conv_gemm_f32_dma_kernel<MODE, BM, BN, WM, WN>), dim3(grid), dim3(512), 0, st, p);
        return hipGetLastError();
    } else {
    if ((stage_variant() == 1 && p.zero) || MODE == GEMM_DUAL) {
        // latency-bound small grids: cut K so that about one workgroup per CU runs (>= 4 slabs per slice)
        const int S = p.K / BK;
        // slabs per slice: >= 4 (HPE_SPLITK_SLABS; a slice shorter than that is all launch ramp).  Every split layer pays a second,
        // dependent launch (the fix-up), which costs a single frame about what 6-8 more slabs in the main loop cost.
        static const int min_slabs = [] {
            const char* e = getenv("HPE_SPLITK_SLABS");
            const int v = e ? atoi(e) : 4;
            return v < 2 ? 2 : v;
        }();
        if (p.partial && splitk_enabled() && grid < 128 && S >= 2 * min_slabs) {
            int sk = 256 / grid;
            if (sk > S / min_slabs) sk = S / min_slabs;
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
    if constexpr (MODE == GEMM_DUAL) return hipErrorInvalidValue;  // (not reached: the dual-source mode is LDS-DMA only)
    else
    switch (sched_variant()) {
        case 1: hipLaunchKernelGGL((conv_gemm_f32_kernel<MODE, BM, BN, WM, WN, 1>), dim3(grid), dim3(256), 0, st, p); break;
        case 2: hipLaunchKernelGGL((conv_gemm_f32_kernel<MODE, BM, BN, WM, WN, 2>), dim3(grid), dim3(256), 0, st, p); break;
#ifdef HPE_ABLATION
        case 3: hipLaunchKernelGGL((conv_gemm_f32_kernel<MODE, BM, BN, WM, WN, 3>), dim3(grid), dim3(256), 0, st, p); break;
        case 4: hipLaunchKernelGGL((conv_gemm_f32_kernel<MODE, BM, BN, WM, WN, 4>), dim3(grid), dim3(256), 0, st, p); break;
        case 5: hipLaunchKernelGGL((conv_gemm_f32_kernel<MODE, BM, BN, WM, WN, 5>), dim3(grid), dim3(256), 0, st, p); break;
        case 6: hipLaunchKernelGGL((conv_gemm_f32_kernel<MODE, BM, BN, WM, WN, 6>), dim3(grid), dim3(256), 0, st, p); break;
        case 7: hipLaunchKernelGGL((conv_gemm_f32_kernel<MODE, BM, BN, WM, WN, 7>), dim3(grid), dim3(256), 0, st, p); break;
        case 8: hipLaunchKernelGGL((conv_gemm_f32_kernel<MODE, BM, BN, WM, WN, 8>), dim3(grid), dim3(256), 0, st, p); break;
        case 9: hipLaunchKernelGGL((conv_gemm_f32_kernel<MODE, BM, BN, WM, WN, 9>), dim3(grid), dim3(256), 0, st, p); break;
#endif
        default: hipLaunchKernelGGL((conv_gemm_f32_kernel<MODE, BM, BN, WM, WN, 0>), dim3(grid), dim3(256), 0, st, p); break;
    }
    return hipGetLastError();
    }
}

template <int MODE>
hipError_t launch_mode(GemmArgs& p, int tile, hipStream_t st) {
    switch (tile) {
        case TILE_128x128: return launch_cfg<MODE, 128, 128, 2, 2>(p, st);
        case TILE_128x64: return launch_cfg<MODE, 128, 64, 2, 2>(p, st);
        case TILE_64x64: return launch_cfg<MODE, 64, 64, 2, 2>(p, st);
        case TILE_64x128: return launch_cfg<MODE, 64, 128, 2, 2>(p, st);
        case TILE_128x128_W8: return launch_cfg<MODE, 128, 128, 2, 4>(p, st);
        case TILE_128x64_W8: return launch_cfg<MODE, 128, 64, 4, 2>(p, st);
        case TILE_256x128_W8: return launch_cfg<MODE, 256, 128, 4, 2>(p, st);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace

// Host-side shape contract (checked here so a bad plan cannot fault on the device).
hipError_t hpe_launch_gemm(GemmArgs p, int mode, int tile, hipStream_t st) {
    if (p.M <= 0 || p.N <= 0 || p.K <= 0 || (p.K % BK) != 0 || (p.ldw % 4) != 0 || p.ldw < p.K) return hipErrorInvalidValue;
    if (!p.x || !p.w || !p.y || !p.scale || !p.shift) return hipErrorInvalidValue;
    // vector epilogue: 16-B aligned rows of y / residual
    if ((p.ldy % 4) != 0 || ((uintptr_t)p.y & 15) != 0) return hipErrorInvalidValue;
    if (p.y_slab8 && (p.N % 8) != 0) return hipErrorInvalidValue;
    if (p.res && ((p.ldres % 4) != 0 || ((uintptr_t)p.res & 15) != 0)) return hipErrorInvalidValue;
    if (((uintptr_t)p.x & 15) != 0 || ((uintptr_t)p.w & 15) != 0) return hipErrorInvalidValue;
    const int bn = (tile == TILE_128x128 || tile == TILE_64x128 || tile == TILE_128x128_W8 || tile == TILE_256x128_W8) ? 128 : 64;
    const int n_pad = ((p.N + bn - 1) / bn) * bn;
    if (n_pad > p.w_rows) return hipErrorInvalidValue;  // packed weights must cover the padded N tiles
    switch (mode) {
        case GEMM_DENSE:
            if (p.lda < p.K || (p.lda % 4) != 0) return hipErrorInvalidValue;
            return launch_mode<GEMM_DENSE>(p, tile, st);
        case GEMM_STRIDED:
            if (p.Cin != p.K || (p.Cin % 4) != 0) return hipErrorInvalidValue;
            if ((p.Ho - 1) * p.stride >= p.Hi || (p.Wo - 1) * p.stride >= p.Wi) return hipErrorInvalidValue;
            return launch_mode<GEMM_STRIDED>(p, tile, st);
        case GEMM_CONV3:
            if ((p.Cin % BK) != 0 || p.K != 9 * p.Cin || p.cin_slabs != p.Cin / BK || p.Ho != p.Hi || p.Wo != p.Wi)
                return hipErrorInvalidValue;
            return launch_mode<GEMM_CONV3>(p, tile, st);
        case GEMM_STEM:
            if (p.K != 7 * BK || p.Hi < 2 * (p.Ho - 1) + 7 || p.Wi < 2 * (p.Wo - 1) + 8) return hipErrorInvalidValue;
            return launch_mode<GEMM_STEM>(p, tile, st);
        case GEMM_DUAL:
            if (!p.x2 || ((uintptr_t)p.x2 & 15) != 0 || p.k1_slabs < 1 || p.k1_slabs * BK >= p.K || p.lda < p.k1_slabs * BK || (p.lda % 4) != 0)
                return hipErrorInvalidValue;
            if (p.Cin != p.K - p.k1_slabs * BK || (p.Cin % 4) != 0 || p.M != (p.M / (p.Ho * p.Wo)) * p.Ho * p.Wo) return hipErrorInvalidValue;
            if ((p.Ho - 1) * p.stride >= p.Hi || (p.Wo - 1) * p.stride >= p.Wi) return hipErrorInvalidValue;
            return launch_mode<GEMM_DUAL>(p, tile, st);
        default: return hipErrorInvalidValue;
    }
}
