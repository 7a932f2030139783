// conv_stream_f32s.hip -- the identity-block expand layers with a short k axis (1x1 / stride 1, K = C <= 128, N = 4C, + residual + ReLU on
// the 56x56 and 28x28 maps: res2c_branch2c, res3{b,c,d}_branch2c) and the dual-source launch of the stage-2 conv_block (res2a_branch2c +
// res2a_branch1: K = 64 + 64 over the concatenated k axis, folded weights, no residual) on the bf16 matrix cores, fp32-exact
// (bf16_split.h), as a persistent workgroup that keeps its weights and streams the activations.
//
// With K = 64 or 128 a 128-wide tile of conv_gemm_f32s.hip has two or four k-slabs: a grid of one-tile workgroups is all prologue and
// epilogue, and its LDS-DMA queue drains at every tile.  Here the whole weight matrix of an N-slice is on the CU for the launch:
//
//   * a workgroup (4 waves) owns the 128 couts n0 .. n0 + 127 and walks the M tiles of 32 rows  walker, walker + walkers, ...; wave w owns the
//     32 couts n0 + 32 w .. + 31 of EVERY row of the tile (wave grid 1 x 4).
//   * weights: the three bf16 pieces of the wave's 32 couts x K are MFMA B operands in registers for the whole launch, K / 16 x 3 x 4 =
//     48 (K = 64) or 96 (K = 128) VGPRs, read once with 16-B loads straight from the [n_pad][3][k] packing (lane l: cout l & 31,
//     k = 16 q + 8 (l >> 5) .. + 7 of step q -- the operand layout is the packing's own byte order).
//   * activations: the fp32 A tile [32][K] arrives by LDS-DMA into a ring of two raw buffers, one tile ahead: the DMA of tile i + 1 and the
//     loads of its residual rows are issued before the matrix phase of tile i and stay in flight through its epilogue stores; the wait in
//     front of tile i + 1 leaves those stores (and the residual loads) in flight, so the queue never drains between tiles.
//   * the split is done ONCE per workgroup: after the raw tile has landed the 256 threads split 8 values each into three bf16 planes
//     [piece][32][K] (16-B chunk c of row r at chunk c ^ f(r), f(r) = (r / (128 / K)) & (K / 8 - 1): the 16 lanes of a ds_read_b128 /
//     ds_write_b128 group then cover the 16 slots of the 256-B bank row once); every wave reads its A operands from the planes.
//   * arithmetic: per 16-k step q the six products with i + j <= 2, smallest first, a0 w0 in an accumulator of its own (the rule
//     conv_gemm_f32s.hip measured: the leading accumulator then rounds once per 16 k); k order fixed, tiles independent of each other: the
//     output bits depend neither on the grid nor on the workgroup that computed a tile.
//   * epilogue: conv_epilogue of conv_gemm_common.h (its transpose tile shares the LDS of the bf16 planes, a barrier in between), the
//     lane's scale / shift kept in registers, the residual rows prefetched a tile ahead.
//
// LDS: max(3 x 32 x K x 2, 32 x 132 x 4) + 2 x 32 x K x 4 = 32.5 KB (K = 64) / 56 KB (K = 128): two workgroups per CU.  VGPRs 164 / 226
// (two waves per SIMD at K = 128), no scratch.  Waits: every barrier that publishes DMA'd data has its vmcnt wait written out in front of it
// (lds_dma.h); the counts are exact because every thread of a full tile issues the same number of stores and only the last tile of the walk
// can be partial.  DESIGN.md ("conv_stream_f32s.hip") has the budget table and what hipcc's own waits forced on this file.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bf16_split.h"
#include "conv_gemm_common.h"
#include "gemm_contract.h"
#include "hpe_internal.h"
#include "lds_dma.h"

namespace {

constexpr int SBM = 32, SBN = 128, SNW = 4;  // tile rows, couts of a workgroup, waves

// DUAL: the conv_block form -- no residual; k = 0 .. 63 of a row comes from the dense x [M][lda], k = 64 .. 127 from x2, the block input of a
// stride-1 projection shortcut ([M][Cin], Cin = 64): the same walk with a second A stream (a lane of a DMA instruction reads one or the other)
template <int K, bool DUAL>
__global__ __launch_bounds__(64 * SNW, 2) void conv_stream_f32s_kernel(GemmArgs p, int walkers) {
    constexpr bool RES = !DUAL;                   // the identity-block form has its residual, the dual form has none
    constexpr int NRES = RES ? SBM / (64 * SNW / (SBN / 4)) : 0;  // residual loads per thread and tile
    constexpr int KS = K / 16;                    // MFMA steps over k
    constexpr int CH = K / 8;                     // 16-B bf16 chunks per plane row
    constexpr int RAW_BYTES = SBM * K * 4;        // one raw fp32 tile
    constexpr int PLANE_BYTES = SBM * K * 2;      // one bf16 piece of a tile
    constexpr int EP_BYTES = SBM * (SBN + 4) * 4;  // transpose tile of conv_epilogue
    constexpr int WORK_BYTES = 3 * PLANE_BYTES > EP_BYTES ? 3 * PLANE_BYTES : EP_BYTES;
    constexpr int AP = RAW_BYTES / 1024 / SNW;    // DMA instructions per wave and tile (2 / 4)
    constexpr int UN = SBM * CH / (64 * SNW);     // 8-value units a thread splits per tile (1 / 2)
    constexpr int NPASS = SBM / (64 * SNW / (SBN / 4));  // row stores (and residual vectors) per thread and tile: 4
    static_assert(K == 64 || K == 128, "K = 64 or 128");
    static_assert(!DUAL || K == 128, "dual: two sources of 64");
    static_assert(AP >= 1 && UN >= 1 && NPASS == 4, "tile geometry");  // NPASS = BM / RPP of conv_epilogue: its row stores per thread, which the waits below count

    // two LDS objects on purpose: hipcc orders an LDS store behind every LDS-DMA in flight that may write the same object (a vmcnt(0) in front
    // of the epilogue's transpose stores would drain the ring); the DMA only ever writes raw_lds
    __shared__ __attribute__((aligned(16))) float lds[WORK_BYTES / 4];  // the bf16 planes; the epilogue's transpose tile
    __shared__ __attribute__((aligned(16))) float raw_lds[2 * RAW_BYTES / 4];
    char* const work = reinterpret_cast<char*>(lds);
    char* const raw = reinterpret_cast<char*>(raw_lds);

    // workgroups b, b + 8, ... share an XCD (one L2): there the n_ntiles slices of one walker run side by side and fetch the A tile once
    const int bid = blockIdx.x;
    const int j = bid >> 3;
    const int slice = j % p.n_ntiles;
    const int walker = (j / p.n_ntiles) * 8 + (bid & 7);
    if (walker >= walkers || walker >= p.n_mtiles) return;
    const int n0 = slice * SBN;
    const int cnt = (p.n_mtiles - walker + walkers - 1) / walkers;  // tiles of this walk

    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int hi = lane >> 5;

    // ---- the wave's weights: pieces j of couts n0 + 32 wave + (lane & 31), all of k, as B operands
    bf16x8 wreg[KS][3];
    {
        const __bf16* wsrc = reinterpret_cast<const __bf16*>(p.w) + (size_t)(n0 + 32 * wave + (lane & 31)) * p.ldw + 8 * hi;
#pragma unroll
        for (int q = 0; q < KS; ++q)
#pragma unroll
            for (int pc = 0; pc < 3; ++pc) wreg[q][pc] = *reinterpret_cast<const bf16x8*>(wsrc + pc * p.w_piece + 16 * q);
    }
    const int ncol = n0 + 32 * wave + (lane & 31);
    const float sc0 = p.scale[ncol], sh0 = p.shift[ncol];

    // ---- per-thread constants of the three phases
    // DMA: instruction i of this wave fills raw bytes [(SNW i + wave) * 1024, + 1024), 16-B slot s = (SNW i + wave) * 64 + lane:
    // row s / (K / 4), floats 4 (s % (K / 4)) .. + 3 of it (the raw tile is plain row-major)
    int dma_row[AP], dma_col[AP];
#pragma unroll
    for (int i = 0; i < AP; ++i) {
        const int s = (SNW * i + wave) * 64 + lane;
        dma_row[i] = s / (K / 4);
        dma_col[i] = (s % (K / 4)) * 4;
    }
    // split: unit u = t + 256 j is the 8 values k = 8 c .. + 7 of row r
    int sp_src[UN], sp_dst[UN];
#pragma unroll
    for (int u = 0; u < UN; ++u) {
        const int un = t + 64 * SNW * u;
        const int r = un / CH, c = un % CH;
        sp_src[u] = r * (K * 4) + c * 32;
        sp_dst[u] = r * (K * 2) + ((c ^ ((r / (16 / CH)) & (CH - 1))) << 4);
    }
    // A operands: row lane & 31, chunk 2 q + hi of step q
    const int a_row = (lane & 31) * (K * 2);
    const int a_x = ((lane & 31) / (16 / CH)) & (CH - 1);
    // residual rows of the epilogue: thread t adds to row 8 pass + t / 32, columns n0 + 4 (t % 32) .. + 3
    const int r_row = t >> 5;
    const float* const res_col = RES ? p.res + n0 + (t & 31) * 4 : nullptr;

    auto issue_tile = [&](int m0, int buf, f32x4 (&rnext)[NPASS]) {
        asm volatile("" ::: "memory");
#pragma unroll
        for (int i = 0; i < AP; ++i) {
            int m = m0 + dma_row[i];
            m = m < p.M ? m : p.M - 1;  // tail rows: read a valid row, the store guard drops the result
            const float* src = p.x + ((size_t)m * p.lda + dma_col[i]);
            if (DUAL && dma_col[i] >= 64) src = p.x2 + ((size_t)m * p.Cin + (dma_col[i] - 64));
            dma16(src, raw + buf * RAW_BYTES + (SNW * i + wave) * 1024);
        }
        asm volatile("" ::: "memory");
#pragma unroll
        for (int pass = 0; pass < NRES; ++pass) {
            int m = m0 + pass * 8 + r_row;
            m = m < p.M ? m : p.M - 1;
            rnext[pass] = HPE_RES_LOAD(reinterpret_cast<const f32x4*>(res_col + (size_t)m * p.ldres));
        }
        asm volatile("" ::: "memory");
    };

    // one tile: k-th of the walk, its A in raw buffer buf, its residual rows in rcur; the next tile's go to buffer buf ^ 1 and rnext
    auto tile_step = [&](int k, int buf, f32x4 (&rcur)[NPASS], f32x4 (&rnext)[NPASS]) {
        const int m0 = (walker + k * walkers) * SBM;
        // (the last tile of the walk issues itself again: one path through the loop body, so that the waits hipcc adds for the residual
        // registers count the same operations as the ones written out here; the kernel's last wait takes that DMA in)
        const int m0n = k + 1 < cnt ? m0 + walkers * SBM : m0;
        // A(k) has landed: behind its DMA this wave issued the NRES residual loads of tile k and the NPASS row stores of tile k - 1 (a
        // full tile: tile k exists), which stay in flight.  (k = 0: the prologue waited for everything.)
        wait_counts<NRES + NPASS>();
        bare_barrier();  // ... in every wave; and every wave is through the epilogue of tile k - 1 (the work area is free)
        // The raw tile is read with the LDS instructions written out: behind a C++ load from the object the DMA writes, hipcc waits for every
        // DMA it cannot prove complete -- it does not know that each row store of the epilogue is issued, so it cannot count as the wait above
        // does -- and that is vmcnt(0): the drain this kernel exists to avoid.
        const unsigned rb = (unsigned)(uintptr_t)(const __attribute__((address_space(3))) char*)(raw + buf * RAW_BYTES);
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            f32x4 lo, up;
            asm volatile("ds_read_b128 %0, %2\n\tds_read_b128 %1, %2 offset:16\n\ts_waitcnt lgkmcnt(0)" : "=&v"(lo), "=&v"(up) : "v"(rb + sp_src[u]) : "memory");
            bf16x8 h0, h1, h2;
            bf16_split3_cast<8>([&](int e) { return e < 4 ? lo[e] : up[e - 4]; }, h0, h1, h2);
            *reinterpret_cast<bf16x8*>(work + sp_dst[u]) = h0;
            *reinterpret_cast<bf16x8*>(work + PLANE_BYTES + sp_dst[u]) = h1;
            *reinterpret_cast<bf16x8*>(work + 2 * PLANE_BYTES + sp_dst[u]) = h2;
        }
        lds_barrier();  // the planes are whole, raw buffer buf is free; no DMA was issued since the wait above
        issue_tile(m0n, buf ^ 1, rnext);  // (buffer buf ^ 1 was split a tile ago, two barriers back)

        f32x16 acc[1][1], acx;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[0][0][e] = acx[e] = 0.f;
#pragma unroll
        for (int q = 0; q < KS; ++q) {
            const int off = a_row + (((2 * q + hi) ^ a_x) << 4);
            const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(work + off);
            const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(work + PLANE_BYTES + off);
            const bf16x8 a2 = *reinterpret_cast<const bf16x8*>(work + 2 * PLANE_BYTES + off);
            // cross terms smallest first
            acx = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, wreg[q][0], acx, 0, 0, 0);
            acx = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, wreg[q][1], acx, 0, 0, 0);
            acx = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, wreg[q][2], acx, 0, 0, 0);
            acx = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, wreg[q][0], acx, 0, 0, 0);
            acx = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, wreg[q][1], acx, 0, 0, 0);
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, wreg[q][0], acc[0][0], 0, 0, 0);
        }
        acc[0][0] += acx;
        // every wave has read its operands before the transpose tile overwrites the planes.  The wait names what this wave issued behind the
        // split barrier (AP DMAs + NRES residual loads): the stores of tile k - 1 are done, the next tile stays in flight
        wait_counts<AP + NRES, 0>();
        bare_barrier();
        conv_epilogue<SBM, SBN, 1, SNW, true>(p, lds, acc, m0, n0, t, lane, 0, wave, rcur, RES, sc0, sh0);
    };

    f32x4 ra[NPASS], rb[NPASS];
    issue_tile(walker * SBM, 0, ra);
    wait_counts<0>();  // tile 0 (and the weights) have landed
    for (int k = 0; k < cnt; k += 2) {
        tile_step(k, 0, ra, rb);
        if (k + 1 < cnt) tile_step(k + 1, 1, rb, ra);
    }
    wait_counts<0>();  // the DMA the last tile issued writes this workgroup's LDS: it lands before the wave ends
}

}  // namespace

int hpe_stream_device_cus() {
    static int n = 0;  // of the first device asked about, for the process: the devices of one host are the same part
    if (n == 0) {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) n = v;
        else n = 256;
    }
    return n;
}

bool hpe_stream_f32s_supported(int M, int N, int K) { return M > 0 && (K == 64 || K == 128) && N >= SBN && N % SBN == 0; }

// the dual-source form: two A sources of 64 channels, the second one the input of a stride-1 shortcut on the same map (its rows are the GEMM's rows)
bool hpe_stream_f32s_dual_supported(int M, int N, int K1, int K2, int stride, int Hi, int Ho) {
    return K1 == 64 && K2 == 64 && stride == 1 && Hi == Ho && hpe_stream_f32s_supported(M, N, K1 + K2);
}

hipError_t hpe_launch_stream_f32s(GemmArgs p, int mode, int max_walkers, hipStream_t st) {
    // the clauses of the split-bf16 GEMM (pitches, alignment, the three pieces inside a weight row, w_rows, the dual geometry) + this kernel's own
    if ((mode != GEMM_DENSE && mode != GEMM_DUAL) || gemm_contract(p, mode, TILE_128x128, GEMM_K_F32S) || !hpe_stream_f32s_supported(p.M, p.N, p.K))
        return hipErrorInvalidValue;
    if (mode == GEMM_DENSE ? !p.res : (p.res || !hpe_stream_f32s_dual_supported(p.M, p.N, p.k1_slabs * BK, p.Cin, p.stride, p.Hi, p.Ho) || p.Wi != p.Wo))
        return hipErrorInvalidValue;
    p.n_mtiles = (p.M + SBM - 1) / SBM;
    p.n_ntiles = p.N / SBN;
    p.split_k = 1;
    p.res_prefetch = 1;
    // two workgroups per CU, as many walkers per N-slice as that gives (a multiple of 8: one walker per XCD and round)
    int walkers = 2 * hpe_stream_device_cus() / p.n_ntiles;
    if (max_walkers > 0 && walkers > max_walkers) walkers = max_walkers;
    if (walkers > p.n_mtiles) walkers = p.n_mtiles;
    if (walkers < 1) walkers = 1;
    const int grid = 8 * p.n_ntiles * ((walkers + 7) / 8);
    if (mode == GEMM_DUAL) hipLaunchKernelGGL((conv_stream_f32s_kernel<128, true>), dim3(grid), dim3(64 * SNW), 0, st, p, walkers);
    else if (p.K == 64) hipLaunchKernelGGL((conv_stream_f32s_kernel<64, false>), dim3(grid), dim3(64 * SNW), 0, st, p, walkers);
    else hipLaunchKernelGGL((conv_stream_f32s_kernel<128, false>), dim3(grid), dim3(64 * SNW), 0, st, p, walkers);
    return hipGetLastError();
}
