// conv_stream_chain_f32s.hip -- the chained forms of conv_stream_f32s.hip: the expand 1x1 of a stage-2 block and the reduce 1x1 of the NEXT block
// in one persistent launch, both GEMMs on the bf16 matrix cores, fp32-exact (bf16_split.h):
//
//     t3 = relu(bn2c(W2c . t2) + x)                 form 3, the identity chain (res2b -> res2c): K = 64, residual x [M][256]
//     t3 = relu([s2c W2c | s1 W1] . [t2 | x] + sh)  form 4, the conv_block chain (res2a -> res2b): K = 64 + 64, folded weights, x [M][64]
//     u1 = relu(bn2a'(W2a' . t3))                   both: K = 256, N = 64
//
// t3 is written once and never read back; u1 leaves NHWC or channel-slab-8 major (what the fused Winograd 3x3 of the next block reads).
//
//   * a workgroup (8 waves, one per CU) owns all 256 couts of a 32-row tile and walks the tiles walker, walker + walkers, ...; wave w owns
//     couts 32 w .. 32 w + 31 of the expand and the SAME 32 channels as its k-slice of the reduce.
//   * activations as in conv_stream_f32s.hip: the raw fp32 tile [32][K] by LDS-DMA into a ring of two, one tile ahead; one split per
//     workgroup into three bf16 planes (same chunk swizzle); the residual rows prefetched a tile ahead.
//   * the expand runs TRANSPOSED (weights = MFMA A operand, pixels = B; the 32x32 operand layouts are symmetric): a lane then holds pixel
//     lane & 31 and the 16 couts 8 j + 4 hi + i (j, i = 0..3, hi = lane >> 5) of its wave -- scale / shift, residual, ReLU happen in
//     registers.  t3 then goes through an LDS tile and leaves by whole rows, a wave-instruction per pixel, behind the tile's last barrier:
//     stored straight from the accumulator layout (16 B per lane, 64 lines an instruction) it took 0.48 of 0.87 ms at B = 256.
//   * the reduce takes the wave's t3 block straight from those registers: its 16 values per lane are split in place and are the B operand
//     of 2 k-steps x 2 cout blocks; slot t of k-step s on lane half hi stands for channel 16 s + 8 (t >> 2) + 4 hi + (t & 3) of the wave's
//     32 -- the accumulator's own register order -- and the reduce weights are loaded in that order (chain_k below).  No t3 is read
//     back from LDS for it.  Each wave ends with a 32 x 64 partial u1; the eight partials are summed through LDS in wave order, then bn / ReLU.
//   * weights: both matrices are read ONCE per workgroup from the layers' fp32 weights (L.w / L.w_dual: what every other fp32 kernel and the
//     device-side update already keep) and split in registers with the same round-to-nearest-even split as the activations -- 64 or 96
//     values per lane and launch, against 49 or 98 tiles of work; so these forms need no weight image of their own.
//   * arithmetic of BOTH GEMMs: per 16-k step the six products with i + j <= 2, smallest first, a0 w0 in an accumulator of its own; fixed k
//     order, fixed wave order of the partial sums, tiles independent: the output bits depend neither on the grid nor on the walker count.
//
// Whole tiles only (stage 2: 3136 = 98 x 32 rows per image): every thread issues the same vector-memory operations per tile, which the counted
// vmcnt waits rely on; the launcher refuses any other M.  LDS: planes 12 / 24 KB + partial sums 64 KB + t3 tile 32 KB + ring 16 / 32 KB = 124.5 / 152.5 KB.  DESIGN.md
// ("conv_stream_f32s.hip -- chained forms") has the register report and the measurements.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bf16_split.h"
#include "conv_gemm_common.h"
#include "hpe_internal.h"
#include "lds_dma.h"

namespace {

constexpr int CBM = 32, CNW = 8, CN4 = 256, CNP = 64;  // tile rows, waves, expand couts, reduce couts

// channel (of the wave's 32) behind slot t of k-step s of the reduce on lane half hi: the register order of a transposed 32x32 accumulator
constexpr int chain_k(int s, int hi, int t) { return 16 * s + 8 * (t >> 2) + 4 * hi + (t & 3); }

// the three bf16 pieces of 8 floats (two 16-B vectors) as one MFMA operand each
__device__ __forceinline__ void split8(const f32x4& lo, const f32x4& up, bf16x8& h0, bf16x8& h1, bf16x8& h2) {
    bf16_split3_cast<8>([&](int e) { return e < 4 ? lo[e] : up[e - 4]; }, h0, h1, h2);
}

// the six products of one 16-k step: cross terms smallest first into x, a0 w0 into its own accumulator
__device__ __forceinline__ void six(const bf16x8 (&w)[3], const bf16x8& b0, const bf16x8& b1, const bf16x8& b2, f32x16& acc, f32x16& x) {
    x = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[0], b2, x, 0, 0, 0);
    x = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[1], b1, x, 0, 0, 0);
    x = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[2], b0, x, 0, 0, 0);
    x = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[0], b1, x, 0, 0, 0);
    x = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[1], b0, x, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[0], b0, acc, 0, 0, 0);
}

template <int K, bool DUAL>
__global__ __launch_bounds__(64 * CNW, 2) void conv_stream_chain_f32s_kernel(StreamChainArgs p, int walkers) {
    constexpr int NRES = DUAL ? 0 : 4;           // residual loads per thread and tile
    constexpr int NST = 4;                       // t3 stores per thread and tile (+ one u1 store)
    constexpr int KS = K / 16;                   // MFMA steps of the expand
    constexpr int CH = K / 8;                    // 16-B bf16 chunks per plane row
    constexpr int RAW_BYTES = CBM * K * 4;       // one raw fp32 tile
    constexpr int PLANE_BYTES = CBM * K * 2;     // one bf16 piece of a tile
    constexpr int PART_BYTES = CBM * CNP * 4;    // one wave's partial u1
    constexpr int STAGE_BYTES = CBM * CN4 * 4;   // the t3 tile on its way out
    constexpr int AP = RAW_BYTES / 1024 / CNW;   // DMA instructions per wave and tile (1 / 2)
    constexpr int UNITS = CBM * CH;              // 8-value units of the split: one per thread of the first 256 (K = 64) / of all 512
    static_assert((K == 64 && !DUAL) || (K == 128 && DUAL), "identity chain: K = 64; conv_block chain: K = 64 + 64");
    static_assert(AP >= 1 && UNITS <= 64 * CNW && UNITS % 64 == 0, "tile geometry");

    // two LDS objects, as in conv_stream_f32s.hip: the DMA only ever writes raw_lds, so no LDS store to lds waits for the ring
    __shared__ __attribute__((aligned(16))) float lds[(3 * PLANE_BYTES + CNW * PART_BYTES + STAGE_BYTES) / 4 + 2 * CNP];  // the bf16 planes | the eight partial sums | the t3 tile | scaleB, shiftB
    __shared__ __attribute__((aligned(16))) float raw_lds[2 * RAW_BYTES / 4];
    char* const work = reinterpret_cast<char*>(lds);
    char* const part = work + 3 * PLANE_BYTES;
    char* const raw = reinterpret_cast<char*>(raw_lds);
    char* const stage = part + CNW * PART_BYTES;
    float* const bnB = reinterpret_cast<float*>(stage + STAGE_BYTES);

    const int walker = blockIdx.x;
    const int n_mtiles = p.M / CBM;
    if (walker >= walkers || walker >= n_mtiles) return;
    const int cnt = (n_mtiles - walker + walkers - 1) / walkers;  // tiles of this walk

    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int hi = lane >> 5;
    const int px = lane & 31;

    // ---- the wave's weights, split here: expand couts 32 wave + px, all of k (A operands); reduce couts 32 nb + px, the wave's 32 channels in
    // accumulator order (chain_k: two 4-float runs 8 apart per lane and k-step)
    bf16x8 wexp[KS][3], wred[2][2][3];
    {
        const float* wa = p.wA + (size_t)(32 * wave + px) * p.ldwA + 8 * hi;
#pragma unroll
        for (int q = 0; q < KS; ++q) {
            split8(*reinterpret_cast<const f32x4*>(wa + 16 * q), *reinterpret_cast<const f32x4*>(wa + 16 * q + 4), wexp[q][0], wexp[q][1], wexp[q][2]);
            if (q % 4 == 3) asm volatile("" ::: "memory");  // (four steps' loads in flight at a time: the raw values of all of them would not fit the registers)
        }
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const float* wb = p.wB + (size_t)(32 * nb + px) * p.ldwB + 32 * wave + chain_k(s, hi, 0);
                static_assert(chain_k(0, 0, 4) - chain_k(0, 0, 0) == 8 && chain_k(1, 1, 0) == 20, "two runs of 4, 8 apart");
                split8(*reinterpret_cast<const f32x4*>(wb), *reinterpret_cast<const f32x4*>(wb + 8), wred[nb][s][0], wred[nb][s][1], wred[nb][s][2]);
            }
    }

    // ---- per-thread constants
    // DMA: instruction i of this wave fills raw bytes [(CNW i + wave) * 1024, + 1024): 16-B slot s, row s / (K / 4), floats 4 (s % (K / 4)) .. + 3
    // (conv_block form: floats 64 .. 127 of a row, slots 16 .. 31 of its 32, are the block input's)
    unsigned dma_off[AP];
#pragma unroll
    for (int i = 0; i < AP; ++i) {
        const int s = (CNW * i + wave) * 64 + lane;
        dma_off[i] = (unsigned)(s / (K / 4)) * 64 + ((s % (K / 4)) * 4 & 63);
    }
    // (the two sources pass through an empty asm: hipcc otherwise selects between the ADDRESSES of the two kernel arguments and loads the
    // pointer per tile, a vector load with a vmcnt(0) behind it)
    const float *src_t2 = p.t2, *src_x = p.x;
    asm volatile("" : "+s"(src_t2), "+s"(src_x));
    const float* const dma_src = (DUAL && (lane & 16)) ? src_x : src_t2;
    // split: unit t is the 8 values k = 8 c .. + 7 of row r (chunk swizzle of conv_stream_f32s.hip)
    const int sp_r = (t % UNITS) / CH, sp_c = t % CH;
    const int sp_src = sp_r * (K * 4) + sp_c * 32;
    const int sp_dst = sp_r * (K * 2) + ((sp_c ^ ((sp_r / (16 / CH)) & (CH - 1))) << 4);
    // B operands of the expand: row px, chunk 2 q + hi of step q
    const int a_row = px * (K * 2);
    const int a_x = (px / (16 / CH)) & (CH - 1);
    // t3 / residual: pixel px, couts 32 wave + 8 j + 4 hi .. + 3
    // (lane offsets are 32-bit beside a wave-uniform tile base: one register each, and the address arithmetic stays scalar)
    const unsigned t3_off = (unsigned)px * CN4 + 32 * wave + 4 * hi;
    // the t3 tile [pixel][256 couts] on its way out: 16-B chunk c of a pixel's 1-KB row at chunk c ^ (pixel & 15) (the 8 lanes of a ds_write_b128
    // group, 8 pixels at one chunk, then fall into 8 slots of a bank row; a wave reads a row back whole)
    // partial sums: [wave][pixel][64 couts], 16-B chunk c of a pixel's 256-B row at chunk c ^ (pixel & 15): the 16 lanes of a
    // ds_write_b128 / ds_read_b128 group cover the 16 slots of the bank row once, in the write and in both read orders below
    // u1: this thread sums pixel ur, couts 4 uc .. + 3.  NHWC: 16 consecutive threads a row; slab-8: 32 consecutive threads the pixels of one half slab
    const int ur = p.u1_slab8 ? (t & 31) : (t >> 4);
    const int uc = p.u1_slab8 ? (((t >> 6) << 1) | ((t >> 5) & 1)) : (t & 15);
    const char* const part_r = part + ur * 256 + ((uc ^ (ur & 15)) << 4);
    const unsigned u1_off = p.u1_slab8 ? ((unsigned)(uc >> 1) * p.M + ur) * 8 + (uc & 1) * 4 : (unsigned)ur * CNP + uc * 4;
    const unsigned u1_tile = p.u1_slab8 ? CBM * 8 : CBM * CNP;  // floats from one tile to the next
    if (t < CNP) bnB[t] = p.scaleB[t], bnB[CNP + t] = p.shiftB[t];  // (published by the first barrier of the walk, read behind the third)
    cfloat_p scp = (cfloat_p)(p.scaleA + 32 * wave);
    cfloat_p shp = (cfloat_p)(p.shiftA + 32 * wave);

    auto issue_tile = [&](int m0, int buf, f32x4 (&rnext)[4]) {
        asm volatile("" ::: "memory");
#pragma unroll
        for (int i = 0; i < AP; ++i) {
            dma16(dma_src + (size_t)m0 * 64 + dma_off[i], raw + buf * RAW_BYTES + (CNW * i + wave) * 1024);
        }
        asm volatile("" ::: "memory");
#pragma unroll
        for (int j = 0; j < NRES; ++j) rnext[j] = HPE_RES_LOAD(reinterpret_cast<const f32x4*>(p.x + (size_t)m0 * CN4 + (t3_off + 8 * j)));
        asm volatile("" ::: "memory");
    };

    // one tile: k-th of the walk, its A in raw buffer buf, its residual in rcur; the next tile's go to buffer buf ^ 1 and rnext
    auto tile_step = [&](int k, int buf, f32x4 (&rcur)[4], f32x4 (&rnext)[4]) {
        const int m0 = (walker + k * walkers) * CBM;
        // (the last tile of the walk issues itself again: one path through the loop body, so that every wait counts the same operations;
        // the kernel's last wait takes that DMA in)
        const int m0n = k + 1 < cnt ? m0 + walkers * CBM : m0;
        // A(k) has landed: behind its DMA this wave issued the NRES residual loads of tile k and the NST + 1 stores of tile k - 1, which stay
        // in flight.  (k = 0: the prologue waited for everything.)
        wait_counts<NRES + NST + 1>();
        bare_barrier();  // ... in every wave; and every wave is through the partial sums of tile k - 1
        if (t < UNITS) {  // (whole waves)
            // the raw tile is read with the LDS instructions written out: behind a C++ load from the object the DMA writes hipcc waits for vmcnt(0)
            const unsigned rb = (unsigned)(uintptr_t)(const __attribute__((address_space(3))) char*)(raw + buf * RAW_BYTES);
            f32x4 lo, up;
            asm volatile("ds_read_b128 %0, %2\n\tds_read_b128 %1, %2 offset:16\n\ts_waitcnt lgkmcnt(0)" : "=&v"(lo), "=&v"(up) : "v"(rb + sp_src) : "memory");
            bf16x8 h0, h1, h2;
            split8(lo, up, h0, h1, h2);
            *reinterpret_cast<bf16x8*>(work + sp_dst) = h0;
            *reinterpret_cast<bf16x8*>(work + PLANE_BYTES + sp_dst) = h1;
            *reinterpret_cast<bf16x8*>(work + 2 * PLANE_BYTES + sp_dst) = h2;
        }
        lds_barrier();  // the planes are whole, raw buffer buf is free; no DMA was issued since the wait above
        issue_tile(m0n, buf ^ 1, rnext);  // (buffer buf ^ 1 was split a tile ago, two barriers back)

        // ---- expand, transposed: acc[cout 8 j + 4 hi + i][pixel px]
        f32x16 acc, acx;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = acx[e] = 0.f;
        // (the operands of step q + 1 are read before the products of step q and no further ahead: the fence keeps hipcc from hoisting every
        // step's reads to the top, which the registers beside the resident weights do not have room for.)
        bf16x8 b[2][3];
        auto read_b = [&](int q, bf16x8 (&d)[3]) {
            const int off = a_row + (((2 * q + hi) ^ a_x) << 4);
#pragma unroll
            for (int pc = 0; pc < 3; ++pc) d[pc] = *reinterpret_cast<const bf16x8*>(work + pc * PLANE_BYTES + off);
        };
        read_b(0, b[0]);
#pragma unroll
        for (int q = 0; q < KS; ++q) {
            if (q + 1 < KS) read_b(q + 1, b[(q + 1) & 1]);
            asm volatile("" ::: "memory");
            six(wexp[q], b[q & 1][0], b[q & 1][1], b[q & 1][2], acc, acx);
        }
        acc += acx;
        // the residual of this tile has landed: it is older than the stores of tile k - 1, which stay in flight with what this wave issued behind
        // the split barrier.  Written out because hipcc's own wait for the residual registers, with a DMA pending, is vmcnt(0): the drain of the ring
        if (!DUAL) wait_counts<AP + NRES + NST + 1>();
        // ---- epilogue in registers (scale / shift through the scalar cache: the address is wave-uniform), t3 out, and the same values split
        // into the reduce's B operands
        // (the pointers pass through an empty asm per tile: scale / shift are then loaded -- s_load -- and selected per tile; hoisted out of the walk
        // as loop invariants the 32 selected values would be 32 more resident registers)
        cfloat_p scq = scp, shq = shp;
        asm volatile("" : "+s"(scq), "+s"(shq));
        // (conv_block form: the lane's rows of the t3 tile and of its partial sum are addressed from px per tile, not kept -- two registers that
        // form, with 96 of expand weights, does not have; the identity form spills if it does the same)
        int pxq = px;
        if (DUAL) asm volatile("" : "+v"(pxq));
        char* const stage_w = stage + pxq * 1024;
        char* const part_w = part + wave * PART_BYTES + pxq * 256;
        bf16x8 tb[2][3];
        float* const t3p = p.t3 + (size_t)m0 * CN4;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            f32x4 o[2];
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) {
                const int j = 2 * s + jj;
                const f32x4 sc_lo = *reinterpret_cast<cf32x4_p>(scq + 8 * j), sc_hi = *reinterpret_cast<cf32x4_p>(scq + 8 * j + 4);
                const f32x4 sh_lo = *reinterpret_cast<cf32x4_p>(shq + 8 * j), sh_hi = *reinterpret_cast<cf32x4_p>(shq + 8 * j + 4);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float v = acc[4 * j + i] * (hi ? sc_hi[i] : sc_lo[i]) + (hi ? sh_hi[i] : sh_lo[i]);
                    if (!DUAL) v += rcur[j][i];
                    o[jj][i] = fmaxf(v, 0.f);
                }
                *reinterpret_cast<f32x4*>(stage_w + (((8 * wave + 2 * j + hi) ^ (px & 15)) << 4)) = o[jj];
            }
            split8(o[0], o[1], tb[s][0], tb[s][1], tb[s][2]);
        }
        // ---- reduce, transposed, over the wave's 32 channels: one 32-cout block at a time, its partial sum to LDS
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            f32x16 r, rx;
#pragma unroll
            for (int e = 0; e < 16; ++e) r[e] = rx[e] = 0.f;
#pragma unroll
            for (int s = 0; s < 2; ++s) six(wred[nb][s], tb[s][0], tb[s][1], tb[s][2], r, rx);
            r += rx;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                f32x4 v;
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = r[4 * j + i];
                *reinterpret_cast<f32x4*>(part_w + (((8 * nb + 2 * j + hi) ^ (px & 15)) << 4)) = v;
            }
        }
        // the eight partial sums and the t3 tile are whole.  (The wait names more than is in flight behind the stores of tile k - 1: no
        // vector-memory operation is waited for)
        wait_counts<AP + NRES + NST + 1, 0>();
        bare_barrier();
        // t3 leaves by rows: a wave-instruction stores one pixel's 1 KB (lane-per-pixel stores of 16 B, 64 lines an instruction, took 0.48 of
        // the 0.87 ms of the launch at B = 256)
#pragma unroll
        for (int i = 0; i < NST; ++i) {
            const int r = 8 * i + wave;
            const f32x4 v = *reinterpret_cast<const f32x4*>(stage + r * 1024 + ((lane ^ (r & 15)) << 4));
            __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(t3p + (r * CN4 + 4 * lane)));
        }
        f32x4 u = *reinterpret_cast<const f32x4*>(part_r);
#pragma unroll
        for (int w = 1; w < CNW; ++w) u += *reinterpret_cast<const f32x4*>(part_r + w * PART_BYTES);  // wave order
        const f32x4 scB = *reinterpret_cast<const f32x4*>(bnB + 4 * uc), shB = *reinterpret_cast<const f32x4*>(bnB + CNP + 4 * uc);
#pragma unroll
        for (int i = 0; i < 4; ++i) u[i] = fmaxf(u[i] * scB[i] + shB[i], 0.f);
        *reinterpret_cast<f32x4*>(p.u1 + (size_t)(m0 / CBM) * u1_tile + u1_off) = u;
    };

    f32x4 ra[4], rb[4];
    issue_tile(walker * CBM, 0, ra);
    wait_counts<0>();  // tile 0 (and the weights) have landed
    for (int k = 0; k < cnt; k += 2) {
        tile_step(k, 0, ra, rb);
        if (k + 1 < cnt) tile_step(k + 1, 1, rb, ra);
    }
    wait_counts<0>();  // the DMA the last tile issued writes this workgroup's LDS: it lands before the wave ends
}

}  // namespace

// C / C4 / CP: channels of t2, t3 and u1; C2: channels of the block input in the conv_block form, 0 in the identity form
bool hpe_stream_chain_f32s_supported(int M, int C, int C4, int CP, int C2) {
    return M > 0 && M % CBM == 0 && C == 64 && C4 == CN4 && CP == CNP && (C2 == 0 || C2 == 64);
}

hipError_t hpe_launch_stream_chain_f32s(const StreamChainArgs& p, int C, int C4, int CP, int C2, int max_walkers, hipStream_t st) {
    if (!hpe_stream_chain_f32s_supported(p.M, C, C4, CP, C2)) return hipErrorInvalidValue;
    if (!p.t2 || !p.x || !p.wA || !p.wB || !p.t3 || !p.u1 || !p.scaleA || !p.shiftA || !p.scaleB || !p.shiftB) return hipErrorInvalidValue;
    if (p.ldwA < C + C2 || p.ldwB < C4 || (p.ldwA % 4) != 0 || (p.ldwB % 4) != 0) return hipErrorInvalidValue;
    if ((((uintptr_t)p.t2 | (uintptr_t)p.x | (uintptr_t)p.wA | (uintptr_t)p.wB | (uintptr_t)p.t3 | (uintptr_t)p.u1 | (uintptr_t)p.scaleA | (uintptr_t)p.shiftA |
          (uintptr_t)p.scaleB | (uintptr_t)p.shiftB) & 15) != 0)
        return hipErrorInvalidValue;
    // one workgroup per CU (its LDS and its 8 waves of 256 registers fill one)
    int walkers = hpe_stream_device_cus();
    if (max_walkers > 0 && walkers > max_walkers) walkers = max_walkers;
    if (walkers > p.M / CBM) walkers = p.M / CBM;
    if (C2) hipLaunchKernelGGL((conv_stream_chain_f32s_kernel<128, true>), dim3(walkers), dim3(64 * CNW), 0, st, p, walkers);
    else hipLaunchKernelGGL((conv_stream_chain_f32s_kernel<64, false>), dim3(walkers), dim3(64 * CNW), 0, st, p, walkers);
    return hipGetLastError();
}
