// stem_fused.hip -- the stem of the Keras ResNet-50 v1 the reference instantiates (src/models.py:35-41 ->
// keras_applications resnet50.py: conv1_pad ZeroPadding2D(3) -> conv1 7x7/2 (+bias) -> bn_conv1 -> ReLU -> pool1_pad
// ZeroPadding2D(1) -> MaxPooling2D(3, strides 2)) as ONE kernel: [B,224,224,3] fp32 images in, [B,56,56,64] out.
// Nothing of the 112x112x64 conv1 map (0.82 GB at B = 256 in fp32) ever reaches HBM, and there is no separate pad pass.
//
// A workgroup (8 waves) owns one strip of an image: R pooled rows = 2R (+1 halo) conv rows.  It stages the 4R+7 padded
// input rows it needs in LDS once (zero borders written here: that IS conv1_pad) and then runs an implicit GEMM whose A
// operand is read straight from that LDS image -- no per-slab global traffic at all -- against weights held in registers:
//   bf16:  v_mfma_f32_16x16x32_bf16 (M = 112 = 7 x 16 conv pixels of a row: no padding rows); the LDS image is bf16 with the
//          channel padded 3 -> 4, so one kernel row of a pixel pair is one aligned ds_read_b128 and one MFMA k-step is one
//          kernel row (8 px x 4 ch = 32 k); the matrix pipe is idle most of the time anyway -- this variant is bound by the
//          image read and the LDS traffic.
//   fp32:  the same k enumeration on the same instruction, image and weights each split exactly into three bf16 pieces and six
//          products per step (see the fp32 section); a strip taller than 4 pooled rows is walked in passes that restage LDS.
// A workgroup has 8 waves: wave w owns output channels 16 (w & 3) .. + 15 and the conv pixels 0-63 (w < 4: 4 blocks of 16) or
// 64-111 (w >= 4: 3 blocks) of a conv row pair; the two waves that share a SIMD cover each other's LDS latency (one wave per SIMD
// ran the fp32 MFMA loop this file had before the split at 66 % of the matrix rate).  The conv rows 2py and 2py+1 of pooled row py sit in the same lanes / register slots as row 2py-1 kept from the previous
// iteration, so the vertical 3-max is register-wise; the maximum goes through one LDS buffer for the horizontal 3-max
// (stride 2) and leaves as full NHWC rows.  ReLU output is >= 0, so pool1_pad's zeros never win and are not materialised.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hpe_ctx.h"
#include "hpe_internal.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

constexpr int IMG = 224;        // input side
constexpr int CONV = 112;       // conv1 output side
constexpr int POOL = 56;        // pooled output side
constexpr int NCH = 64;         // conv1 output channels
constexpr int PITCH_B = 464;    // bf16 image row in LDS, in floats: 232 px x 4 ch x 2 B = 1856 B
constexpr int VP = 68;          // V buffer row pitch in floats (64 channels + 4: the 4 lane groups of a store hit 4 bank sets)

struct StemArgs {
    const float* img;    // [B,224,224,3] fp32
    const void* w;       // bf16 [64][7][32] (kh, then 8 px x 4 ch);  fp32: its three bf16 pieces, [3][64][7][32]
    const float* scale;  // [64] folded BN
    const float* shift;
    void* y;             // [B,56,56,64] fp32 or bf16
    int B, R, strips;    // pooled rows per strip, strips per image (R * strips == 56)
};

// horizontal 3-max (stride 2, left pad = 0 which never wins after ReLU) of the V buffer -> one pooled NHWC row
template <bool BF16>
__device__ __forceinline__ void pool_store(const float* sV, void* y, int b, int py, int t) {
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int idx = t + 512 * it;
        if (idx < POOL * 16) {
            const int px = idx >> 4;
            const int c = (idx & 15) * 4;
            f32x4 m = *reinterpret_cast<const f32x4*>(sV + (2 * px) * VP + c);
            const f32x4 r = *reinterpret_cast<const f32x4*>(sV + (2 * px + 1) * VP + c);
            m.x = fmaxf(m.x, r.x);
            m.y = fmaxf(m.y, r.y);
            m.z = fmaxf(m.z, r.z);
            m.w = fmaxf(m.w, r.w);
            if (px > 0) {
                const f32x4 l = *reinterpret_cast<const f32x4*>(sV + (2 * px - 1) * VP + c);
                m.x = fmaxf(m.x, l.x);
                m.y = fmaxf(m.y, l.y);
                m.z = fmaxf(m.z, l.z);
                m.w = fmaxf(m.w, l.w);
            }
            const size_t o = (((size_t)b * POOL + py) * POOL + px) * NCH + c;
            if (BF16) {
                bf16x4 v;
                v[0] = (__bf16)m.x;
                v[1] = (__bf16)m.y;
                v[2] = (__bf16)m.z;
                v[3] = (__bf16)m.w;
                *reinterpret_cast<bf16x4*>(reinterpret_cast<__bf16*>(y) + o) = v;
            } else {
                *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(y) + o) = m;
            }
        }
    }
}

// BN + ReLU of the row pair in acc, vertical 3-max with the row kept from the previous iteration, V -> LDS.
// PAIR == false: only acc[1] holds a conv row (the halo row 2 r0 - 1): it just becomes `prev`.
template <bool PAIR, int RB0, int NRB>
__device__ __forceinline__ void bn_relu_vmax(f32x4 (&acc)[2][NRB], f32x4 (&prev)[NRB], float sc, float sh, float* sV, int lane, int wave) {
    const int m = lane & 15, g = lane >> 4;
#pragma unroll
    for (int rb = 0; rb < NRB; ++rb) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float v1 = fmaxf(acc[1][rb][i] * sc + sh, 0.f);
            if (PAIR) {
                const float v0 = fmaxf(acc[0][rb][i] * sc + sh, 0.f);
                const float v = fmaxf(fmaxf(prev[rb][i], v0), v1);
                sV[(16 * (RB0 + rb) + 4 * g + i) * VP + 16 * (wave & 3) + m] = v;  // C layout of the 16x16 MFMA: col = lane & 15, row = 4 (lane >> 4) + i
            }
            prev[rb][i] = v1;
        }
    }
}

// The same, one conv row at a time (the split kernel).  STEP 0: the halo row 2 r0 - 1, it just becomes `prev`; STEP 1: row 2 py,
// `prev` becomes the maximum of the two; STEP 2: row 2 py + 1 completes the vertical 3-max, V -> LDS, and becomes `prev`.
template <int STEP, int RB0, int NRB>
__device__ __forceinline__ void bn_relu_row(f32x4 (&acc)[NRB], f32x4 (&prev)[NRB], float sc, float sh, float* sV, int lane, int wave) {
    const int m = lane & 15, g = lane >> 4;
#pragma unroll
    for (int rb = 0; rb < NRB; ++rb) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float v = fmaxf(acc[rb][i] * sc + sh, 0.f);
            if (STEP == 2) sV[(16 * (RB0 + rb) + 4 * g + i) * VP + 16 * (wave & 3) + m] = fmaxf(prev[rb][i], v);
            prev[rb][i] = STEP == 1 ? fmaxf(prev[rb][i], v) : v;
        }
    }
}

// --------------------------------------------------------------------------------------------------------- fp32 (split)
// The fp32 stem on the bf16 matrix cores (v_mfma_f32_16x16x4_f32 runs at 1/16 of the bf16 rate): image and weights as three bf16
// pieces each, x = x0 + x1 + x2 exactly (bf16_split3; bf16_split.h), the six products a_i w_j with i + j <= 2 in the bf16 kernel's k enumeration
// (one kernel row of 8 px x 4 ch per MFMA) -- 7 x 6 x 16 = 672 cycles per 16 x 16 block of a conv row against 40 x 32 = 1280.
//   * the image is split ONCE, while it is staged: three bf16 planes per staged row, each in the bf16 kernel's layout
//     ([232 px][4 ch], borders and pad channel exactly zero), PITCH_S floats per row; a fragment is one ds_read_b128 per piece.
//   * the weights arrive split (pack_stem_weights / repack_stem_kernel): bf16 [3][64][7][32], 84 VGPRs per lane.
//   * a0 w0 goes into one accumulator, the five cross terms (smallest first) into a second one; they are added once per conv row,
//     before BN (the order conv_gemm_f32s.hip proved).
//   * three planes of 4 R + 7 rows do not fit in LDS for R > 4, so a workgroup walks its strip in passes of at most PASS pooled
//     rows: 23 staged rows (128,064 B) + the V buffer = 158,528 B.  `prev` (the last conv row after BN and ReLU) stays in registers
//     across passes, so no conv row is computed twice inside a strip; a pass restages 4 PASS + 7 rows from the same relative origin
//     as the first one (the two rows above its first window are not read).  The global loads of the next pass are issued before
//     the MFMA work of the current one and written to LDS after the barrier that retires it.
constexpr int PITCH_S = 3 * PITCH_B;                           // floats per staged row: three bf16 planes
constexpr int PASS = 4;                                        // pooled rows per pass
constexpr int STAGE_ROWS = 4 * PASS + 7;                       // staged rows of a full pass
constexpr int STAGE_IT = (STAGE_ROWS * (IMG / 4) + 511) / 512;  // 4-pixel groups per thread

typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));

struct StageGroup {
    f32x4 v0, v1, v2;  // 4 raw pixels (12 floats)
};

// group idx (staged row idx / 56, pixels 4 (idx % 56) ..) of raw rows 4 py0 - 5 .. + rows - 1 of image img4 into registers; rows
// outside the picture are conv1_pad's zeros
__device__ __forceinline__ StageGroup stage_load(const f32x4* img4, int py0, int rows, int idx) {
    const int sr = idx / (IMG / 4);
    const int u = idx - sr * (IMG / 4);
    const int raw = 4 * py0 - 5 + sr;
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    StageGroup s = {z, z, z};
    if (sr < rows && (unsigned)raw < (unsigned)IMG) {
        const f32x4* src = img4 + raw * (IMG * 3 / 4) + 3 * u;
        s.v0 = src[0];
        s.v1 = src[1];
        s.v2 = src[2];
    }
    return s;
}

// ... split and written as three planes: raw pixel 4u + i = padded column 4u + 3 + i, 8 B per pixel and piece
__device__ __forceinline__ void stage_store(const StageGroup& s, float* sIn, int rows, int idx) {
    const int sr = idx / (IMG / 4);
    const int u = idx - sr * (IMG / 4);
    if (sr >= rows) return;
    const float px[12] = {s.v0.x, s.v0.y, s.v0.z, s.v0.w, s.v1.x, s.v1.y, s.v1.z, s.v1.w, s.v2.x, s.v2.y, s.v2.z, s.v2.w};
    unsigned short* dst = reinterpret_cast<unsigned short*>(sIn + (size_t)sr * PITCH_S) + (4 * u + 3) * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        unsigned short h0[3], h1[3], h2[3];
        bf16_split3(px[3 * i], h0);
        bf16_split3(px[3 * i + 1], h1);
        bf16_split3(px[3 * i + 2], h2);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const u16x4 o = {h0[j], h1[j], h2[j], 0};
            *reinterpret_cast<u16x4*>(dst + j * (2 * PITCH_B) + 4 * i) = o;
        }
    }
}

// a wave: conv pixels 16 RB0 .. 16 (RB0 + NRB) - 1 of every conv row, channels 16 (wave & 3) .. + 15
template <int RB0, int NRB>
__device__ __forceinline__ void stem_rows_f32s(const StemArgs& p, float* sIn, float* sV, int b, int r0, int t, int lane, int wave) {
    const int m = lane & 15, g = lane >> 4;
    const int ch = 16 * (wave & 3) + m;
    // ---- weights: piece j of lane (col = m, pixel pair g), kernel row kh: the 8 values of pixels 2g, 2g + 1 (4 ch each)
    bf16x8 wb[3][7];
    {
        const bf16x8* wrow = reinterpret_cast<const bf16x8*>(p.w) + (size_t)ch * 28 + g;
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int kh = 0; kh < 7; ++kh) wb[j][kh] = wrow[j * (NCH * 28) + 4 * kh];
    }
    const float sc = p.scale[ch], sh = p.shift[ch];
    // pixel wo = 16 rb + m, pixel pair g: 16 B at padded column 2 wo + 2 g of a plane
    const float* abase = sIn + 4 * (16 * RB0 + m + g);

    f32x4 acc[NRB], acx[NRB], prev[NRB];  // a0 w0 / the cross terms
#pragma unroll
    for (int rb = 0; rb < NRB; ++rb) prev[rb] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // conv row hl (local: conv row 2 py0 - 1 + hl of the pass that starts at pooled row py0) reads staged rows 2 hl .. 2 hl + 6.
    // One conv row at a time: the two rows of a pooled row together would hold 64 accumulator registers, and the staged loads of
    // the next pass then no longer fit next to the weights.
    auto conv_row = [&](int hl) {
#pragma unroll
        for (int rb = 0; rb < NRB; ++rb) acc[rb] = acx[rb] = (f32x4){0.f, 0.f, 0.f, 0.f};
        const float* a0 = abase + (2 * hl) * PITCH_S;
#pragma unroll
        for (int kh = 0; kh < 7; ++kh) {
            bf16x8 a[3][NRB];
#pragma unroll
            for (int j = 0; j < 3; ++j)
#pragma unroll
                for (int rb = 0; rb < NRB; ++rb) a[j][rb] = *reinterpret_cast<const bf16x8*>(a0 + kh * PITCH_S + j * PITCH_B + rb * 64);
            // cross terms smallest first; consecutive MFMAs go to different accumulators
#pragma unroll
            for (int rb = 0; rb < NRB; ++rb) acx[rb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[2][rb], wb[0][kh], acx[rb], 0, 0, 0);
#pragma unroll
            for (int rb = 0; rb < NRB; ++rb) acx[rb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0][rb], wb[2][kh], acx[rb], 0, 0, 0);
#pragma unroll
            for (int rb = 0; rb < NRB; ++rb) acx[rb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1][rb], wb[1][kh], acx[rb], 0, 0, 0);
#pragma unroll
            for (int rb = 0; rb < NRB; ++rb) acx[rb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1][rb], wb[0][kh], acx[rb], 0, 0, 0);
#pragma unroll
            for (int rb = 0; rb < NRB; ++rb) acx[rb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0][rb], wb[1][kh], acx[rb], 0, 0, 0);
#pragma unroll
            for (int rb = 0; rb < NRB; ++rb) acc[rb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0][rb], wb[0][kh], acc[rb], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);  // keep the scheduler from hoisting the fragment reads of every kernel row to the top
        }
#pragma unroll
        for (int rb = 0; rb < NRB; ++rb) acc[rb] += acx[rb];
    };

    const int rows = 4 * (p.R < PASS ? p.R : PASS) + 7;
    const f32x4* img4 = reinterpret_cast<const f32x4*>(p.img) + (size_t)b * IMG * (IMG * 3 / 4);
    static_assert(STAGE_IT == 3, "three groups per thread");
    StageGroup s0 = stage_load(img4, r0, rows, t), s1 = stage_load(img4, r0, rows, t + 512), s2 = stage_load(img4, r0, rows, t + 1024);
    {  // zero the planes once: the borders and the pad channel are never written again
        const int total = rows * (PITCH_S / 4);
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        for (int idx = t; idx < total; idx += 512) reinterpret_cast<f32x4*>(sIn)[idx] = z;
    }
    __syncthreads();
    stage_store(s0, sIn, rows, t), stage_store(s1, sIn, rows, t + 512), stage_store(s2, sIn, rows, t + 1024);
    __syncthreads();

    for (int q0 = 0; q0 < p.R; q0 += PASS) {
        const int py0 = r0 + q0;
        const int n = p.R - q0 < PASS ? p.R - q0 : PASS;
        const bool more = q0 + PASS < p.R;
        if (more) {
            s0 = stage_load(img4, py0 + PASS, rows, t);
            s1 = stage_load(img4, py0 + PASS, rows, t + 512);
            s2 = stage_load(img4, py0 + PASS, rows, t + 1024);
        }
        if (q0 == 0 && r0 > 0) {  // halo: conv row 2 r0 - 1 (local 0) becomes `prev` (for r0 == 0 it is pool1_pad's zero row)
            conv_row(0);
            bn_relu_row<0, RB0, NRB>(acc, prev, sc, sh, sV, lane, wave);
        }
        for (int pyl = 0; pyl < n; ++pyl) {
            conv_row(2 * pyl + 1);  // local rows 2 pyl + 1, 2 pyl + 2 = conv rows 2 py, 2 py + 1
            bn_relu_row<1, RB0, NRB>(acc, prev, sc, sh, sV, lane, wave);
            conv_row(2 * pyl + 2);
            // every wave has read the V buffer of the previous pooled row (its pool_store ran before these MFMAs, so this barrier
            // finds the others there already) and, once pyl == n - 1, has read the staged rows for the last time
            __syncthreads();
            bn_relu_row<2, RB0, NRB>(acc, prev, sc, sh, sV, lane, wave);
            __syncthreads();
            pool_store<false>(sV, p.y, b, py0 + pyl, t);  // overlaps the next pooled row's MFMAs of the other waves
        }
        if (more) {
            stage_store(s0, sIn, rows, t), stage_store(s1, sIn, rows, t + 512), stage_store(s2, sIn, rows, t + 1024);
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(512) void stem_fused_f32s_kernel(StemArgs p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* sIn = lds;  // [rows][3 pieces][232 px][4 ch] bf16
    float* sV = lds + (4 * (p.R < PASS ? p.R : PASS) + 7) * PITCH_S;

    const int b = blockIdx.x / p.strips;
    const int strip = blockIdx.x - b * p.strips;
    const int r0 = strip * p.R;  // first pooled row of the strip
    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    if (wave < 4)
        stem_rows_f32s<0, 4>(p, sIn, sV, b, r0, t, lane, wave);
    else
        stem_rows_f32s<4, 3>(p, sIn, sV, b, r0, t, lane, wave);
}

// --------------------------------------------------------------------------------------------------------- bf16
template <int RB0, int NRB>
__device__ __forceinline__ void stem_rows_bf16(const StemArgs& p, const float* sIn, float* sV, int b, int r0, int t, int lane, int wave) {
    const int m = lane & 15, g = lane >> 4;
    const int ch = 16 * (wave & 3) + m;
    // ---- weights: lane (col = m, pixel pair g) holds for each kernel row kh the 8 values of pixels 2g, 2g + 1 (4 ch each)
    bf16x8 wb[7];
    {
        const bf16x8* wrow = reinterpret_cast<const bf16x8*>(p.w) + (size_t)ch * 28 + g;
#pragma unroll
        for (int kh = 0; kh < 7; ++kh) wb[kh] = wrow[4 * kh];
    }
    const float sc = p.scale[ch], sh = p.shift[ch];
    // pixel wo = 16 rb + m, pixel pair g: 16 B at padded column 2 wo + 2 g of the staged row
    const float* abase = sIn + 4 * (16 * RB0 + m + g);

    f32x4 acc[2][NRB], prev[NRB];
#pragma unroll
    for (int rb = 0; rb < NRB; ++rb) prev[rb] = (f32x4){0.f, 0.f, 0.f, 0.f};

    auto conv_rows = [&](int hl0, bool both) {
#pragma unroll
        for (int cr = 0; cr < 2; ++cr)
#pragma unroll
            for (int rb = 0; rb < NRB; ++rb) acc[cr][rb] = (f32x4){0.f, 0.f, 0.f, 0.f};
        const float* a0 = abase + (2 * (hl0 + 1)) * PITCH_B;  // staged row of conv row hl0 + 1 (cr = 1)
#pragma unroll
        for (int kh = 0; kh < 7; ++kh) {
#pragma unroll
            for (int cr = 0; cr < 2; ++cr) {
                if (cr == 0 && !both) continue;
#pragma unroll
                for (int rb = 0; rb < NRB; ++rb) {
                    const bf16x8 a = *reinterpret_cast<const bf16x8*>(a0 + (kh + 2 * (cr - 1)) * PITCH_B + rb * 64);
                    acc[cr][rb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, wb[kh], acc[cr][rb], 0, 0, 0);
                }
            }
        }
    };

    if (r0 > 0) {
        conv_rows(-1, false);
        bn_relu_vmax<false, RB0, NRB>(acc, prev, sc, sh, sV, lane, wave);
    }
    for (int pyl = 0; pyl < p.R; ++pyl) {
        conv_rows(2 * pyl + 1, true);
        bn_relu_vmax<true, RB0, NRB>(acc, prev, sc, sh, sV, lane, wave);
        __syncthreads();
        pool_store<true>(sV, p.y, b, r0 + pyl, t);
        __syncthreads();
    }
}

__global__ __launch_bounds__(512, 2) void stem_fused_bf16_kernel(StemArgs p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int rows = 4 * p.R + 7;
    float* sIn = lds;  // bf16 image [rows][232 px][4 ch]
    float* sV = lds + rows * PITCH_B;

    const int b = blockIdx.x / p.strips;
    const int strip = blockIdx.x - b * p.strips;
    const int r0 = strip * p.R;
    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);

    // ---- zero the image (borders + rows outside the picture), then copy: 4 raw pixels (3 aligned float4) -> 4 x 8 B
    {
        const int total = rows * (PITCH_B / 4);
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        for (int idx = t; idx < total; idx += 512) reinterpret_cast<f32x4*>(sIn)[idx] = z;
    }
    __syncthreads();
    {
        const int total = rows * (IMG / 4);
        const f32x4* img4 = reinterpret_cast<const f32x4*>(p.img) + (size_t)b * IMG * (IMG * 3 / 4);
#pragma unroll 4
        for (int idx = t; idx < total; idx += 512) {
            const int s = idx / (IMG / 4);
            const int u = idx - s * (IMG / 4);
            const int raw = 4 * r0 - 5 + s;
            if ((unsigned)raw < (unsigned)IMG) {
                const f32x4* src = img4 + raw * (IMG * 3 / 4) + 3 * u;
                const f32x4 v0 = src[0], v1 = src[1], v2 = src[2];
                const float px[12] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, v2.x, v2.y, v2.z, v2.w};
                // raw pixel 4u + i = padded column 4u + 3 + i, 8 B per pixel
                __bf16* dst = reinterpret_cast<__bf16*>(sIn) + ((size_t)s * 232 + 4 * u + 3) * 4;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    bf16x4 o;
                    o[0] = (__bf16)px[3 * i];
                    o[1] = (__bf16)px[3 * i + 1];
                    o[2] = (__bf16)px[3 * i + 2];
                    o[3] = (__bf16)0.f;
                    *reinterpret_cast<bf16x4*>(dst + 4 * i) = o;
                }
            }
        }
    }
    __syncthreads();
    if (wave < 4)
        stem_rows_bf16<0, 4>(p, sIn, sV, b, r0, t, lane, wave);
    else
        stem_rows_bf16<4, 3>(p, sIn, sV, b, r0, t, lane, wave);
}

}  // namespace

// bf16: the whole strip's 4 R + 7 rows; fp32: three planes of the rows of one pass
size_t hpe_stem_fused_lds_bytes(int R, int bf16) {
    const size_t image = bf16 ? (size_t)(4 * R + 7) * PITCH_B : (size_t)(4 * (R < PASS ? R : PASS) + 7) * PITCH_S;
    return (image + (size_t)CONV * VP) * sizeof(float);
}

// per-device attribute (dynamic LDS above 64 KB); call with the target device current
hipError_t hpe_stem_fused_init_device() {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(stem_fused_f32s_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)hpe_stem_fused_lds_bytes(8, 0));
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(stem_fused_bf16_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)hpe_stem_fused_lds_bytes(8, 1));
}

// pooled rows per strip: 8 (7 strips per image, halo recompute 1/16) once the grid fills the chip several times over,
// smaller strips for small batches (more workgroups, more halo)
int hpe_stem_fused_pick_rows(int B) {
    if (B >= 96) return 8;
    if (B >= 24) return 4;
    if (B >= 6) return 2;
    return 1;
}

hipError_t hpe_launch_stem_fused(const float* img, const void* w, const float* scale, const float* shift, void* y, int B, int R, int bf16,
                                 hipStream_t st) {
    if (!img || !w || !scale || !shift || !y || B < 1 || R < 1 || R > 8 || (POOL % R) != 0) return hipErrorInvalidValue;
    if (((uintptr_t)img & 15) != 0 || ((uintptr_t)y & 15) != 0 || ((uintptr_t)w & 15) != 0) return hipErrorInvalidValue;
    StemArgs p{};
    p.img = img;
    p.w = w;
    p.scale = scale;
    p.shift = shift;
    p.y = y;
    p.B = B;
    p.R = R;
    p.strips = POOL / R;
    const size_t ldsb = hpe_stem_fused_lds_bytes(R, bf16);
    if (bf16)
        hipLaunchKernelGGL(stem_fused_bf16_kernel, dim3(B * p.strips), dim3(512), ldsb, st, p);
    else
        hipLaunchKernelGGL(stem_fused_f32s_kernel, dim3(B * p.strips), dim3(512), ldsb, st, p);
    return hipGetLastError();
}
