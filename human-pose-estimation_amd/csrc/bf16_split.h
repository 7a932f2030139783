// bf16_split.h -- the exact three-piece bf16 split of an fp32 value, and why six products of the pieces are an fp32-exact product.
//
// gfx950 has no xf32: the fp32 MFMA (v_mfma_f32_32x32x2_f32) runs at 1/16 of the bf16 one.  An fp32 value splits EXACTLY into three
// bf16 pieces, each rounded to nearest even:  x0 = bf16(x), x1 = bf16(x - x0), x2 = bf16(x - x0 - x1)  (8 + 8 + 8 significand bits;
// both subtractions are exact, x finite), and the product of two split values is
//     a * w = sum_{i + j <= 2} a_i w_j  +  (a1 w2 + a2 w1 + a2 w2),
// where the dropped terms are below 2^-9 * 2^-18 = 2^-27 of |a w| (the pieces shrink by >= 2^-9 each with round-to-nearest) -- under
// fp32's own rounding of the product.  The six kept products go through v_mfma_f32_32x32x16_bf16 into fp32 accumulators.
// Users: conv_gemm_f32s.hip (A in registers, weights split by the host packer), conv_stream_f32s.hip (A split once per workgroup), conv_stream_chain_f32s.hip (that, and t3 and both weight matrices split in registers), conv_wino.hip (the fused F(2x2) kernel), stem_fused.hip;
// each says which of the six products goes where.  tests/gemm_ref.py, stem_split_ref.py and wino_split_ref.py restate the arithmetic
// in NumPy, separately on purpose.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>

// ---- integer rounding, host and device: what the packers (hpe_finalize.hip), the repack kernel and stem_fused.hip call
__host__ __device__ inline unsigned short f2bf(float f) {  // round-to-nearest-even fp32 -> bf16 (finite inputs)
    unsigned u;
    memcpy(&u, &f, 4);
    return (unsigned short)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}
__host__ __device__ inline float bf2f(unsigned short h) {
    const unsigned u = (unsigned)h << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
// x = h[0] + h[1] + h[2] exactly (finite x): each piece the bf16 nearest to what the pieces before it left
__host__ __device__ inline void bf16_split3(float x, unsigned short h[3]) {
    h[0] = f2bf(x);
    const float r1 = x - bf2f(h[0]);
    h[1] = f2bf(r1);
    const float r2 = r1 - bf2f(h[1]);
    h[2] = f2bf(r2);
}

// ---- the same split through the __bf16 conversions of the device (v_cvt_pk_bf16_f32: round to nearest even), one lane ...
__device__ __forceinline__ void bf16_split3_cast(float x, __bf16& h0, __bf16& h1, __bf16& h2) {
    h0 = (__bf16)x;
    const float r1 = x - (float)h0;
    h1 = (__bf16)r1;
    const float r2 = r1 - (float)h1;
    h2 = (__bf16)r2;
}
// ... and N lanes (4, 8) into three __bf16 vectors: x(e) is lane e of the source
template <int N, typename X, typename V>
__device__ __forceinline__ void bf16_split3_cast(X x, V& h0, V& h1, V& h2) {
#pragma unroll
    for (int e = 0; e < N; ++e) {
        __bf16 b0, b1, b2;
        bf16_split3_cast(x(e), b0, b1, b2);
        h0[e] = b0;
        h1[e] = b1;
        h2[e] = b2;
    }
}
