// augment.hip -- training-batch augmentation (DESIGN.md "Training-batch augmentation"): the reference's DataLoader.image_preprocessing
// (src/data_loader.py:160-213) = jitter_center + jitter_scale + pad_image_edge + tf.slice + random_flip (src/util/data_utils.py:144-238)
// + the [-1,1] normalisations, for a whole batch in ONE launch.  No resized, padded, sliced or reversed intermediate exists: output pixel
// (oy, ox) of the 224 x 224 window reads resized pixel (clamp(cy - 112 + oy), clamp(cx - 112 + ox)) (edge padding = clamping), and that
// pixel is tf.image.resize's bilinear value (half-pixel centres, no antialiasing) of four uint8 taps.  The kernel is bound by its output
// writes (803 KB per image); the taps are byte gathers inside a small window that the L2 serves.
//
// The arithmetic is float32 in the reference's operation order and the compiler must not fuse or reorder it: every function that
// computes a coordinate, a weight or a value runs under `#pragma clang fp contract(off)`; the one fused multiply-add, the resize's source
// coordinate, is written out as __fmaf_rn.  Nothing here is shared with prepost.hip, which restates
// OpenCV's 8-bit fixed-point rule: a different rule, whose bits must not move.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "hpe_ctx.h"

namespace {

constexpr int AUG_S = 224;                                           // output side
constexpr int AUG_RUN = 4;                                           // adjacent output pixels per thread: 3 float4 image stores, 1 float4 mask store
constexpr int AUG_THREADS = 256;
constexpr int AUG_PIX_BLOCKS = AUG_S * AUG_S / AUG_RUN / AUG_THREADS;  // 49 blocks per image, block 49 writes the keypoints
constexpr int AUG_KP = 19;
constexpr int AUG_MAX_SIDE = 1 << 20;
static_assert(AUG_PIX_BLOCKS * AUG_THREADS * AUG_RUN == AUG_S * AUG_S, "the pixel blocks tile the image exactly");
static_assert(AUG_S % AUG_RUN == 0, "a run of pixels stays in one row");
static_assert(sizeof(HpeAugmentFrame) == 64, "the table entry is 64 bytes (include/hpe.h, augment.py)");

// flip_image's swap_inds (src/util/data_utils.py:234-235)
__constant__ int c_swap_inds[AUG_KP] = {5, 4, 3, 2, 1, 0, 11, 10, 9, 8, 7, 6, 12, 13, 14, 16, 15, 18, 17};

struct AxisTap {
    int lo, hi;  // source taps
    float w;     // weight of hi
};

// tf.image.resize (bilinear, half_pixel_centers) for destination coordinate o: in = (o + 0.5) * scale - 0.5 as ONE explicit fused
// multiply-add (the form torch's interpolate evaluates, which is what pins this rule), taps max(floor(in), 0) and
// min(ceil(in), src - 1), weight in - floor(in).  The second clamp of each tap is a no-op for every in the rule can produce and only keeps
// a read inside the frame whatever the table holds.
__device__ __forceinline__ AxisTap axis_tap(int o, float scale, int src) {
#pragma clang fp contract(off)
    const float in = __fmaf_rn((float)o + 0.5f, scale, -0.5f);
    const float fl = floorf(in);
    AxisTap t;
    t.lo = min(max((int)fl, 0), src - 1);
    t.hi = max(min((int)ceilf(in), src - 1), 0);
    t.w = in - fl;
    return t;
}

__device__ __forceinline__ float lerp_rn(float a, float b, float w) {
#pragma clang fp contract(off)
    return a + (b - a) * w;
}

// x lerp of the top and of the bottom row, then the y lerp; source values are u8 * float32(1 / 255)
__device__ __forceinline__ float bilinear_u8(unsigned char t0, unsigned char t1, unsigned char b0, unsigned char b1, float wx, float wy) {
#pragma clang fp contract(off)
    const float k = 1.0f / 255.0f;
    const float top = lerp_rn((float)t0 * k, (float)t1 * k, wx);
    const float bot = lerp_rn((float)b0 * k, (float)b1 * k, wx);
    return lerp_rn(top, bot, wy);
}

__device__ __forceinline__ void augment_keypoint(const HpeAugmentFrame& f, const float* __restrict__ kp, float* __restrict__ out, int j) {
#pragma clang fp contract(off)
    const int src = f.flip ? c_swap_inds[j] : j;
    const float x = kp[src * 3], y = kp[src * 3 + 1], vis = kp[src * 3 + 2];
    float xp = (x * f.fx - (float)f.cx) + 112.0f;
    const float yp = (y * f.fy - (float)f.cy) + 112.0f;
    if (f.flip) xp = (224.0f - xp) - 1.0f;
    const float v = vis > 0.0f ? 1.0f : 0.0f;
    out[j * 3] = v * (2.0f * (xp / 224.0f) - 1.0f);
    out[j * 3 + 1] = v * (2.0f * (yp / 224.0f) - 1.0f);
    out[j * 3 + 2] = v * v;
}

// grid (AUG_PIX_BLOCKS + 1, B): blocks [0, 49) of column b write images[b] and seg[b], AUG_RUN adjacent pixels per thread; block 49 writes
// kp_out[b].  The frame geometry comes from table[b].
__global__ __launch_bounds__(AUG_THREADS) void augment_batch_kernel(const unsigned char* __restrict__ frames, const unsigned char* __restrict__ segs,
                                                                    const HpeAugmentFrame* __restrict__ table, const float* __restrict__ kp,
                                                                    float* __restrict__ images, float* __restrict__ seg_out,
                                                                    float* __restrict__ kp_out) {
#pragma clang fp contract(off)
    const int b = blockIdx.y;
    const HpeAugmentFrame f = table[b];
    if (f.H < 1 || f.W < 1 || f.newH < 1 || f.newW < 1) return;  // refused on the host already: no read from such an entry
    if (blockIdx.x == AUG_PIX_BLOCKS) {
        if (threadIdx.x < AUG_KP) augment_keypoint(f, kp + (size_t)b * AUG_KP * 3, kp_out + (size_t)b * AUG_KP * 3, threadIdx.x);
        return;
    }
    const int t = blockIdx.x * AUG_THREADS + threadIdx.x;  // run index in the image, < 224 * 56 by the grid
    const int oy = t / (AUG_S / AUG_RUN), ox0 = (t - oy * (AUG_S / AUG_RUN)) * AUG_RUN;
    const int ry = min(max(f.cy - AUG_S / 2 + oy, 0), f.newH - 1);  // row of the resized image (edge padding = clamp)
    const AxisTap ty = axis_tap(ry, f.ry, f.H);
    const unsigned char* img = frames + f.frame_offset;
    const unsigned char* msk = segs + f.seg_offset;
    const unsigned char* i0 = img + (size_t)ty.lo * f.W * 3;
    const unsigned char* i1 = img + (size_t)ty.hi * f.W * 3;
    const unsigned char* m0 = msk + (size_t)ty.lo * f.W;
    const unsigned char* m1 = msk + (size_t)ty.hi * f.W;
    float o[AUG_RUN * 3], s[AUG_RUN];
#pragma unroll
    for (int p = 0; p < AUG_RUN; ++p) {
        const int ox = ox0 + p;
        const int wx = f.flip ? AUG_S - 1 - ox : ox;  // tf.reverse(axis 1) of the window
        const int rx = min(max(f.cx - AUG_S / 2 + wx, 0), f.newW - 1);
        const AxisTap tx = axis_tap(rx, f.rx, f.W);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = bilinear_u8(i0[tx.lo * 3 + c], i0[tx.hi * 3 + c], i1[tx.lo * 3 + c], i1[tx.hi * 3 + c], tx.w, ty.w);
            o[p * 3 + c] = 2.0f * (v - 0.5f);
        }
        s[p] = bilinear_u8(m0[tx.lo], m0[tx.hi], m1[tx.lo], m1[tx.hi], tx.w, ty.w);
    }
    float4* io = reinterpret_cast<float4*>(images + ((size_t)b * AUG_S * AUG_S + (size_t)t * AUG_RUN) * 3);
    io[0] = make_float4(o[0], o[1], o[2], o[3]);
    io[1] = make_float4(o[4], o[5], o[6], o[7]);
    io[2] = make_float4(o[8], o[9], o[10], o[11]);
    *reinterpret_cast<float4*>(seg_out + (size_t)b * AUG_S * AUG_S + (size_t)t * AUG_RUN) = make_float4(s[0], s[1], s[2], s[3]);
}

bool entry_ok(const HpeAugmentFrame& f) {
    return f.frame_offset >= 0 && f.seg_offset >= 0 && f.H >= 1 && f.W >= 1 && f.newH >= 1 && f.newW >= 1 && f.H <= AUG_MAX_SIDE &&
           f.W <= AUG_MAX_SIDE && f.newH <= AUG_MAX_SIDE && f.newW <= AUG_MAX_SIDE;
}

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int hpe_augment_plan(int B, const int* sizes_hw, const int* centers_xy, const int* trans_xy, const float* scales, const unsigned char* flips,
                     int trans_max, const long long* frame_offsets, const long long* seg_offsets, HpeAugmentFrame* table_out) {
#pragma clang fp contract(off)
    if (!sizes_hw || !centers_xy || !trans_xy || !scales || !flips || !frame_offsets || !seg_offsets || !table_out)
        return fail(HPE_ERR_INVALID, "null argument");
    if (B < 1) return fail(HPE_ERR_INVALID, "B must be >= 1");
    if (trans_max < 0 || trans_max > AUG_MAX_SIDE) return fail(HPE_ERR_INVALID, "trans_max must be in [0, 2^20]");
    const int margin = AUG_S / 2;
    const int margin_safe = margin + trans_max + 50;  // src/data_loader.py:176
    for (int b = 0; b < B; ++b) {
        const std::string at = " (sample " + std::to_string(b) + ")";
        const int H = sizes_hw[2 * b], W = sizes_hw[2 * b + 1];
        if (H < 1 || W < 1 || H > AUG_MAX_SIDE || W > AUG_MAX_SIDE) return fail(HPE_ERR_INVALID, "H and W must be in [1, 2^20]" + at);
        if (frame_offsets[b] < 0 || seg_offsets[b] < 0) return fail(HPE_ERR_INVALID, "negative offset" + at);
        const float scale = scales[b];
        if (!std::isfinite(scale) || !(scale > 0.f)) return fail(HPE_ERR_INVALID, "scale must be finite and positive" + at);
        const long long cxi = (long long)centers_xy[2 * b] + trans_xy[2 * b], cyi = (long long)centers_xy[2 * b + 1] + trans_xy[2 * b + 1];
        if (std::llabs(cxi) > (1LL << 24) || std::llabs(cyi) > (1LL << 24)) return fail(HPE_ERR_INVALID, "jittered centre outside +-2^24" + at);
        // jitter_scale (src/util/data_utils.py:158-172): new_size = int(float(size) * scale), actual_factor = float(new) / float(size)
        const float nhf = (float)H * scale, nwf = (float)W * scale;
        if (!(nhf >= 1.f) || !(nwf >= 1.f) || !(nhf < (float)AUG_MAX_SIDE + 1.f) || !(nwf < (float)AUG_MAX_SIDE + 1.f))
            return fail(HPE_ERR_INVALID, "the scaled frame has a side < 1 or > 2^20" + at);
        HpeAugmentFrame f;
        f.frame_offset = frame_offsets[b];
        f.seg_offset = seg_offsets[b];
        f.H = H;
        f.W = W;
        f.newH = (int)nhf;
        f.newW = (int)nwf;
        f.fy = (float)f.newH / (float)H;
        f.fx = (float)f.newW / (float)W;
        const float cxf = (float)(int)cxi * f.fx, cyf = (float)(int)cyi * f.fy;
        if (!(std::fabs(cxf) < 1073741824.f) || !(std::fabs(cyf) < 1073741824.f))
            return fail(HPE_ERR_INVALID, "scaled centre outside +-2^30" + at);
        f.cx = (int)cxf;
        f.cy = (int)cyf;
        f.flip = flips[b] ? 1 : 0;
        // tf.slice(image_pad, start = c + margin_safe - margin, size 224) succeeds iff the window lies in the padded image
        const long long sx = (long long)f.cx + margin_safe - margin, sy = (long long)f.cy + margin_safe - margin;
        f.inside = sx >= 0 && sy >= 0 && sx + AUG_S <= (long long)f.newW + 2 * margin_safe && sy + AUG_S <= (long long)f.newH + 2 * margin_safe;
        f.rx = (float)W / (float)f.newW;
        f.ry = (float)H / (float)f.newH;
        table_out[b] = f;
    }
    return HPE_OK;
}

int hpe_augment_batch(const unsigned char* frames_dev, const unsigned char* segs_dev, const HpeAugmentFrame* table_host,
                      const HpeAugmentFrame* table_dev, const float* kp_dev, int B, float* images_out, float* seg_out, float* kp_out,
                      void* stream) {
    if (!frames_dev || !segs_dev || !table_host || !table_dev || !kp_dev || !images_out || !seg_out || !kp_out)
        return fail(HPE_ERR_INVALID, "null argument");
    if (B < 1 || B > 65535) return fail(HPE_ERR_INVALID, "B must be in [1, 65535]");
    if (((uintptr_t)images_out | (uintptr_t)seg_out) & 15) return fail(HPE_ERR_INVALID, "images_out and seg_out must be 16-byte aligned");
    for (int b = 0; b < B; ++b)
        if (!entry_ok(table_host[b]))
            return fail(HPE_ERR_INVALID, "table entry " + std::to_string(b) + ": sizes must be in [1, 2^20] and offsets >= 0");
    hipLaunchKernelGGL(augment_batch_kernel, dim3(AUG_PIX_BLOCKS + 1, B), dim3(AUG_THREADS), 0, static_cast<hipStream_t>(stream), frames_dev,
                       segs_dev, table_dev, kp_dev, images_out, seg_out, kp_out);
    HIP_TRY(hipGetLastError());
    return HPE_OK;
}

}  // extern "C"
#pragma GCC visibility pop
