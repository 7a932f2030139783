// draw.hip -- the drawing half of the training summaries (DESIGN.md "Training summaries"): the reference's draw_skeleton
// (src/util/renderer.py:286-447, cv2 circles and lines) and the panel of visualize_img / draw_results (src/trainer.py:622-679) on the
// device, in GATHER form: the paint calls of a drawing become a list of primitives in LDS, built per workgroup from the joints, and
// every pixel walks that list BACKWARDS and takes the colour of the first primitive that covers it -- the last paint wins, as in the
// reference, without any pixel being written twice and without atomics.
//
// The raster rules are this project's own (cv2 is the reference's; PARITY UNPINNED), in exact integer arithmetic so that the NumPy
// restatement of tests/draw_ref.py agrees bit for bit.  With d2 the squared distance of the pixel to the centre:
//   disc of radius r:          d2 <= r*r
//   ring of radius r, 1 thick: (2r-1)^2 <= 4*d2 < (2r+1)^2
//   edge p0-p1 of thickness th, a = p - p0, b = p1 - p0:  a.b <= 0 (or b.b == 0): 4*|a|^2 <= th*th;  a.b >= b.b: 4*|p-p1|^2 <= th*th;
//       else 4*(|a|^2*(b.b) - (a.b)^2) <= th*th*(b.b).  |a|^2*(b.b) - (a.b)^2 is (a x b)^2, and coordinates reach +-32768, where that
//       square leaves 64 bits; so the test is evaluated as 2*|a x b| <= isqrt(th*th*(b.b)), the same truth value with every
//       intermediate below 2^52.  isqrt is taken once per primitive.
// Joint pixels are rint (half to even) of the float coordinate, clamped to +-32768 (a NaN goes to -32768) before the conversion.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "hpe_ctx.h"

namespace {

constexpr int NJ = HPE_DRAW_JOINTS;
constexpr int DRAW_THREADS = 256;
constexpr int DRAW_ROWS = 8;            // rows of the output one workgroup composes
constexpr int SLOTS_PER_CHILD = 4;      // white disc, joint disc, parent disc, edge (a ring pass uses the first only)
constexpr int PASS_SLOTS = NJ * SLOTS_PER_CHILD;
constexpr int SKEL_STRIDE = 8;          // int32 per joint of the skeleton table: parent, joint RGB, edge RGB, 0

typedef unsigned int u32;
typedef long long i64;

enum { PRIM_NONE = 0, PRIM_DISC = 1, PRIM_RING = 2, PRIM_EDGE = 3 };

struct Prim {
    int type;
    int x0, y0, x1, y1;
    int r;        // disc / ring: the radius; edge: the thickness
    u32 color;    // R | G << 8 | B << 16
    int pad;
    i64 lim;      // edge: isqrt(th * th * b.b)
};

__device__ __forceinline__ int joint_pixel(float v) {  // v already in pixels
    const float c = fminf(fmaxf(rintf(v), -32768.0f), 32768.0f);  // fmaxf returns the other operand for a NaN: -32768
    return (int)c;
}

__device__ __forceinline__ i64 isqrt64(i64 v) {  // floor(sqrt(v)) for 0 <= v < 2^52
    i64 r = (i64)sqrt((double)v);
    while (r * r > v) --r;
    while ((r + 1) * (r + 1) <= v) ++r;
    return r;
}

__device__ __forceinline__ u32 rgb_of(const int* __restrict__ t) { return ((u32)t[0] & 255u) | ((u32)t[1] & 255u) << 8 | ((u32)t[2] & 255u) << 16; }

// The slots of child `c` of one draw_skeleton call (renderer.py:411-438).  jx / jy: the 19 joint pixels; vis: nullptr = all visible
__device__ void emit_child(Prim* slots, int c, const int* jx, const int* jy, const unsigned char* vis, bool draw_edges, int r,
                           const int* __restrict__ skel) {
#pragma unroll
    for (int k = 0; k < SLOTS_PER_CHILD; ++k) slots[k].type = PRIM_NONE;
    if (vis && !vis[c]) return;
    const int* row = skel + c * SKEL_STRIDE;
    const u32 jc = rgb_of(row + 1);
    Prim p;
    p.x0 = p.x1 = jx[c], p.y0 = p.y1 = jy[c], p.pad = 0, p.lim = 0;
    if (!draw_edges) {
        p.type = PRIM_RING, p.r = r - 1, p.color = jc;
        slots[0] = p;
        return;
    }
    p.type = PRIM_DISC, p.r = r, p.color = 0xFFFFFFu;
    slots[0] = p;
    p.r = r - 1, p.color = jc;
    slots[1] = p;
    int pa = row[0];
    if (pa < 0 || pa >= NJ) return;  // -1: no parent
    if (vis && !vis[pa]) return;
    p.x0 = p.x1 = jx[pa], p.y0 = p.y1 = jy[pa], p.color = rgb_of(skel + pa * SKEL_STRIDE + 1);
    slots[2] = p;
    const int th = max(1, r - 2);
    p.type = PRIM_EDGE, p.x0 = jx[c], p.y0 = jy[c], p.r = th, p.color = rgb_of(row + 4);
    const i64 bx = (i64)p.x1 - p.x0, by = (i64)p.y1 - p.y0;
    p.lim = isqrt64((i64)th * th * (bx * bx + by * by));  // th <= 2^8, b.b <= 2^35
    slots[3] = p;
}

__device__ __forceinline__ bool covers(const Prim& p, int x, int y) {
    if (p.type == PRIM_NONE) return false;
    const i64 ax = (i64)x - p.x0, ay = (i64)y - p.y0;
    const i64 d2 = ax * ax + ay * ay;
    if (p.type == PRIM_DISC) return d2 <= (i64)p.r * p.r;
    if (p.type == PRIM_RING) {
        const i64 lo = 2 * (i64)p.r - 1, hi = 2 * (i64)p.r + 1;
        return lo * lo <= 4 * d2 && 4 * d2 < hi * hi;
    }
    const i64 bx = (i64)p.x1 - p.x0, by = (i64)p.y1 - p.y0;
    const i64 ab = ax * bx + ay * by, bb = bx * bx + by * by, t2 = (i64)p.r * p.r;
    if (ab <= 0) return 4 * d2 <= t2;  // bb == 0 lands here
    if (ab >= bb) {
        const i64 cx = (i64)x - p.x1, cy = (i64)y - p.y1;
        return 4 * (cx * cx + cy * cy) <= t2;
    }
    const i64 cross = ax * by - ay * bx;
    return 2 * (cross < 0 ? -cross : cross) <= p.lim;
}

// the colour of pixel (x, y) under `count` slots, or `under` when none covers it
__device__ __forceinline__ u32 paint(const Prim* list, int count, int x, int y, u32 under) {
    for (int k = count - 1; k >= 0; --k)
        if (covers(list[k], x, y)) return list[k].color;
    return under;
}

__device__ __forceinline__ u32 crop_byte(float v) {  // trunc(((v + 1) * 0.5) * 255) clamped to [0, 255], each operation rounded on its own
    const float f = __fmul_rn(__fmul_rn(__fadd_rn(v, 1.0f), 0.5f), 255.0f);
    return (u32)truncf(fminf(fmaxf(f, 0.0f), 255.0f));  // a NaN reads 0
}

__global__ __launch_bounds__(DRAW_THREADS) void draw_panels_kernel(const float* __restrict__ images, const float* __restrict__ kp_gt,
                                                                   const float* __restrict__ kp_pred, const unsigned char* __restrict__ rend_img,
                                                                   const unsigned char* __restrict__ rend_seg, const int* __restrict__ skel, int T,
                                                                   int S, unsigned char* __restrict__ out) {
    __shared__ Prim list[2 * PASS_SLOTS];
    __shared__ int gx[NJ], gy[NJ], px[NJ], py[NJ];
    __shared__ unsigned char gvis[NJ];
    const int panel = blockIdx.y, i = panel / T;  // panel = i * T + t
    const int r = max(4, (int)(0.01 * (double)S));
    if (threadIdx.x < NJ) {
        const int j = threadIdx.x;
        const float* g = kp_gt + ((size_t)i * NJ + j) * 3;
        const float* p = kp_pred + ((size_t)panel * NJ + j) * 2;
        const float s = (float)S;
        gx[j] = joint_pixel(__fmul_rn(__fmul_rn(__fadd_rn(g[0], 1.0f), 0.5f), s));
        gy[j] = joint_pixel(__fmul_rn(__fmul_rn(__fadd_rn(g[1], 1.0f), 0.5f), s));
        gvis[j] = g[2] != 0.0f ? 1 : 0;  // astype(bool): a NaN is visible
        px[j] = joint_pixel(__fmul_rn(__fmul_rn(__fadd_rn(p[0], 1.0f), 0.5f), s));
        py[j] = joint_pixel(__fmul_rn(__fmul_rn(__fadd_rn(p[1], 1.0f), 0.5f), s));
    }
    __syncthreads();
    if (threadIdx.x < NJ) {
        emit_child(list + threadIdx.x * SLOTS_PER_CHILD, threadIdx.x, gx, gy, gvis, false, r, skel);               // ground truth: rings
        emit_child(list + PASS_SLOTS + threadIdx.x * SLOTS_PER_CHILD, threadIdx.x, px, py, nullptr, true, r, skel);  // then the prediction
    }
    __syncthreads();
    const int W3 = 3 * S, y0 = blockIdx.x * DRAW_ROWS, rows = min(DRAW_ROWS, S - y0);
    const float* img = images + (size_t)i * S * S * 3;
    const unsigned char* ri = rend_img + (size_t)panel * S * S * 3;
    const unsigned char* rs = rend_seg + (size_t)panel * S * S * 3;
    unsigned char* dst = out + (size_t)panel * S * W3 * 3;  // [n][T*S][3S][3]: panel (i, t) starts at row (i * T + t) * S
    for (int q = threadIdx.x; q < rows * W3; q += DRAW_THREADS) {
        const int y = y0 + q / W3, X = q % W3, col = X / S, x = X - col * S;
        u32 c;
        if (col == 0) {
            const float* s = img + ((size_t)y * S + x) * 3;
            c = paint(list, 2 * PASS_SLOTS, x, y, crop_byte(s[0]) | crop_byte(s[1]) << 8 | crop_byte(s[2]) << 16);
        } else {
            const unsigned char* s = (col == 1 ? ri : rs) + ((size_t)y * S + x) * 3;
            c = (u32)s[0] | (u32)s[1] << 8 | (u32)s[2] << 16;
        }
        unsigned char* d = dst + ((size_t)y * W3 + X) * 3;
        d[0] = (unsigned char)c, d[1] = (unsigned char)(c >> 8), d[2] = (unsigned char)(c >> 16);
    }
}

// in place: a pixel reads and writes only itself
__global__ __launch_bounds__(DRAW_THREADS) void draw_skeleton_kernel(unsigned char* __restrict__ images, const float* __restrict__ joints,
                                                                     const unsigned char* __restrict__ vis, const int* __restrict__ skel, int H, int W,
                                                                     int draw_edges, int r) {
    __shared__ Prim list[PASS_SLOTS];
    __shared__ int jx[NJ], jy[NJ];
    __shared__ unsigned char jv[NJ];
    const int i = blockIdx.y;
    if (threadIdx.x < NJ) {
        const int j = threadIdx.x;
        jx[j] = joint_pixel(joints[((size_t)i * NJ + j) * 2]);
        jy[j] = joint_pixel(joints[((size_t)i * NJ + j) * 2 + 1]);
        jv[j] = vis ? vis[(size_t)i * NJ + j] : 1;
    }
    __syncthreads();
    if (threadIdx.x < NJ) emit_child(list + threadIdx.x * SLOTS_PER_CHILD, threadIdx.x, jx, jy, vis ? jv : nullptr, draw_edges != 0, r, skel);
    __syncthreads();
    const int y0 = blockIdx.x * DRAW_ROWS, rows = min(DRAW_ROWS, H - y0);
    unsigned char* img = images + (size_t)i * H * W * 3;
    for (int q = threadIdx.x; q < rows * W; q += DRAW_THREADS) {
        const int y = y0 + q / W, x = q % W;
        unsigned char* d = img + ((size_t)y * W + x) * 3;
        const u32 none = 0xFF000000u;  // no colour has the top byte set
        const u32 c = paint(list, PASS_SLOTS, x, y, none);
        if (c != none) d[0] = (unsigned char)c, d[1] = (unsigned char)(c >> 8), d[2] = (unsigned char)(c >> 16);
    }
}

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int hpe_draw_panels(const float* images, const float* kp_gt, const float* kp_pred, const unsigned char* rend_img, const unsigned char* rend_seg,
                    const int* skeleton, int n, int T, int S, unsigned char* out, void* stream) {
    if (n < 1 || T < 1) return fail(HPE_ERR_INVALID, "n and T must be >= 1");
    if (S < 1 || S > HPE_PNG_MAX_SIDE) return fail(HPE_ERR_INVALID, "S must be in [1, 16384]");
    if ((long long)n * T > 65535) return fail(HPE_ERR_INVALID, "n * T must be at most 65535");
    if ((long long)T * S > HPE_PNG_MAX_SIDE || 3LL * S > HPE_PNG_MAX_SIDE) return fail(HPE_ERR_INVALID, "the panel T*S x 3*S exceeds 16384 on a side");
    if (!images || !kp_gt || !kp_pred || !rend_img || !rend_seg || !skeleton || !out) return fail(HPE_ERR_INVALID, "null argument");
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(draw_panels_kernel, dim3((unsigned)((S + DRAW_ROWS - 1) / DRAW_ROWS), (unsigned)(n * T)), dim3(DRAW_THREADS), 0, st, images, kp_gt,
                       kp_pred, rend_img, rend_seg, skeleton, T, S, out);
    HIP_TRY(hipGetLastError());
    return HPE_OK;
}

int hpe_draw_skeleton(unsigned char* images, const float* joints, const unsigned char* vis, const int* skeleton, int n, int H, int W,
                      int draw_edges, int radius, void* stream) {
    if (n < 1 || n > 65535) return fail(HPE_ERR_INVALID, "n must be in [1, 65535]");
    if (H < 1 || W < 1 || H > HPE_PNG_MAX_SIDE || W > HPE_PNG_MAX_SIDE) return fail(HPE_ERR_INVALID, "H and W must be in [1, 16384]");
    if (radius < 1 || radius > HPE_DRAW_MAX_RADIUS) return fail(HPE_ERR_INVALID, "radius must be in [1, 256]");  // keeps th * th * b.b below 2^52
    if (!images || !joints || !skeleton) return fail(HPE_ERR_INVALID, "null argument");
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(draw_skeleton_kernel, dim3((unsigned)((H + DRAW_ROWS - 1) / DRAW_ROWS), (unsigned)n), dim3(DRAW_THREADS), 0, st, images, joints, vis,
                       skeleton, H, W, draw_edges, radius);
    HIP_TRY(hipGetLastError());
    return HPE_OK;
}

}  // extern "C"
#pragma GCC visibility pop
