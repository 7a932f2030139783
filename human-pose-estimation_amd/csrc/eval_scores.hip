// eval_scores.hip -- what a checkpoint is scored by (DESIGN.md "Checkpoint scores"): per image and IEF stage the confusion counts of the
// projected mesh's silhouette against the ground-truth mask, and the per-joint keypoint error in pixels with the PCK normalisers.
// One launch, one workgroup per image:
//   keypoints   threads stride over (stage, joint); two threads write the torso and head length of the ground truth.
//   ground truth bitmap, once: a wave reads 64 consecutive mask pixels of a row (coalesced) and its ballot is two dwords of the row.
//   per stage   the predicted bitmap (H x ceil(W / 32) dwords in LDS) is cleared; threads stride over the faces: snap the three vertices
//               to 1/256 px, reject, orient, clip the box of pixel samples to the image.  A face whose box holds at most kSmallBox samples
//               is walked by its own lane; the others are handed round the wave (ballot + shuffles, no queue, no barrier) and walked by
//               its 64 lanes, one (row, dword) span each.  Every span is one LDS atomicOr.  Then tp / fp / fn are popcounts of the two
//               bitmaps, summed over the wave by shuffles and over the workgroup by LDS integer adds.
// Coverage is the renderer's rule (render.hip: int64 edge functions, top-left tie rule) at the sample (x, y) = (column, row), which is where
// mesh_reprojection_loss places the mask's pixels; a silhouette is a union, so it does not depend on the order of the faces, and every sum
// is an integer: the same inputs give the same bits.  No global atomics, no workspace, no synchronisation.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <string>

#include "hpe_ctx.h"

namespace {

constexpr int kThreads = 1024;      // one workgroup per image, so a CU holds one: sixteen waves keep its four SIMDs fed
constexpr int kSmallBox = 64;       // boxes of more samples than this are walked by the wave
constexpr int kMaxStage = 16;
constexpr int kLdsBytes = 64 * 1024;  // what a workgroup gets without an opt-in
constexpr float kGuard = 16384.f;   // the renderer's guard band (pixels)

struct EvalArgs {
    const float* verts2d[kMaxStage];
    const float* kp2d[kMaxStage];
    const int* faces;
    const float* seg;
    const float* kp_gt;
    int* counts;
    float* kp_err;
    float* norm;
    int n_stage, B, P, K, H, W, F, WD;  // WD = dwords per bitmap row
};

// a face in 1/256 px, positively oriented, with the clipped inclusive box of the pixel samples (256 j, 256 i) it may cover
struct Tri {
    int x[3], y[3];
    int bx0, bx1, by0, by1;
};

// render.hip's edge function: directed edge a -> b at p; |coordinates| <= 2^22, so products stay below 2^47
__device__ __forceinline__ long long edge_fn(int ax, int ay, int bx, int by, long long px, long long py) {
    return (long long)(bx - ax) * (py - ay) - (long long)(by - ay) * (px - ax);
}

// render.hip's tie rule: an edge of a positively oriented triangle owns the samples on it when it points down (+y), or along -x when horizontal
__device__ __forceinline__ bool edge_owns(int ax, int ay, int bx, int by) { return (by > ay) || (by == ay && bx < ax); }

__device__ __forceinline__ bool snap(const float* v, int idx, int P, int& X, int& Y) {
    if ((unsigned)idx >= (unsigned)P) return false;  // hpe_eval_scores cannot see the device's face list: never read outside the vertices
    const float x = v[2 * (size_t)idx], y = v[2 * (size_t)idx + 1];
    if (!(isfinite(x) && isfinite(y) && fabsf(x) <= kGuard && fabsf(y) <= kGuard)) return false;
    X = (int)rintf(256.f * x);
    Y = (int)rintf(256.f * y);
    return true;
}

// false for a dropped face or one whose box holds no sample of the image
__device__ __forceinline__ bool tri_setup(const EvalArgs& a, const float* v, int f, Tri& s) {
    const int* fv = a.faces + (size_t)f * 3;
    if (!snap(v, fv[0], a.P, s.x[0], s.y[0]) || !snap(v, fv[1], a.P, s.x[1], s.y[1]) || !snap(v, fv[2], a.P, s.x[2], s.y[2])) return false;
    const long long A = edge_fn(s.x[0], s.y[0], s.x[1], s.y[1], s.x[2], s.y[2]);
    if (A == 0) return false;
    if (A < 0) {  // both windings are drawn
        int t = s.x[1];
        s.x[1] = s.x[2];
        s.x[2] = t;
        t = s.y[1];
        s.y[1] = s.y[2];
        s.y[2] = t;
    }
    const int minX = min(s.x[0], min(s.x[1], s.x[2])), maxX = max(s.x[0], max(s.x[1], s.x[2]));
    const int minY = min(s.y[0], min(s.y[1], s.y[2])), maxY = max(s.y[0], max(s.y[1], s.y[2]));
    // first / last pixel whose sample 256 j lies in [min, max]: ceil(min / 256), floor(max / 256)
    s.bx0 = max(-((-minX) >> 8), 0);
    s.bx1 = min(maxX >> 8, a.W - 1);
    s.by0 = max(-((-minY) >> 8), 0);
    s.by1 = min(maxY >> 8, a.H - 1);
    return s.bx0 <= s.bx1 && s.by0 <= s.by1;
}

// coverage bits of the pixels xa .. xb (one dword's worth) of row y.  E + own - 1 >= 0 is "E > 0, or E == 0 on an owned edge" for integers,
// so a sample is inside when none of the three biased edge functions is negative
__device__ __forceinline__ unsigned span_mask(const Tri& s, int y, int xa, int xb) {
    const long long px = 256LL * xa, py = 256LL * y;
    long long E0 = edge_fn(s.x[1], s.y[1], s.x[2], s.y[2], px, py) + (edge_owns(s.x[1], s.y[1], s.x[2], s.y[2]) ? 0 : -1);
    long long E1 = edge_fn(s.x[2], s.y[2], s.x[0], s.y[0], px, py) + (edge_owns(s.x[2], s.y[2], s.x[0], s.y[0]) ? 0 : -1);
    long long E2 = edge_fn(s.x[0], s.y[0], s.x[1], s.y[1], px, py) + (edge_owns(s.x[0], s.y[0], s.x[1], s.y[1]) ? 0 : -1);
    // one pixel to the right changes edge (a -> b) by -(by - ay) * 256
    const long long d0 = -256LL * (s.y[2] - s.y[1]), d1 = -256LL * (s.y[0] - s.y[2]), d2 = -256LL * (s.y[1] - s.y[0]);
    unsigned m = 0;
    for (int x = xa; x <= xb; ++x) {
        if ((E0 | E1 | E2) >= 0) m |= 1u << (x & 31);
        E0 += d0;
        E1 += d1;
        E2 += d2;
    }
    return m;
}

__device__ __forceinline__ void draw_span(const Tri& s, int y, int w, unsigned* pred, int WD) {
    const unsigned m = span_mask(s, y, max(s.bx0, 32 * w), min(s.bx1, 32 * w + 31));
    if (m) atomicOr(&pred[y * WD + w], m);  // ds_or_b32
}

__device__ __forceinline__ float px_dist(float ax, float ay, float bx, float by, int H, int W) {
    const float dx = 0.5f * (float)W * (ax - bx), dy = 0.5f * (float)H * (ay - by);
    return sqrtf(dx * dx + dy * dy);
}

__global__ __launch_bounds__(kThreads) void eval_scores_kernel(EvalArgs a) {
    extern __shared__ unsigned lds[];
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;

    if (a.kp_gt) {
        const float* g = a.kp_gt + (size_t)b * a.K * 3;
        for (int i = t; i < a.n_stage * a.K; i += kThreads) {
            const int s = i / a.K, k = i - s * a.K;
            const float* p = a.kp2d[s] + ((size_t)b * a.K + k) * 2;
            a.kp_err[((size_t)s * a.B + b) * a.K + k] = g[3 * k + 2] > 0.f ? px_dist(p[0], p[1], g[3 * k], g[3 * k + 1], a.H, a.W) : -1.f;
        }
        if (t < 2) {  // LSP order: torso = left shoulder (9) -- right hip (2), head = head top (13) -- neck (12)
            const int j0 = t ? 13 : 9, j1 = t ? 12 : 2;
            float d = -1.f;
            if (j0 < a.K && g[3 * j0 + 2] > 0.f && g[3 * j1 + 2] > 0.f) d = px_dist(g[3 * j0], g[3 * j0 + 1], g[3 * j1], g[3 * j1 + 1], a.H, a.W);
            a.norm[b * 2 + t] = d;
        }
    }
    if (!a.seg) return;

    const int WD = a.WD, nw = a.H * WD;
    unsigned* pred = lds;
    unsigned* gt = lds + nw;
    int* cnt = (int*)(lds + 2 * nw);  // tp, fp, fn of the stage

    // ground-truth bits: item = (row, 64 columns); the ballot of seg > 0 is dwords 2c and 2c + 1 of the row, each written exactly once
    const int C64 = (a.W + 63) >> 6;
    const float* seg = a.seg + (size_t)b * a.H * a.W;
    for (int it = wave; it < a.H * C64; it += kThreads / 64) {
        const int row = it / C64, c = it - row * C64, col = 64 * c + lane;
        const bool fg = col < a.W && seg[(size_t)row * a.W + col] > 0.f;
        const unsigned long long m = __ballot(fg);
        if (lane == 0) {
            gt[row * WD + 2 * c] = (unsigned)m;
            if (2 * c + 1 < WD) gt[row * WD + 2 * c + 1] = (unsigned)(m >> 32);
        }
    }
    const unsigned last = (a.W & 31) ? (1u << (a.W & 31)) - 1u : ~0u;  // the columns a row's last dword really has

    for (int s = 0; s < a.n_stage; ++s) {
        for (int i = t; i < nw; i += kThreads) pred[i] = 0u;
        if (t == 0) cnt[0] = cnt[1] = cnt[2] = 0;  // thread 0 also read them last, below
        __syncthreads();
        const float* v = a.verts2d[s] + (size_t)b * a.P * 2;
        for (int f0 = 0; f0 < a.F; f0 += kThreads) {  // uniform over the workgroup: every lane reaches the ballot
            const int f = f0 + t;
            Tri tr = {};
            const bool live = f < a.F && tri_setup(a, v, f, tr);
            const bool big = live && (tr.bx1 - tr.bx0 + 1) * (tr.by1 - tr.by0 + 1) > kSmallBox;
            if (live && !big)
                for (int y = tr.by0; y <= tr.by1; ++y)
                    for (int w = tr.bx0 >> 5; w <= tr.bx1 >> 5; ++w) draw_span(tr, y, w, pred, WD);
            unsigned long long todo = __ballot(big);
            while (todo) {  // a large box: its lane's setup goes round the wave, the 64 lanes stride over its (row, dword) spans
                const int src = __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                Tri o;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    o.x[k] = __shfl(tr.x[k], src);
                    o.y[k] = __shfl(tr.y[k], src);
                }
                o.bx0 = __shfl(tr.bx0, src);
                o.bx1 = __shfl(tr.bx1, src);
                o.by0 = __shfl(tr.by0, src);
                o.by1 = __shfl(tr.by1, src);
                const int w0 = o.bx0 >> 5, wn = (o.bx1 >> 5) - w0 + 1, n = wn * (o.by1 - o.by0 + 1);
                for (int i = lane; i < n; i += 64) draw_span(o, o.by0 + i / wn, w0 + i % wn, pred, WD);
            }
        }
        __syncthreads();
        int tp = 0, fp = 0, fn = 0;
        for (int i = t; i < nw; i += kThreads) {
            const unsigned keep = (i % WD == WD - 1) ? last : ~0u;
            const unsigned p = pred[i] & keep, g = gt[i] & keep;
            tp += __popc(p & g);
            fp += __popc(p & ~g);
            fn += __popc(~p & g);
        }
        for (int o = 32; o > 0; o >>= 1) {
            tp += __shfl_down(tp, o);
            fp += __shfl_down(fp, o);
            fn += __shfl_down(fn, o);
        }
        if (lane == 0) {  // integer sums: any order gives the same counts
            atomicAdd(&cnt[0], tp);
            atomicAdd(&cnt[1], fp);
            atomicAdd(&cnt[2], fn);
        }
        __syncthreads();
        if (t == 0) {
            int* o = a.counts + ((size_t)s * a.B + b) * 4;
            o[0] = cnt[0];
            o[1] = cnt[1];
            o[2] = cnt[2];
            o[3] = a.H * a.W - cnt[0] - cnt[1] - cnt[2];
        }
    }
}

}  // namespace

#pragma GCC visibility push(default)
extern "C" int hpe_eval_scores(const float* const* verts2d, const int* faces, int F, const float* seg, const float* kp_gt, const float* const* kp2d,
                               int n_stage, int B, int P, int K, int H, int W, int* counts, float* kp_err, float* norm, void* stream) {
    if (!verts2d && !kp_gt) return fail(HPE_ERR_INVALID, "hpe_eval_scores: neither verts2d nor kp_gt is given, nothing to score");
    if (n_stage < 1 || n_stage > kMaxStage) return fail(HPE_ERR_INVALID, "hpe_eval_scores: n_stage " + std::to_string(n_stage) + " outside [1, 16]");
    if (B < 1) return fail(HPE_ERR_INVALID, "hpe_eval_scores: batch " + std::to_string(B) + " < 1");
    if (H < 1 || W < 1) return fail(HPE_ERR_INVALID, "hpe_eval_scores: image size " + std::to_string(H) + " x " + std::to_string(W));
    EvalArgs a = {};
    a.n_stage = n_stage, a.B = B, a.P = P, a.K = K, a.H = H, a.W = W, a.F = F;
    size_t lds = 0;
    if (verts2d) {
        if (!faces || !seg) return fail(HPE_ERR_INVALID, "hpe_eval_scores: the silhouette part needs faces_dev and seg_dev");
        if (!counts) return fail(HPE_ERR_INVALID, "hpe_eval_scores: counts_dev is NULL");
        if (F < 1 || P < 1) return fail(HPE_ERR_INVALID, "hpe_eval_scores: F and P must be at least 1");
        for (int s = 0; s < n_stage; ++s) {
            if (!verts2d[s]) return fail(HPE_ERR_INVALID, "hpe_eval_scores: verts2d_dev[" + std::to_string(s) + "] is NULL");
            a.verts2d[s] = verts2d[s];
        }
        const long long WD = (W + 31) / 32, need = 2 * WD * H * 4 + 16;
        if (need > kLdsBytes)
            return fail(HPE_ERR_INVALID, "hpe_eval_scores: the two " + std::to_string(H) + " x " + std::to_string(W) + " bitmaps need " +
                                             std::to_string(need) + " bytes of LDS, a workgroup has " + std::to_string(kLdsBytes));
        a.WD = (int)WD, a.faces = faces, a.seg = seg, a.counts = counts;
        lds = (size_t)need;
    }
    if (kp_gt) {
        if (!kp2d) return fail(HPE_ERR_INVALID, "hpe_eval_scores: the keypoint part needs kp2d_dev");
        if (!kp_err || !norm) return fail(HPE_ERR_INVALID, "hpe_eval_scores: kp_err_dev or norm_dev is NULL");
        if (K < 1) return fail(HPE_ERR_INVALID, "hpe_eval_scores: K must be at least 1");
        for (int s = 0; s < n_stage; ++s) {
            if (!kp2d[s]) return fail(HPE_ERR_INVALID, "hpe_eval_scores: kp2d_dev[" + std::to_string(s) + "] is NULL");
            a.kp2d[s] = kp2d[s];
        }
        a.kp_gt = kp_gt, a.kp_err = kp_err, a.norm = norm;
    }
    hipLaunchKernelGGL(eval_scores_kernel, dim3(B), dim3(kThreads), lds, static_cast<hipStream_t>(stream), a);
    HIP_TRY(hipGetLastError());
    return HPE_OK;
}
#pragma GCC visibility pop
