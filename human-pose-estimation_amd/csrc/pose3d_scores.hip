// pose3d_scores.hip -- the 3-D scores of a batch (DESIGN.md "3-D pose scores"): per image and IEF stage the root-aligned and the
// Procrustes-aligned error of every joint, their means (MPJPE, PA-MPJPE), the same two for the mesh vertices (PVE, PA-PVE) and both fits.
// One launch, one workgroup per (image, stage):
//   sweep 1   every thread strides over the points of a cloud pair and keeps 16 double sums of the points relative to a pivot (the first
//             scored point of each cloud): n is counted apart, sum x', sum y', sum |x'|^2, sum x' y'^T.  A wave adds them by shuffles, the
//             waves' sums meet in LDS and thread 0 adds them in wave order; from them the means, var1 and K = X1^T X2.  The pivot keeps the
//             subtraction of the means' product free of cancellation for a cloud far from the origin.
//   solve     thread 0 runs procrustes3::solve and leaves scale, R and both means in LDS.
//   sweep 2   the residuals scale R (x - mu1) - (y - mu2) and the root-aligned differences; their sums go the same way as sweep 1's.
// The joints go first (their roots translate the vertices too), then the vertices.  Everything between the float32 loads and the float32
// stores is double, in an order fixed by the launch shape alone: no atomics, the same inputs give the same bits.
#include <hip/hip_runtime.h>
#include <math.h>

#include <string>

#include "hpe_ctx.h"
#include "procrustes3.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxStage = 16;
constexpr int kSums = 16;

// flag bits of summary[5]
constexpr int kFlagRoot = 1;     // a root joint is not scored: the root-aligned values are NaN
constexpr int kFlagPaJoints = 2; // fewer than 3 scored joints, or var1 == 0: the joint fit is undefined
constexpr int kFlagPaVerts = 4;  // fewer than 3 vertices, or var1 == 0: the vertex fit is undefined
constexpr int kFlagNoVerts = 8;  // no vertices were given

struct Pose3dArgs {
    const float* joints[kMaxStage];
    const float* verts[kMaxStage];
    const float* joints_gt;
    const float* weights;
    const float* verts_gt;
    float* joint_err;
    float* summary;
    float* xform;
    int n_stage, B, K, P, root_a, root_b;
};

struct Fit {
    double scale, R[9], mu1[3], mu2[3];
    int n, valid;
};

struct Shared {
    double part[kWaves][kSums];
    double total[kSums];
    Fit fit;
    int pivot;
};

// sums v[0 .. N) over the workgroup in a fixed order; every thread gets the totals.  Two barriers; s.total is free again after the second
template <int N>
__device__ __forceinline__ void block_sum(double (&v)[N], Shared& s) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
#pragma unroll
    for (int i = 0; i < N; ++i)
        for (int o = 32; o > 0; o >>= 1) v[i] += __shfl_down(v[i], o);
    __syncthreads();  // the previous totals have been read
    if (lane == 0)
#pragma unroll
        for (int i = 0; i < N; ++i) s.part[wave][i] = v[i];
    __syncthreads();
    if (t < N) {
        double a = s.part[0][t];
        for (int w = 1; w < kWaves; ++w) a += s.part[w][t];
        s.total[t] = a;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = s.total[i];
}

__device__ __forceinline__ void load3(const float* p, size_t i, double o[3]) {
    o[0] = (double)p[3 * i], o[1] = (double)p[3 * i + 1], o[2] = (double)p[3 * i + 2];
}

// The similarity fit of X to Y over the points with w > 0 (w == nullptr: all N) into s.fit, for every thread to read after it returns
__device__ void fit_clouds(const float* X, const float* Y, const float* w, int N, Shared& s) {
#pragma clang fp contract(off)
    const int t = threadIdx.x;
    if (t == 0) {
        int p = -1;
        if (!w) p = N > 0 ? 0 : -1;
        else
            for (int i = 0; i < N && p < 0; ++i)
                if (w[i] > 0.f) p = i;
        s.pivot = p;
    }
    __syncthreads();
    const int pivot = s.pivot;
    double px[3] = {0, 0, 0}, py[3] = {0, 0, 0};
    if (pivot >= 0) {
        load3(X, pivot, px);
        load3(Y, pivot, py);
    }
    double v[kSums];
#pragma unroll
    for (int i = 0; i < kSums; ++i) v[i] = 0.0;
    int cnt = 0;
    for (int i = t; i < N; i += kThreads) {
        if (w && !(w[i] > 0.f)) continue;
        double x[3], y[3];
        load3(X, i, x);
        load3(Y, i, y);
#pragma unroll
        for (int a = 0; a < 3; ++a) x[a] -= px[a], y[a] -= py[a];
        ++cnt;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            v[a] += x[a];
            v[3 + a] += y[a];
            v[6] += x[a] * x[a];
#pragma unroll
            for (int b = 0; b < 3; ++b) v[7 + 3 * a + b] += x[a] * y[b];
        }
    }
    block_sum(v, s);
    double c[1] = {(double)cnt};  // exact: at most 2^31 points
    block_sum(c, s);
    if (t == 0) {
        Fit& f = s.fit;
        const double n = c[0];
        f.n = (int)n;
        const double nan = __builtin_nan("");
        double m1[3], m2[3], K[9], var1 = v[6];
        for (int a = 0; a < 3; ++a) m1[a] = n > 0 ? v[a] / n : nan, m2[a] = n > 0 ? v[3 + a] / n : nan;
        for (int a = 0; a < 3; ++a) {
            var1 -= n * m1[a] * m1[a];
            for (int b = 0; b < 3; ++b) K[3 * a + b] = v[7 + 3 * a + b] - n * m1[a] * m2[b];
            f.mu1[a] = px[a] + m1[a];
            f.mu2[a] = py[a] + m2[a];
        }
        f.valid = n >= 3 && !(var1 <= 0.0);  // a NaN var1 is not "undefined": the NaN goes through to the outputs
        if (f.valid) {
            double tr;
            procrustes3::solve(K, f.R, &tr);
            f.scale = tr / var1;
        } else {
            f.scale = nan;
            for (int i = 0; i < 9; ++i) f.R[i] = nan;
        }
    }
    __syncthreads();
}

// | scale R (x - mu1) - (y - mu2) |
__device__ __forceinline__ double pa_residual(const Fit& f, const double x[3], const double y[3]) {
#pragma clang fp contract(off)
    double d[3], e = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) d[a] = x[a] - f.mu1[a];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double r = f.scale * (f.R[3 * a] * d[0] + f.R[3 * a + 1] * d[1] + f.R[3 * a + 2] * d[2]) - (y[a] - f.mu2[a]);
        e += r * r;
    }
    return sqrt(e);
}

// | (x - rx) - (y - ry) |
__device__ __forceinline__ double root_residual(const double x[3], const double rx[3], const double y[3], const double ry[3]) {
#pragma clang fp contract(off)
    double e = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double r = (x[a] - rx[a]) - (y[a] - ry[a]);
        e += r * r;
    }
    return sqrt(e);
}

__device__ __forceinline__ void store_xform(float* o, const Fit& f) {
#pragma clang fp contract(off)
    o[0] = (float)f.scale;
    for (int i = 0; i < 9; ++i) o[1 + i] = (float)f.R[i];
    for (int a = 0; a < 3; ++a)
        o[10 + a] = (float)(f.mu2[a] - f.scale * (f.R[3 * a] * f.mu1[0] + f.R[3 * a + 1] * f.mu1[1] + f.R[3 * a + 2] * f.mu1[2]));
}

__global__ __launch_bounds__(kThreads) void pose3d_scores_kernel(Pose3dArgs a) {
#pragma clang fp contract(off)
    __shared__ Shared s;
    const int b = blockIdx.x, st = blockIdx.y, t = threadIdx.x;
    const size_t img = (size_t)st * a.B + b;
    const float* J = a.joints[st] + (size_t)b * a.K * 3;
    const float* G = a.joints_gt + (size_t)b * a.K * 3;
    const float* w = a.weights ? a.weights + (size_t)b * a.K : nullptr;
    const double nan = __builtin_nan("");

    // the roots: the mean of two joints of each skeleton, defined when both are scored
    const bool root_ok = !w || (w[a.root_a] > 0.f && w[a.root_b] > 0.f);
    double rx[3], ry[3], xa[3], xb[3];
    load3(J, a.root_a, xa);
    load3(J, a.root_b, xb);
    for (int i = 0; i < 3; ++i) rx[i] = root_ok ? 0.5 * (xa[i] + xb[i]) : nan;
    load3(G, a.root_a, xa);
    load3(G, a.root_b, xb);
    for (int i = 0; i < 3; ++i) ry[i] = root_ok ? 0.5 * (xa[i] + xb[i]) : nan;

    fit_clouds(J, G, w, a.K, s);
    Fit f = s.fit;
    int flags = (root_ok ? 0 : kFlagRoot) | (f.valid ? 0 : kFlagPaJoints) | (a.verts_gt ? 0 : kFlagNoVerts);
    if (t == 0 && a.xform) store_xform(a.xform + img * 26, f);
    double e[2] = {0.0, 0.0};
    for (int k = t; k < a.K; k += kThreads) {
        float o0 = -1.f, o1 = -1.f;
        if (!w || w[k] > 0.f) {
            double x[3], y[3];
            load3(J, k, x);
            load3(G, k, y);
            const double e0 = root_residual(x, rx, y, ry), e1 = pa_residual(f, x, y);  // NaN where the alignment is undefined
            e[0] += e0, e[1] += e1;
            o0 = (float)e0, o1 = (float)e1;
        }
        if (a.joint_err) {
            a.joint_err[(img * 2) * a.K + k] = o0;
            a.joint_err[(img * 2 + 1) * a.K + k] = o1;
        }
    }
    block_sum(e, s);
    const double mpjpe = f.n > 0 ? e[0] / f.n : nan, pa_mpjpe = f.n > 0 ? e[1] / f.n : nan;
    const int scored = f.n;

    double pve = nan, pa_pve = nan;
    if (a.verts_gt) {
        const float* V = a.verts[st] + (size_t)b * a.P * 3;
        const float* VG = a.verts_gt + (size_t)b * a.P * 3;
        fit_clouds(V, VG, nullptr, a.P, s);
        f = s.fit;
        if (!f.valid) flags |= kFlagPaVerts;
        e[0] = e[1] = 0.0;
        for (int i = t; i < a.P; i += kThreads) {
            double x[3], y[3];
            load3(V, i, x);
            load3(VG, i, y);
            e[0] += root_residual(x, rx, y, ry);
            e[1] += pa_residual(f, x, y);
        }
        block_sum(e, s);
        pve = e[0] / a.P, pa_pve = e[1] / a.P;
    } else {
        f.valid = 0, f.scale = nan;
        for (int i = 0; i < 9; ++i) f.R[i] = nan;
    }
    if (t == 0) {
        if (a.xform) store_xform(a.xform + img * 26 + 13, f);
        if (a.summary) {
            float* o = a.summary + img * 6;
            o[0] = (float)mpjpe, o[1] = (float)pa_mpjpe, o[2] = (float)pve, o[3] = (float)pa_pve, o[4] = (float)scored, o[5] = (float)flags;
        }
    }
}

}  // namespace

#pragma GCC visibility push(default)
extern "C" int hpe_debug_procrustes3(const double K[9], double R[9], double* trace_RK) {
    if (!K || !R || !trace_RK) return fail(HPE_ERR_INVALID, "hpe_debug_procrustes3: K, R or trace_RK is NULL");
    procrustes3::solve(K, R, trace_RK);
    return HPE_OK;
}

extern "C" int hpe_pose3d_scores(const float* const* joints, const float* joints_gt, const float* joint_weights, const float* const* verts,
                                 const float* verts_gt, int n_stage, int B, int K, int P, int root_a, int root_b, float* joint_err, float* summary,
                                 float* xform, void* stream) {
    if (!joints || !joints_gt) return fail(HPE_ERR_INVALID, "hpe_pose3d_scores: joints_dev or joints_gt_dev is NULL");
    if (n_stage < 1 || n_stage > kMaxStage) return fail(HPE_ERR_INVALID, "hpe_pose3d_scores: n_stage " + std::to_string(n_stage) + " outside [1, 16]");
    if (B < 1) return fail(HPE_ERR_INVALID, "hpe_pose3d_scores: batch " + std::to_string(B) + " < 1");
    if (K < 1) return fail(HPE_ERR_INVALID, "hpe_pose3d_scores: K " + std::to_string(K) + " < 1");
    if (root_a < 0 || root_a >= K || root_b < 0 || root_b >= K)
        return fail(HPE_ERR_INVALID, "hpe_pose3d_scores: roots (" + std::to_string(root_a) + ", " + std::to_string(root_b) + ") outside [0, " + std::to_string(K) + ")");
    if ((verts == nullptr) != (verts_gt == nullptr)) return fail(HPE_ERR_INVALID, "hpe_pose3d_scores: verts_dev and verts_gt_dev must be given together");
    if (verts && P < 1) return fail(HPE_ERR_INVALID, "hpe_pose3d_scores: P " + std::to_string(P) + " < 1");
    if (!joint_err && !summary && !xform) return fail(HPE_ERR_INVALID, "hpe_pose3d_scores: every output is NULL, nothing to write");
    Pose3dArgs a = {};
    for (int s = 0; s < n_stage; ++s) {
        if (!joints[s]) return fail(HPE_ERR_INVALID, "hpe_pose3d_scores: joints_dev[" + std::to_string(s) + "] is NULL");
        if (verts && !verts[s]) return fail(HPE_ERR_INVALID, "hpe_pose3d_scores: verts_dev[" + std::to_string(s) + "] is NULL");
        a.joints[s] = joints[s];
        a.verts[s] = verts ? verts[s] : nullptr;
    }
    a.joints_gt = joints_gt, a.weights = joint_weights, a.verts_gt = verts_gt;
    a.joint_err = joint_err, a.summary = summary, a.xform = xform;
    a.n_stage = n_stage, a.B = B, a.K = K, a.P = verts ? P : 0, a.root_a = root_a, a.root_b = root_b;
    hipLaunchKernelGGL(pose3d_scores_kernel, dim3(B, n_stage), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
    HIP_TRY(hipGetLastError());
    return HPE_OK;
}
#pragma GCC visibility pop
