// adam.hip -- the optimiser update of the reference's two tf.keras.optimizers.Adam (src/trainer.py:183-184), which run TensorFlow's fused
// ResourceApplyAdam (DESIGN.md "Trainer, optimiser and checkpoints"):
//     alpha = lr * sqrt(1 - beta2^t) / (1 - beta1^t)
//     m += (g - m) * (1 - beta1);  v += (g * g - v) * (1 - beta2);  var -= (m * alpha) / (sqrt(v) + eps)
// The step count, the two powers and alpha live in four doubles on the device: hpe_adam_advance is one single-thread launch that moves
// them one step on, hpe_adam_apply one launch per parameter tensor that reads p, m, v, g once and writes p, m, v once.  Nothing reads the
// host, so a step is stream-ordered and capturable.  The powers are computed from t by square-and-multiply and not as running products:
// a run resumed at step N (hpe_adam_set_step) sees the bits of an uninterrupted one.
//
// The element arithmetic is float32, in the order above, under `#pragma clang fp contract(off)`; with the build's -fno-fast-math and
// hipcc's correctly rounded float divide and square root an element's result is the bits of the same lines in NumPy float32 and does
// not depend on its position, on the path it takes (16-byte vectors, the scalar tail, the all-scalar launch for a misaligned pointer)
// or on the grid.  Memory-bound: 28 bytes per element; each lane keeps two 16-byte loads per stream in flight.  No atomics, no LDS, no scratch.
//
// The guarded step (DESIGN.md "Guarded optimiser step") puts three things in front of that update.  hpe_grad_stats reduces a gradient,
// cut into segments by a table of offsets, to one record of three doubles per segment: the sum of squares, the largest |g| over the finite
// elements and the number of non-finite ones.  hpe_adam_guard, in the place of hpe_adam_advance, adds the records up, decides whether
// the step is applied, moves the state if it is and leaves the clipping scale in a guard block.  hpe_adam_apply_guarded is
// hpe_adam_apply on g * scale, and stores nothing when the step is not applied.  The order of the sums is the contract (what
// tests/grad_guard_ref.py restates): see grad_stats_chunk_kernel.  No atomics anywhere; the launches of a step are stream-ordered.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <string>

#include "hpe_ctx.h"

namespace {

constexpr int ADAM_THREADS = 256;
constexpr int ADAM_BLOCKS_PER_CU = 4;

constexpr int GS_THREADS = 256;
constexpr int GS_VECS = 16;                     // 16-byte vectors per lane and chunk
constexpr int GS_CHUNK = GS_THREADS * 4 * GS_VECS;  // 16384 elements: one workgroup, one binary tree of depth 14
constexpr int GS_RECORD = 3;                    // doubles per chunk partial and per segment: sum of squares, max |g|, non-finite count
constexpr int GS_COMBINE_TILE = 1024;           // chunk partials staged in LDS per pass of the combine
constexpr int GUARD_LISTS = 16;                 // record lists one hpe_adam_guard takes (its tensors)
// the guard block: 8 doubles
enum { GUARD_NORM = 0, GUARD_SCALE, GUARD_APPLIED, GUARD_SKIPPED, GUARD_CLIPPED, GUARD_NONFINITE, GUARD_MAXABS, GUARD_SUMSQ, GUARD_DOUBLES };

// beta^t for an integer t >= 0 by square-and-multiply, in double, in this order: what tests/adam_ref.py restates
__host__ __device__ inline double adam_pow(double beta, long long t) {
#pragma clang fp contract(off)
    double r = 1.0, b = beta;
    while (t) {
        if (t & 1) r *= b;
        b *= b;
        t >>= 1;
    }
    return r;
}

// one step on: what hpe_adam_advance does, and hpe_adam_guard when the step is applied
__device__ __forceinline__ void adam_advance_state(double* state, double lr, double beta1, double beta2) {
#pragma clang fp contract(off)
    const double t = state[0] + 1.0;
    const double p1 = adam_pow(beta1, (long long)t), p2 = adam_pow(beta2, (long long)t);
    state[0] = t;
    state[1] = p1;
    state[2] = p2;
    state[3] = lr * sqrt(1.0 - p2) / (1.0 - p1);
}

__global__ void adam_advance_kernel(double* state, double lr, double beta1, double beta2) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    adam_advance_state(state, lr, beta1, beta2);
}

// ---------------------------------------------------------------------------------------------------------- gradient statistics
// first_chunk[s] = number of chunks of the segments before s (first_chunk[S] = all): the map from a workgroup to its segment.  One
// workgroup; integers, so the order of this sum is nobody's business.
__global__ __launch_bounds__(GS_THREADS) void grad_stats_plan_kernel(const long long* __restrict__ offsets, int S, long long* __restrict__ first_chunk) {
    __shared__ long long cnt[GS_THREADS];
    __shared__ long long carry;
    const int t = threadIdx.x;
    if (t == 0) {
        carry = 0;
        first_chunk[0] = 0;
    }
    for (int base = 0; base < S; base += GS_THREADS) {
        const int s = base + t;
        __syncthreads();
        cnt[t] = s < S ? (offsets[s + 1] - offsets[s] + GS_CHUNK - 1) / GS_CHUNK : 0;
        __syncthreads();
        if (t == 0) {
            long long c = carry;
            for (int i = 0; i < GS_THREADS && base + i < S; ++i) {
                c += cnt[i];
                cnt[i] = c;
            }
            carry = c;
        }
        __syncthreads();
        if (s < S) first_chunk[s + 1] = cnt[t];
    }
}

struct GsAcc {
    double sq, mx, bad;
};

// one element: its exact square, and either its magnitude or one more non-finite element
__device__ __forceinline__ double gs_elem(float x, GsAcc& a) {
#pragma clang fp contract(off)
    const float ax = fabsf(x);
    const bool finite = ax <= FLT_MAX;  // false for an infinity and for a NaN
    a.mx = fmax(a.mx, finite ? (double)ax : 0.0);
    a.bad += finite ? 0.0 : 1.0;
    return (double)x * (double)x;
}

// one 16-byte vector of a lane: (x0^2 + x2^2) + (x1^2 + x3^2)
__device__ __forceinline__ double gs_vec(const float4& x, GsAcc& a) {
#pragma clang fp contract(off)
    const double q0 = gs_elem(x.x, a), q1 = gs_elem(x.y, a), q2 = gs_elem(x.z, a), q3 = gs_elem(x.w, a);
    return (q0 + q2) + (q1 + q3);
}

// One workgroup per chunk of GS_CHUNK elements, counted from the chunk's segment's own start.  Element e = 1024 * k + 4 * t + j of the
// chunk is component j of lane t's k-th vector, whatever path loads it: 16-byte loads for a full chunk at a 16-byte boundary, else
// scalar loads with zeros past the segment's end (x + 0.0 is x).  A lane adds a vector as above and its 16 vectors by halving (k with
// k + 8, + 4, + 2, + 1); the 256 lanes are added by halving (t with t + 128, ..., + 1).  So a chunk's partial is one fixed binary tree
// over its values and nothing else: not the grid, not the pointer, not the neighbours.
__global__ __launch_bounds__(GS_THREADS) void grad_stats_chunk_kernel(const float* __restrict__ g, const long long* __restrict__ offsets,
                                                                      const long long* __restrict__ first_chunk, int S,
                                                                      double* __restrict__ partials) {
#pragma clang fp contract(off)
    __shared__ double sh[GS_RECORD][GS_THREADS];
    const int t = threadIdx.x;
    const long long b = blockIdx.x;
    int lo = 0, hi = S;  // the last segment whose first chunk is not after b: empty segments before it share its first_chunk
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (first_chunk[mid] <= b) lo = mid;
        else hi = mid;
    }
    const long long start = offsets[lo], len = offsets[lo + 1] - start, c = b - first_chunk[lo];
    const long long left = len - c * GS_CHUNK;
    const int cnt = left < GS_CHUNK ? (int)left : GS_CHUNK;
    const float* x = g + start + c * GS_CHUNK;
    GsAcc a = {0.0, 0.0, 0.0};
    double q[GS_VECS];
    if (cnt == GS_CHUNK && ((uintptr_t)x & 15) == 0) {
        const float4* x4 = reinterpret_cast<const float4*>(x);
        float4 v[GS_VECS];
#pragma unroll
        for (int k = 0; k < GS_VECS; ++k) v[k] = x4[k * GS_THREADS + t];
#pragma unroll
        for (int k = 0; k < GS_VECS; ++k) q[k] = gs_vec(v[k], a);
    } else {
        const bool aligned = ((uintptr_t)x & 15) == 0;  // a segment's last chunk: whole vectors still take one load
#pragma unroll
        for (int k = 0; k < GS_VECS; ++k) {
            const int e = (k * GS_THREADS + t) * 4;
            float4 v;
            if (aligned && e + 3 < cnt) {
                v = *reinterpret_cast<const float4*>(x + e);
            } else {
                v.x = e < cnt ? x[e] : 0.f;
                v.y = e + 1 < cnt ? x[e + 1] : 0.f;
                v.z = e + 2 < cnt ? x[e + 2] : 0.f;
                v.w = e + 3 < cnt ? x[e + 3] : 0.f;
            }
            q[k] = gs_vec(v, a);
        }
    }
#pragma unroll
    for (int h = GS_VECS / 2; h > 0; h >>= 1) {
#pragma unroll
        for (int k = 0; k < h; ++k) q[k] = q[k] + q[k + h];
    }
    a.sq = q[0];
    sh[0][t] = a.sq;
    sh[1][t] = a.mx;
    sh[2][t] = a.bad;
    __syncthreads();
    if (t < 128) {
        sh[0][t] = sh[0][t] + sh[0][t + 128];
        sh[1][t] = fmax(sh[1][t], sh[1][t + 128]);
        sh[2][t] = sh[2][t] + sh[2][t + 128];
    }
    __syncthreads();
    if (t < 64) {  // the first wave: 64 with + 64 from LDS, then lane l with lane l + 32, ..., + 1; lane 0 holds the tree's root
        a.sq = sh[0][t] + sh[0][t + 64];
        a.mx = fmax(sh[1][t], sh[1][t + 64]);
        a.bad = sh[2][t] + sh[2][t + 64];
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            a.sq = a.sq + __shfl_down(a.sq, d);
            a.mx = fmax(a.mx, __shfl_down(a.mx, d));
            a.bad = a.bad + __shfl_down(a.bad, d);
        }
        if (t == 0) {
            double* p = partials + b * GS_RECORD;
            p[0] = a.sq;
            p[1] = a.mx;
            p[2] = a.bad;
        }
    }
}

// One workgroup per segment: its chunk partials, staged through LDS a tile at a time, added by lane 0 in index order from 0.0.
__global__ __launch_bounds__(GS_THREADS) void grad_stats_combine_kernel(const double* __restrict__ partials, const long long* __restrict__ first_chunk,
                                                                        double* __restrict__ records) {
#pragma clang fp contract(off)
    __shared__ double sh[GS_RECORD][GS_COMBINE_TILE];
    const int t = threadIdx.x;
    const long long c0 = first_chunk[blockIdx.x], nc = first_chunk[blockIdx.x + 1] - c0;
    double sq = 0.0, mx = 0.0, bad = 0.0;
    for (long long base = 0; base < nc; base += GS_COMBINE_TILE) {
        const int m = nc - base < GS_COMBINE_TILE ? (int)(nc - base) : GS_COMBINE_TILE;
        __syncthreads();
        for (int i = t; i < m; i += GS_THREADS) {
            const double* p = partials + (c0 + base + i) * GS_RECORD;
            sh[0][i] = p[0];
            sh[1][i] = p[1];
            sh[2][i] = p[2];
        }
        __syncthreads();
        if (t == 0) {
#pragma unroll 8  // the LDS reads of eight partials ahead of the one chain of additions
            for (int i = 0; i < m; ++i) {
                sq = sq + sh[0][i];
                mx = fmax(mx, sh[1][i]);
                bad = bad + sh[2][i];
            }
        }
    }
    if (t == 0) {
        double* r = records + (long long)blockIdx.x * GS_RECORD;
        r[0] = sq;
        r[1] = mx;
        r[2] = bad;
    }
}

// ------------------------------------------------------------------------------------------------------------------- the guard
struct GuardLists {
    const double* rec[GUARD_LISTS];
    int count[GUARD_LISTS];
    int n;
};

// One workgroup stages the records through LDS; lane 0 adds them in list order, then table order, and decides alone.
__global__ __launch_bounds__(GS_THREADS) void adam_guard_kernel(double* state, double* guard, GuardLists lists, double lr, double beta1, double beta2,
                                                                double clip_norm, int skip_nonfinite) {
#pragma clang fp contract(off)
    __shared__ double sh[GS_RECORD][GS_THREADS];
    const int t = threadIdx.x;
    double sumsq = 0.0, mx = 0.0, bad = 0.0;
    for (int l = 0; l < lists.n; ++l) {
        const double* rec = lists.rec[l];
        const int count = lists.count[l];
        for (int base = 0; base < count; base += GS_THREADS) {
            const int m = count - base < GS_THREADS ? count - base : GS_THREADS;
            __syncthreads();
            if (t < m) {
                const double* p = rec + (long long)(base + t) * GS_RECORD;
                sh[0][t] = p[0];
                sh[1][t] = p[1];
                sh[2][t] = p[2];
            }
            __syncthreads();
            if (t == 0) {
                for (int i = 0; i < m; ++i) {
                    sumsq = sumsq + sh[0][i];
                    mx = fmax(mx, sh[1][i]);
                    bad = bad + sh[2][i];
                }
            }
        }
    }
    if (t != 0) return;
    const double norm = sqrt(sumsq);
    guard[GUARD_SUMSQ] = sumsq;
    guard[GUARD_NORM] = norm;
    guard[GUARD_NONFINITE] = bad;
    guard[GUARD_MAXABS] = mx;
    if (skip_nonfinite && bad > 0.0) {  // the state keeps its bits: t does not move
        guard[GUARD_APPLIED] = 0.0;
        guard[GUARD_SCALE] = 0.0;
        guard[GUARD_SKIPPED] = guard[GUARD_SKIPPED] + 1.0;
        return;
    }
    adam_advance_state(state, lr, beta1, beta2);
    // clip_norm / fmax(norm, clip_norm): exactly 1 for norm <= clip_norm, for clip_norm = +inf, and for a NaN norm (fmax drops it)
    const float scale = norm > clip_norm ? (float)(clip_norm / norm) : 1.0f;
    guard[GUARD_APPLIED] = 1.0;
    guard[GUARD_SCALE] = (double)scale;
    if (scale < 1.0f) guard[GUARD_CLIPPED] = guard[GUARD_CLIPPED] + 1.0;
}

__global__ void adam_set_step_kernel(double* state, long long t, double beta1, double beta2) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    state[0] = (double)t;
    state[1] = adam_pow(beta1, t);
    state[2] = adam_pow(beta2, t);
    state[3] = 0.0;  // alpha belongs to a step: the next hpe_adam_advance writes it
}

// the four operations of ResourceApplyAdam on one element
__device__ __forceinline__ void adam_elem(float& p, float& m, float& v, float g, float alpha, float omb1, float omb2, float eps) {
#pragma clang fp contract(off)
    m = m + (g - m) * omb1;
    v = v + (g * g - v) * omb2;
    p = p - (m * alpha) / (sqrtf(v) + eps);
}

__device__ __forceinline__ void adam_vec(float4& p, float4& m, float4& v, const float4& g, float alpha, float omb1, float omb2, float eps) {
    adam_elem(p.x, m.x, v.x, g.x, alpha, omb1, omb2, eps);
    adam_elem(p.y, m.y, v.y, g.y, alpha, omb1, omb2, eps);
    adam_elem(p.z, m.z, v.z, g.z, alpha, omb1, omb2, eps);
    adam_elem(p.w, m.w, v.w, g.w, alpha, omb1, omb2, eps);
}

// The guarded step's gradient: g * scale, one float32 multiply and one rounding; g itself when scale is 1.0f.  GUARDED = false (hpe_adam_apply)
// reads no guard block and multiplies nothing.
template <bool GUARDED>
__device__ __forceinline__ float guarded_g(float g, float scale) {
#pragma clang fp contract(off)
    if constexpr (GUARDED) return g * scale;
    else return g;
}

template <bool GUARDED>
__device__ __forceinline__ float4 guarded_g4(const float4& g, float scale) {
    return make_float4(guarded_g<GUARDED>(g.x, scale), guarded_g<GUARDED>(g.y, scale), guarded_g<GUARDED>(g.z, scale), guarded_g<GUARDED>(g.w, scale));
}

// all four pointers 16-byte aligned: n4 = n / 4 vectors in a grid-stride loop, two vectors per lane and stream in flight; the last n % 4
// elements are the first lanes of block 0.  GUARDED: a step that is not applied returns before any load of p, m, v and stores nothing.
template <bool GUARDED>
__global__ __launch_bounds__(ADAM_THREADS) void adam_apply_vec_kernel(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                                                      const float* __restrict__ g, long long n, const double* __restrict__ state,
                                                                      const double* __restrict__ guard, float omb1, float omb2, float eps) {
    float scale = 1.0f;
    if constexpr (GUARDED) {
        if (guard[GUARD_APPLIED] == 0.0) return;
        scale = (float)guard[GUARD_SCALE];
    }
    const float alpha = (float)state[3];
    const size_t n4 = (size_t)n >> 2;
    const size_t stride = (size_t)gridDim.x * ADAM_THREADS;
    float4* p4 = reinterpret_cast<float4*>(p);
    float4* m4 = reinterpret_cast<float4*>(m);
    float4* v4 = reinterpret_cast<float4*>(v);
    const float4* g4 = reinterpret_cast<const float4*>(g);
    size_t i = (size_t)blockIdx.x * ADAM_THREADS + threadIdx.x;
    for (; i + stride < n4; i += 2 * stride) {
        const size_t j = i + stride;
        float4 pa = p4[i], ma = m4[i], va = v4[i];
        const float4 ga = guarded_g4<GUARDED>(g4[i], scale);
        float4 pb = p4[j], mb = m4[j], vb = v4[j];
        const float4 gb = guarded_g4<GUARDED>(g4[j], scale);
        adam_vec(pa, ma, va, ga, alpha, omb1, omb2, eps);
        adam_vec(pb, mb, vb, gb, alpha, omb1, omb2, eps);
        p4[i] = pa;
        m4[i] = ma;
        v4[i] = va;
        p4[j] = pb;
        m4[j] = mb;
        v4[j] = vb;
    }
    if (i < n4) {
        float4 pa = p4[i], ma = m4[i], va = v4[i];
        const float4 ga = guarded_g4<GUARDED>(g4[i], scale);
        adam_vec(pa, ma, va, ga, alpha, omb1, omb2, eps);
        p4[i] = pa;
        m4[i] = ma;
        v4[i] = va;
    }
    if (blockIdx.x == 0) {
        const size_t e = (n4 << 2) + threadIdx.x;
        if (threadIdx.x < 4 && e < (size_t)n) {
            float pe = p[e], me = m[e], ve = v[e];
            adam_elem(pe, me, ve, guarded_g<GUARDED>(g[e], scale), alpha, omb1, omb2, eps);
            p[e] = pe;
            m[e] = me;
            v[e] = ve;
        }
    }
}

// some pointer is not 16-byte aligned: every element alone
template <bool GUARDED>
__global__ __launch_bounds__(ADAM_THREADS) void adam_apply_scalar_kernel(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                                                         const float* __restrict__ g, long long n, const double* __restrict__ state,
                                                                         const double* __restrict__ guard, float omb1, float omb2, float eps) {
    float scale = 1.0f;
    if constexpr (GUARDED) {
        if (guard[GUARD_APPLIED] == 0.0) return;
        scale = (float)guard[GUARD_SCALE];
    }
    const float alpha = (float)state[3];
    const size_t stride = (size_t)gridDim.x * ADAM_THREADS;
    for (size_t e = (size_t)blockIdx.x * ADAM_THREADS + threadIdx.x; e < (size_t)n; e += stride) {
        float pe = p[e], me = m[e], ve = v[e];
        adam_elem(pe, me, ve, guarded_g<GUARDED>(g[e], scale), alpha, omb1, omb2, eps);
        p[e] = pe;
        m[e] = me;
        v[e] = ve;
    }
}

bool beta_ok(double b) { return std::isfinite(b) && b >= 0.0 && b < 1.0; }

// a few workgroups per compute unit, never more than the work items ask for
int adam_grid(long long items, int* blocks_out) {
    static int cus = 0;  // asked once (every gfx950 of a node has the same count); a race writes the same value twice
    if (cus == 0) {
        int dev = 0, n = 0;
        HIP_TRY(hipGetDevice(&dev));
        HIP_TRY(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev));
        cus = n > 0 ? n : 256;
    }
    const long long want = (items + ADAM_THREADS - 1) / ADAM_THREADS;
    const long long cap = (long long)(cus > 0 ? cus : 256) * ADAM_BLOCKS_PER_CU;
    *blocks_out = (int)(want < 1 ? 1 : (want < cap ? want : cap));
    return HPE_OK;
}

// the launch of hpe_adam_apply and of hpe_adam_apply_guarded: the same choice of path and grid
template <bool GUARDED>
int adam_apply_launch(float* p, float* m, float* v, const float* g, long long n, const double* state_dev, const double* guard_dev, float omb1,
                      float omb2, float eps, void* stream) {
    const bool aligned = ((((uintptr_t)p | (uintptr_t)m | (uintptr_t)v | (uintptr_t)g) & 15) == 0) && n >= 4;
    int blocks = 1;
    if (aligned) {
        // two vectors per lane and pass
        if (int rc = adam_grid(((n >> 2) + 1) / 2, &blocks)) return rc;
        hipLaunchKernelGGL(adam_apply_vec_kernel<GUARDED>, dim3(blocks), dim3(ADAM_THREADS), 0, static_cast<hipStream_t>(stream), p, m, v, g, n,
                           state_dev, guard_dev, omb1, omb2, eps);
    } else {
        if (int rc = adam_grid(n, &blocks)) return rc;
        hipLaunchKernelGGL(adam_apply_scalar_kernel<GUARDED>, dim3(blocks), dim3(ADAM_THREADS), 0, static_cast<hipStream_t>(stream), p, m, v, g, n,
                           state_dev, guard_dev, omb1, omb2, eps);
    }
    HIP_TRY(hipGetLastError());
    return HPE_OK;
}

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int hpe_adam_advance(double* state_dev, double lr, double beta1, double beta2, void* stream) {
    if (!state_dev) return fail(HPE_ERR_INVALID, "null argument");
    if (!std::isfinite(lr)) return fail(HPE_ERR_INVALID, "lr must be finite");
    if (!beta_ok(beta1) || !beta_ok(beta2)) return fail(HPE_ERR_INVALID, "beta1 and beta2 must be in [0, 1)");
    hipLaunchKernelGGL(adam_advance_kernel, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), state_dev, lr, beta1, beta2);
    HIP_TRY(hipGetLastError());
    return HPE_OK;
}

int hpe_adam_set_step(double* state_dev, long long t, double beta1, double beta2, void* stream) {
    if (!state_dev) return fail(HPE_ERR_INVALID, "null argument");
    if (t < 0 || t > (1LL << 53)) return fail(HPE_ERR_INVALID, "t must be in [0, 2^53]");
    if (!beta_ok(beta1) || !beta_ok(beta2)) return fail(HPE_ERR_INVALID, "beta1 and beta2 must be in [0, 1)");
    hipLaunchKernelGGL(adam_set_step_kernel, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), state_dev, t, beta1, beta2);
    HIP_TRY(hipGetLastError());
    return HPE_OK;
}

int hpe_adam_apply(float* p, float* m, float* v, const float* g, long long n, const double* state_dev, float one_minus_beta1,
                   float one_minus_beta2, float eps, void* stream) {
    if (!p || !m || !v || !g || !state_dev) return fail(HPE_ERR_INVALID, "null argument");
    if (n < 0) return fail(HPE_ERR_INVALID, "n must be >= 0");
    if (n == 0) return HPE_OK;
    return adam_apply_launch<false>(p, m, v, g, n, state_dev, nullptr, one_minus_beta1, one_minus_beta2, eps, stream);
}

int hpe_adam_apply_guarded(float* p, float* m, float* v, const float* g, long long n, const double* state_dev, const double* guard_dev,
                           float one_minus_beta1, float one_minus_beta2, float eps, void* stream) {
    if (!p || !m || !v || !g || !state_dev || !guard_dev) return fail(HPE_ERR_INVALID, "null argument");
    if (n < 0) return fail(HPE_ERR_INVALID, "n must be >= 0");
    if (n == 0) return HPE_OK;
    return adam_apply_launch<true>(p, m, v, g, n, state_dev, guard_dev, one_minus_beta1, one_minus_beta2, eps, stream);
}

int hpe_grad_stats_chunk(void) { return GS_CHUNK; }

long long hpe_grad_stats_workspace_bytes(long long n, int S) {
    if (n < 0 || S < 1) {
        fail(HPE_ERR_INVALID, "hpe_grad_stats_workspace_bytes: n must be >= 0 and S >= 1");
        return -1;
    }
    // the first-chunk table, then one partial per chunk: a segment ends in at most one chunk that is not full
    return (long long)sizeof(long long) * (S + 1) + (long long)sizeof(double) * GS_RECORD * (n / GS_CHUNK + S);
}

int hpe_grad_stats(const float* g, long long n, const long long* offsets_host, const long long* offsets_dev, int S, double* records_dev,
                   void* workspace_dev, long long workspace_bytes, void* stream) {
    if (!g || !offsets_host || !offsets_dev || !records_dev || !workspace_dev) return fail(HPE_ERR_INVALID, "null argument");
    if (n < 0) return fail(HPE_ERR_INVALID, "n must be >= 0");
    if (S < 1) return fail(HPE_ERR_INVALID, "S must be >= 1");
    if (offsets_host[0] < 0) return fail(HPE_ERR_INVALID, "offsets[0] must be >= 0");
    long long chunks = 0;
    for (int s = 0; s < S; ++s) {
        if (offsets_host[s + 1] < offsets_host[s])
            return fail(HPE_ERR_INVALID, "offsets must ascend: offsets[" + std::to_string(s + 1) + "] < offsets[" + std::to_string(s) + "]");
        chunks += (offsets_host[s + 1] - offsets_host[s] + GS_CHUNK - 1) / GS_CHUNK;
    }
    if (offsets_host[S] > n)
        return fail(HPE_ERR_INVALID, "offsets[" + std::to_string(S) + "] = " + std::to_string(offsets_host[S]) + " is beyond n = " + std::to_string(n));
    const long long need = hpe_grad_stats_workspace_bytes(n, S);
    if (workspace_bytes < need)
        return fail(HPE_ERR_INVALID, "workspace of " + std::to_string(workspace_bytes) + " bytes, hpe_grad_stats_workspace_bytes asks for " + std::to_string(need));
    if (((uintptr_t)workspace_dev & 7) != 0) return fail(HPE_ERR_INVALID, "workspace must be 8-byte aligned");
    if (chunks > 0x7fffffffLL) return fail(HPE_ERR_INVALID, "more than 2^31 - 1 chunks");
    long long* first_chunk = static_cast<long long*>(workspace_dev);
    double* partials = reinterpret_cast<double*>(first_chunk + (S + 1));
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(grad_stats_plan_kernel, dim3(1), dim3(GS_THREADS), 0, st, offsets_dev, S, first_chunk);
    HIP_TRY(hipGetLastError());
    if (chunks > 0) {
        hipLaunchKernelGGL(grad_stats_chunk_kernel, dim3((unsigned)chunks), dim3(GS_THREADS), 0, st, g, offsets_dev, first_chunk, S, partials);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(grad_stats_combine_kernel, dim3(S), dim3(GS_THREADS), 0, st, partials, first_chunk, records_dev);
    HIP_TRY(hipGetLastError());
    return HPE_OK;
}

int hpe_adam_guard(double* state_dev, double* guard_dev, const double* const* records_dev, const int* counts, int n_lists, double lr,
                   double beta1, double beta2, double clip_norm, int skip_nonfinite, void* stream) {
    if (!state_dev || !guard_dev || !records_dev || !counts) return fail(HPE_ERR_INVALID, "null argument");
    if (n_lists < 1 || n_lists > GUARD_LISTS) return fail(HPE_ERR_INVALID, "n_lists must be in [1, " + std::to_string(GUARD_LISTS) + "]");
    if (!std::isfinite(lr)) return fail(HPE_ERR_INVALID, "lr must be finite");
    if (!beta_ok(beta1) || !beta_ok(beta2)) return fail(HPE_ERR_INVALID, "beta1 and beta2 must be in [0, 1)");
    if (!(clip_norm >= 0.0)) return fail(HPE_ERR_INVALID, "clip_norm must be >= 0 (+inf: no clipping), not negative or NaN");
    GuardLists lists = {};
    for (int l = 0; l < n_lists; ++l) {
        if (!records_dev[l]) return fail(HPE_ERR_INVALID, "null argument: records list " + std::to_string(l));
        if (counts[l] < 1) return fail(HPE_ERR_INVALID, "records list " + std::to_string(l) + " must hold at least one record");
        lists.rec[l] = records_dev[l];
        lists.count[l] = counts[l];
    }
    lists.n = n_lists;
    hipLaunchKernelGGL(adam_guard_kernel, dim3(1), dim3(GS_THREADS), 0, static_cast<hipStream_t>(stream), state_dev, guard_dev, lists, lr, beta1,
                       beta2, clip_norm, skip_nonfinite);
    HIP_TRY(hipGetLastError());
    return HPE_OK;
}

int hpe_debug_adam_power(double beta, long long t, double* out) {
    if (!out) return fail(HPE_ERR_INVALID, "null argument");
    if (t < 0) return fail(HPE_ERR_INVALID, "t must be >= 0");
    *out = adam_pow(beta, t);
    return HPE_OK;
}

}  // extern "C"
#pragma GCC visibility pop
