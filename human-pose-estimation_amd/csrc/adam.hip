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
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "hpe_ctx.h"

namespace {

constexpr int ADAM_THREADS = 256;
constexpr int ADAM_BLOCKS_PER_CU = 4;

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

__global__ void adam_advance_kernel(double* state, double lr, double beta1, double beta2) {
#pragma clang fp contract(off)
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const double t = state[0] + 1.0;
    const double p1 = adam_pow(beta1, (long long)t), p2 = adam_pow(beta2, (long long)t);
    state[0] = t;
    state[1] = p1;
    state[2] = p2;
    state[3] = lr * sqrt(1.0 - p2) / (1.0 - p1);
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

// all four pointers 16-byte aligned: n4 = n / 4 vectors in a grid-stride loop, two vectors per lane and stream in flight; the last n % 4
// elements are the first lanes of block 0
__global__ __launch_bounds__(ADAM_THREADS) void adam_apply_vec_kernel(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                                                      const float* __restrict__ g, long long n, const double* __restrict__ state,
                                                                      float omb1, float omb2, float eps) {
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
        const float4 ga = g4[i];
        float4 pb = p4[j], mb = m4[j], vb = v4[j];
        const float4 gb = g4[j];
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
        const float4 ga = g4[i];
        adam_vec(pa, ma, va, ga, alpha, omb1, omb2, eps);
        p4[i] = pa;
        m4[i] = ma;
        v4[i] = va;
    }
    if (blockIdx.x == 0) {
        const size_t e = (n4 << 2) + threadIdx.x;
        if (threadIdx.x < 4 && e < (size_t)n) {
            float pe = p[e], me = m[e], ve = v[e];
            adam_elem(pe, me, ve, g[e], alpha, omb1, omb2, eps);
            p[e] = pe;
            m[e] = me;
            v[e] = ve;
        }
    }
}

// some pointer is not 16-byte aligned: every element alone
__global__ __launch_bounds__(ADAM_THREADS) void adam_apply_scalar_kernel(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                                                         const float* __restrict__ g, long long n, const double* __restrict__ state,
                                                                         float omb1, float omb2, float eps) {
    const float alpha = (float)state[3];
    const size_t stride = (size_t)gridDim.x * ADAM_THREADS;
    for (size_t e = (size_t)blockIdx.x * ADAM_THREADS + threadIdx.x; e < (size_t)n; e += stride) {
        float pe = p[e], me = m[e], ve = v[e];
        adam_elem(pe, me, ve, g[e], alpha, omb1, omb2, eps);
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
    const bool aligned = ((((uintptr_t)p | (uintptr_t)m | (uintptr_t)v | (uintptr_t)g) & 15) == 0) && n >= 4;
    int blocks = 1;
    if (aligned) {
        // two vectors per lane and pass
        if (int rc = adam_grid(((n >> 2) + 1) / 2, &blocks)) return rc;
        hipLaunchKernelGGL(adam_apply_vec_kernel, dim3(blocks), dim3(ADAM_THREADS), 0, static_cast<hipStream_t>(stream), p, m, v, g, n,
                           state_dev, one_minus_beta1, one_minus_beta2, eps);
    } else {
        if (int rc = adam_grid(n, &blocks)) return rc;
        hipLaunchKernelGGL(adam_apply_scalar_kernel, dim3(blocks), dim3(ADAM_THREADS), 0, static_cast<hipStream_t>(stream), p, m, v, g, n,
                           state_dev, one_minus_beta1, one_minus_beta2, eps);
    }
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
