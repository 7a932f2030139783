// encoder_bn_bf16.hip -- BatchNorm with the statistics of the batch on bf16 tensors, for the mixed-precision encoder walk with batch
// statistics (encoder_train.hip, the walks at T = bf16e; DESIGN.md section 4, "Mixed-precision encoder training with batch statistics"):
// the bf16 forms of the four memory passes of encoder_bn.hip, launched by the cmx16 / mx16 overloads of its bn_launch_* functions with its
// geometry (bn_geom, bn_bad_shape) at eight channels a thread.  Per layer, z16 [M][N] = RNE(conv(x16, W16) + b), M = B * hout * hout:
//
//   forward    mu, var, r of z16 (what is normalised is what was measured)    y16 = RNE(act(gamma * ((z16 - mu) * r) + beta (+ res16)))
//   backward   dz = dy16 * [y16 > 0] (exact)    xhat = (z16 - mu) * r    dbeta = sum_m dz    dgamma = sum_m dz * xhat
//              dzraw16 = RNE(gamma * r * (dz - dbeta / M - xhat * dgamma / M))
//
// The arithmetic is fp32 in the order of the fp32 kernels, with one rounding to bf16 where a tensor is written, and no product is fused
// into a sum (fp contract off), so a float32 restatement of these lines gives the same bits.  The sums are double: a bf16 value, its
// square and the product of a bf16 dz with a float xhat are all exact in double.
//
// bn_stats_bf16_kernel / bn_bwd_reduce_bf16_kernel: a thread owns EIGHT consecutive channels (one 16-byte load per row and operand) and
// walks the rows of its slice of the pixel axis with 16 double accumulators, eight (stats) or four (backward, three operands) rows in
// flight, added in the order of the plain loop.  The row lanes of a workgroup are added in ascending order through LDS, the sums first
// and the second moments after them through the same 16 KiB.  Each slice writes its partial in the layout of encoder_bn.hip,
// part[slice][2][N], within BN_MAX_SLICES and BN_PART_COLS, so the finish kernels of encoder_bn.hip (and with them the split for
// data-parallel training) run unchanged behind these.  No atomics.  bn_apply_bf16_kernel / bn_bwd_apply_bf16_kernel are elementwise,
// eight channels a thread.  N is a multiple of 64 on every layer; rows past M are never read.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "hpe_ctx.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// eight floats of a 16-byte aligned per-channel array / of one that is only float-aligned (the caller's gradient)
__device__ __forceinline__ void load8(const float* __restrict__ p, int c8, float (&o)[8]) {
    const f32x4 a = reinterpret_cast<const f32x4*>(p)[2 * c8], b = reinterpret_cast<const f32x4*>(p)[2 * c8 + 1];
    o[0] = a.x, o[1] = a.y, o[2] = a.z, o[3] = a.w, o[4] = b.x, o[5] = b.y, o[6] = b.z, o[7] = b.w;
}
__device__ __forceinline__ void load8_unaligned(const float* __restrict__ p, int c8, float (&o)[8]) {
#pragma unroll
    for (int u = 0; u < 8; ++u) o[u] = p[8 * c8 + u];
}

// acc[0..7] / acc[8..15] of the workgroup's row lanes, added in ascending lane order; lane 0 of every column writes part[slice][0 / 1][N].
// Every thread of the workgroup arrives here
__device__ inline void bn_block_reduce_bf16(const double (&acc)[16], int cg, int rows, int N, double* __restrict__ part) {
    __shared__ double red[8][256];
    const int t = threadIdx.x, col = t % cg, ry = t / cg;
    const int n = (blockIdx.x * cg + col) * 8;
    double* out = part + (size_t)blockIdx.y * 2 * N + n;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        if (h) __syncthreads();
#pragma unroll
        for (int j = 0; j < 8; ++j) red[j][t] = acc[8 * h + j];
        __syncthreads();
        if (ry == 0) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                double s = red[j][col];
                for (int q = 1; q < rows; ++q) s += red[j][q * cg + col];
                out[h * N + j] = s;
            }
        }
    }
}

// part[slice][0][n] = sum over the slice's rows of z16, part[slice][1][n] = of z16^2.  grid (gx, slices), 256 threads = rows x cg
__global__ __launch_bounds__(256) void bn_stats_bf16_kernel(const bf16x8* __restrict__ z, int M, int N, int cg, int rows, int P,
                                                            double* __restrict__ part) {
    const int col = threadIdx.x % cg, ry = threadIdx.x / cg;
    const int n8 = N / 8, c8 = blockIdx.x * cg + col;
    const int m_end = min(M, ((int)blockIdx.y + 1) * P);
    double acc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 0.0;
    auto add = [&](const bf16x8 v) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const double a = (double)(float)v[u];
            acc[u] += a;
            acc[8 + u] += a * a;
        }
    };
    int m = blockIdx.y * P + ry;
    for (; m + 7 * rows < m_end; m += 8 * rows) {  // eight rows in flight, added in the order of the plain loop
        bf16x8 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = z[(size_t)(m + u * rows) * n8 + c8];
#pragma unroll
        for (int u = 0; u < 8; ++u) add(v[u]);
    }
    for (; m < m_end; m += rows) add(z[(size_t)m * n8 + c8]);
    bn_block_reduce_bf16(acc, cg, rows, N, part);
}

// y16 = RNE(act(gamma * ((z16 - mu) * r) + beta (+ res16))): bn_apply_kernel's expression, the residual added in fp32 before the one
// rounding; n8 groups of eight, N8 = N / 8
__global__ __launch_bounds__(256) void bn_apply_bf16_kernel(const bf16x8* __restrict__ z, const float* __restrict__ mu, const float* __restrict__ r,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            const bf16x8* __restrict__ res, int relu, bf16x8* __restrict__ y, long n8, int N8) {
#pragma clang fp contract(off)
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n8) return;
    const int c = (int)(i % N8);
    float m8[8], r8[8], g8[8], b8[8];
    load8(mu, c, m8), load8(r, c, r8), load8(gamma, c, g8), load8(beta, c, b8);
    const bf16x8 zz = z[i];
    bf16x8 rr;
    if (res) rr = res[i];
    bf16x8 o;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        float v = g8[u] * (((float)zz[u] - m8[u]) * r8[u]) + b8[u];
        if (res) v += (float)rr[u];
        if (relu) v = v > 0.f ? v : 0.f;
        o[u] = (__bf16)v;
    }
    y[i] = o;
}

// part[slice][0][n] = sum over the slice's rows of dz = dy16 * [y16 > 0] (y == nullptr: dz = dy16), part[slice][1][n] = of dz * xhat
__global__ __launch_bounds__(256) void bn_bwd_reduce_bf16_kernel(const bf16x8* __restrict__ dy, const bf16x8* __restrict__ y,
                                                                 const bf16x8* __restrict__ z, const float* __restrict__ mu,
                                                                 const float* __restrict__ r, int M, int N, int cg, int rows, int P,
                                                                 double* __restrict__ part) {
#pragma clang fp contract(off)
    const int col = threadIdx.x % cg, ry = threadIdx.x / cg;
    const int n8 = N / 8, c8 = blockIdx.x * cg + col;
    const int m_end = min(M, ((int)blockIdx.y + 1) * P);
    float m8[8], r8[8];
    load8(mu, c8, m8), load8(r, c8, r8);
    double acc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 0.0;
    auto add = [&](const bf16x8 d, const bf16x8 a, const bf16x8 zz) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const float dz = (!y || (float)a[u] > 0.f) ? (float)d[u] : 0.f;
            const float xh = ((float)zz[u] - m8[u]) * r8[u];
            acc[u] += (double)dz;
            acc[8 + u] += (double)dz * (double)xh;
        }
    };
    int m = blockIdx.y * P + ry;
    for (; m + 3 * rows < m_end; m += 4 * rows) {  // four rows of three operands in flight, added in the order of the plain loop
        bf16x8 d[4], a[4], zz[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const size_t i = (size_t)(m + u * rows) * n8 + c8;
            d[u] = dy[i];
            a[u] = y ? y[i] : d[u];
            zz[u] = z[i];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) add(d[u], a[u], zz[u]);
    }
    for (; m < m_end; m += rows) {
        const size_t i = (size_t)m * n8 + c8;
        const bf16x8 d = dy[i];
        add(d, y ? y[i] : d, z[i]);
    }
    bn_block_reduce_bf16(acc, cg, rows, N, part);
}

// dz = dy16 * [y16 > 0] (y == nullptr: dz = dy16), exact, and dzraw16 = RNE(gamma * r * (dz - dbeta / M - xhat * (dgamma / M))):
// bn_bwd_apply_kernel's expression.  dz may be nullptr and may alias dy; dgamma / dbeta are only float-aligned
__global__ __launch_bounds__(256) void bn_bwd_apply_bf16_kernel(const bf16x8* dy, const bf16x8* __restrict__ y, const bf16x8* __restrict__ z,
                                                                const float* __restrict__ mu, const float* __restrict__ r,
                                                                const float* __restrict__ gamma, const float* __restrict__ dgamma,
                                                                const float* __restrict__ dbeta, float M, bf16x8* dz, bf16x8* __restrict__ dzraw,
                                                                long n8, int N8) {
#pragma clang fp contract(off)
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n8) return;
    const int c = (int)(i % N8);
    float m8[8], r8[8], g8[8], dg8[8], db8[8];
    load8(mu, c, m8), load8(r, c, r8), load8(gamma, c, g8);
    load8_unaligned(dgamma, c, dg8), load8_unaligned(dbeta, c, db8);
    bf16x8 d = dy[i];
    const bf16x8 zz = z[i];
    if (y) {
        const bf16x8 a = y[i];
#pragma unroll
        for (int u = 0; u < 8; ++u) d[u] = (float)a[u] > 0.f ? d[u] : (__bf16)0.f;
    }
    if (dz) dz[i] = d;
    bf16x8 o;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const float xh = ((float)zz[u] - m8[u]) * r8[u];
        o[u] = (__bf16)(g8[u] * r8[u] * ((float)d[u] - db8[u] / M - xh * (dg8[u] / M)));
    }
    dzraw[i] = o;
}

const bf16x8* v8(cmx16 p) { return reinterpret_cast<const bf16x8*>(p); }
bf16x8* v8(mx16 p) { return reinterpret_cast<bf16x8*>(p); }

constexpr int VEC = 8;  // channels a thread
bool bad_shape(long M, int N) { return bn_bad_shape(M, N, VEC); }

hipError_t launch_stats(cmx16 z, int M, int N, double* part, int* slices, hipStream_t st) {
    if (bad_shape(M, N)) return hipErrorInvalidValue;
    const BnGeom g = bn_geom(M, N, VEC);
    hipLaunchKernelGGL(bn_stats_bf16_kernel, dim3(g.gx, g.slices), dim3(256), 0, st, v8(z), M, N, g.cg, g.rows, g.P, part);
    *slices = g.slices;
    return hipGetLastError();
}

hipError_t launch_bwd_reduce(cmx16 dy, cmx16 y, cmx16 z, const float* mu, const float* r, int M, int N, double* part, int* slices, hipStream_t st) {
    if (bad_shape(M, N)) return hipErrorInvalidValue;
    const BnGeom g = bn_geom(M, N, VEC);
    hipLaunchKernelGGL(bn_bwd_reduce_bf16_kernel, dim3(g.gx, g.slices), dim3(256), 0, st, v8(dy), v8(y), v8(z), mu, r, M, N, g.cg, g.rows, g.P, part);
    *slices = g.slices;
    return hipGetLastError();
}

}  // namespace

hipError_t bn_launch_stats(cmx16 z, int M, int N, float eps, double* part, float* mu, float* var, float* r, hipStream_t st) {
    int slices;
    hipError_t e = launch_stats(z, M, N, part, &slices, st);
    return e != hipSuccess ? e : bn_finish_stats(part, slices, M, N, eps, mu, var, r, st);
}

hipError_t bn_launch_stats_sums(cmx16 z, int M, int N, double* part, double* sums, hipStream_t st) {
    int slices;
    hipError_t e = launch_stats(z, M, N, part, &slices, st);
    return e != hipSuccess ? e : bn_finish_sums(part, slices, N, sums, st);
}

hipError_t bn_launch_apply(cmx16 z, const float* mu, const float* r, const float* gamma, const float* beta, cmx16 res, int relu, mx16 y, int M, int N,
                           hipStream_t st) {
    if (bad_shape(M, N)) return hipErrorInvalidValue;
    const long n8 = (long)M * (N / 8);
    hipLaunchKernelGGL(bn_apply_bf16_kernel, grid1(n8), dim3(256), 0, st, v8(z), mu, r, gamma, beta, v8(res), relu, v8(y), n8, N / 8);
    return hipGetLastError();
}

hipError_t bn_launch_bwd_reduce(cmx16 dy, cmx16 y, cmx16 z, const float* mu, const float* r, int M, int N, double* part, float* db, float* dgamma,
                                float* dbeta, hipStream_t st) {
    int slices;
    hipError_t e = launch_bwd_reduce(dy, y, z, mu, r, M, N, part, &slices, st);
    return e != hipSuccess ? e : bn_finish_bwd(part, slices, N, db, dgamma, dbeta, st);
}

hipError_t bn_launch_bwd_sums(cmx16 dy, cmx16 y, cmx16 z, const float* mu, const float* r, int M, int N, double* part, double* sums, float* db,
                              float* dgamma, float* dbeta, hipStream_t st) {
    int slices;
    hipError_t e = launch_bwd_reduce(dy, y, z, mu, r, M, N, part, &slices, st);
    return e != hipSuccess ? e : bn_finish_bwd_sums(part, slices, N, sums, db, dgamma, dbeta, st);
}

hipError_t bn_launch_bwd_apply(cmx16 dy, cmx16 y, cmx16 z, const float* mu, const float* r, const float* gamma, const float* dgamma, const float* dbeta,
                               int M, int N, mx16 dz, mx16 dzraw, hipStream_t st, double M_all) {
    if (bad_shape(M, N)) return hipErrorInvalidValue;
    const long n8 = (long)M * (N / 8);
    hipLaunchKernelGGL(bn_bwd_apply_bf16_kernel, grid1(n8), dim3(256), 0, st, v8(dy), v8(y), v8(z), mu, r, gamma, dgamma, dbeta,
                       M_all > 0.0 ? (float)M_all : (float)M, v8(dz), v8(dzraw), n8, N / 8);
    return hipGetLastError();
}
