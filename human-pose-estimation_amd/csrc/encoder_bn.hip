// encoder_bn.hip -- BatchNorm with the statistics of the batch (Keras' training=True, src/trainer.py:386), for encoder training: the
// bandwidth-bound kernels around the convolutions.  Per layer, z [M][N] = conv(x, W) + b (NHWC rows, M = B * hout * hout):
//
//   forward    mu = mean_m z    var = mean_m (z - mu)^2    r = 1 / sqrt(var + eps)    xhat = (z - mu) * r    y = act(gamma * xhat + beta (+ res))
//   backward   dz = dy * [y > 0]    dbeta = sum_m dz    dgamma = sum_m dz * xhat    dzraw = gamma * r * (dz - dbeta / M - xhat * dgamma / M)
//
// bn_stats_kernel / bn_bwd_reduce_kernel: the two column sums of a layer.  A thread owns four consecutive channels (one 16-byte load per
// row and operand) and walks the rows of its slice of the pixel axis with double accumulators; the row lanes of a workgroup are added
// in ascending order through LDS, each slice writes its partial, the finish kernels add the slices in a fixed order (16 interleaved
// ascending sums per channel, then those ascending).  No atomics:
// the same inputs give the same bits.  The variance is E[z^2] - mu^2 in double (z^2 is exact in double, so the cancellation costs
// nothing a float sees until mu^2 / var nears 2^29).  bn_apply_kernel / bn_bwd_apply_kernel are elementwise, one f32x4 per thread.
// bn_momentum_kernel moves the whole statistics tensor [mean of every channel | variance of every channel] in one launch;
// bn_install_kernel rewrites what the frozen path folds (mean, sqrt(var + eps) in double, its reciprocal) from such a tensor.
// Data-parallel training cuts both reductions where the ranks meet: bn_sums_kernel / bn_bwd_sums_kernel leave the column sums of this
// rank's rows as [2][N] doubles (added over the slices in the finish kernels' order), the caller adds the other ranks' to them, and
// bn_stats_from_sums_kernel / bn_bwd_from_sums_kernel finish from the sums over all M rows with the arithmetic of the one-rank finish.
// N is a multiple of 64 on every layer; rows past M are never read.
// bn_geom and bn_bad_shape (the slicing and the shapes taken, at `vec` channels a thread) and the finish launches serve the bf16 first
// stages of encoder_bn_bf16.hip too, whose launchers are overloads of the ones here.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "hpe_ctx.h"

namespace {

// acc[0..3] / acc[4..7] of the workgroup's row lanes, added in ascending lane order; lane 0 of every column writes part[slice][0 / 1][N]
__device__ inline void bn_block_reduce(const double (&acc)[8], int cg, int rows, int N, double* __restrict__ part) {
    __shared__ double red[8][256];
    const int t = threadIdx.x, col = t % cg, ry = t / cg;
#pragma unroll
    for (int j = 0; j < 8; ++j) red[j][t] = acc[j];
    __syncthreads();
    if (ry != 0) return;
    const int n = (blockIdx.x * cg + col) * 4;
    double* out = part + (size_t)blockIdx.y * 2 * N + n;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        double s = red[j][col];
        for (int q = 1; q < rows; ++q) s += red[j][q * cg + col];
        out[(j >> 2) * N + (j & 3)] = s;
    }
}

// part[slice][0][n] = sum over the slice's rows of z, part[slice][1][n] = of z^2.  grid (gx, slices), 256 threads = rows x cg
__global__ __launch_bounds__(256) void bn_stats_kernel(const f32x4* __restrict__ z, int M, int N, int cg, int rows, int P, double* __restrict__ part) {
    const int col = threadIdx.x % cg, ry = threadIdx.x / cg;
    const int n4 = N / 4, c4 = blockIdx.x * cg + col;
    const int m_end = min(M, ((int)blockIdx.y + 1) * P);
    double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    auto add = [&](const f32x4 v) {
        const double a = v.x, b = v.y, c = v.z, d = v.w;
        acc[0] += a, acc[1] += b, acc[2] += c, acc[3] += d;
        acc[4] += a * a, acc[5] += b * b, acc[6] += c * c, acc[7] += d * d;
    };
    int m = blockIdx.y * P + ry;
    for (; m + 3 * rows < m_end; m += 4 * rows) {  // four rows in flight, added in the order of the plain loop
        f32x4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = z[(size_t)(m + u * rows) * n4 + c4];
#pragma unroll
        for (int u = 0; u < 4; ++u) add(v[u]);
    }
    for (; m < m_end; m += rows) add(z[(size_t)m * n4 + c4]);
    bn_block_reduce(acc, cg, rows, N, part);
}

// The two column sums of channel n = blockIdx.x * 16 + (thread & 15) over the slices: 16 interleaved partial sums per channel (slices g,
// g + 16, ..., each ascending, four slices in flight), then 0 + 1 + ... + 15 through LDS.  256 threads = 16 channels x 16 groups, grid
// N / 16; true in the threads of group 0, which hold the sums.  (One thread per channel walking up to 512 slices was 76 us a launch.)
__device__ inline bool bn_sum_slices(const double* __restrict__ part, int slices, int N, int* n_out, double* s_out, double* q_out) {
    __shared__ double rs[16][16], rq[16][16];
    const int tx = threadIdx.x & 15, g = threadIdx.x >> 4;
    const int n = blockIdx.x * 16 + tx;
    double s = 0.0, q = 0.0;
    int sl = g;
    for (; sl + 48 < slices; sl += 64) {
        double a[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            a[u] = part[(size_t)(sl + 16 * u) * 2 * N + n];
            b[u] = part[((size_t)(sl + 16 * u) * 2 + 1) * N + n];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) s += a[u], q += b[u];
    }
    for (; sl < slices; sl += 16) {
        s += part[(size_t)sl * 2 * N + n];
        q += part[((size_t)sl * 2 + 1) * N + n];
    }
    rs[g][tx] = s;
    rq[g][tx] = q;
    __syncthreads();
    if (g != 0) return false;
    for (int k = 1; k < 16; ++k) s += rs[k][tx], q += rq[k][tx];
    *n_out = n, *s_out = s, *q_out = q;
    return true;
}

// mu, var (biased) and r = 1 / sqrt(var + eps) of channel n from its two column sums over M rows
__device__ inline void bn_finish_channel(double s, double q, double M, float eps, int n, float* __restrict__ mu, float* __restrict__ var,
                                         float* __restrict__ r) {
#pragma clang fp contract(off)
    const double mean = s / M;
    double v = q / M - mean * mean;
    if (v < 0.0) v = 0.0;
    const float vf = (float)v;
    mu[n] = (float)mean;
    var[n] = vf;
    r[n] = (float)(1.0 / __dsqrt_rn((double)vf + (double)eps));
}

// mu, var (biased) and r = 1 / sqrt(var + eps) of every channel from the slices' partials (bn_sum_slices)
__global__ __launch_bounds__(256) void bn_stats_finish_kernel(const double* __restrict__ part, int slices, int M, int N, float eps, float* __restrict__ mu,
                                                              float* __restrict__ var, float* __restrict__ r) {
    int n;
    double s, q;
    if (!bn_sum_slices(part, slices, N, &n, &s, &q)) return;
    bn_finish_channel(s, q, (double)M, eps, n, mu, var, r);
}

// The same in two launches, for statistics over more rows than this device holds (data-parallel training): the slices' partials into
// sums [2][N] = (sum z | sum z^2) in the order of bn_sum_slices; the caller adds the other ranks' sums to them in place; then mu, var
// and r from the sums over all M rows, one thread per channel
__global__ __launch_bounds__(256) void bn_sums_kernel(const double* __restrict__ part, int slices, int N, double* __restrict__ sums) {
    int n;
    double s, q;
    if (!bn_sum_slices(part, slices, N, &n, &s, &q)) return;
    sums[n] = s;
    sums[N + n] = q;
}

__global__ __launch_bounds__(256) void bn_stats_from_sums_kernel(const double* __restrict__ sums, double M, int N, float eps, float* __restrict__ mu,
                                                                 float* __restrict__ var, float* __restrict__ r) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n < N) bn_finish_channel(sums[n], sums[N + n], M, eps, n, mu, var, r);
}

__device__ inline f32x4 relu4(f32x4 v) {
    v.x = v.x > 0.f ? v.x : 0.f;
    v.y = v.y > 0.f ? v.y : 0.f;
    v.z = v.z > 0.f ? v.z : 0.f;
    v.w = v.w > 0.f ? v.w : 0.f;
    return v;
}

__device__ inline f32x4 gate4(f32x4 v, f32x4 a) {
    v.x = a.x > 0.f ? v.x : 0.f;
    v.y = a.y > 0.f ? v.y : 0.f;
    v.z = a.z > 0.f ? v.z : 0.f;
    v.w = a.w > 0.f ? v.w : 0.f;
    return v;
}

// y = act(gamma * ((z - mu) * r) + beta (+ res)); n4 quads, N4 = N / 4
__global__ __launch_bounds__(256) void bn_apply_kernel(const f32x4* __restrict__ z, const f32x4* __restrict__ mu, const f32x4* __restrict__ r,
                                                       const f32x4* __restrict__ gamma, const f32x4* __restrict__ beta, const f32x4* __restrict__ res,
                                                       int relu, f32x4* __restrict__ y, long n4, int N4) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const int c = (int)(i % N4);
    f32x4 v = gamma[c] * ((z[i] - mu[c]) * r[c]) + beta[c];
    if (res) v += res[i];
    y[i] = relu ? relu4(v) : v;
}

// part[slice][0][n] = sum over the slice's rows of dz = dy * [y > 0] (y == nullptr: dz = dy), part[slice][1][n] = of dz * xhat
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const f32x4* __restrict__ dy, const f32x4* __restrict__ y, const f32x4* __restrict__ z,
                                                            const f32x4* __restrict__ mu, const f32x4* __restrict__ r, int M, int N, int cg, int rows, int P,
                                                            double* __restrict__ part) {
    const int col = threadIdx.x % cg, ry = threadIdx.x / cg;
    const int n4 = N / 4, c4 = blockIdx.x * cg + col;
    const int m_end = min(M, ((int)blockIdx.y + 1) * P);
    const f32x4 mu4 = mu[c4], r4 = r[c4];
    double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    auto add = [&](f32x4 d, const f32x4 a, const f32x4 zz) {
        if (y) d = gate4(d, a);
        const f32x4 xh = (zz - mu4) * r4;
        acc[0] += (double)d.x, acc[1] += (double)d.y, acc[2] += (double)d.z, acc[3] += (double)d.w;
        acc[4] += (double)d.x * (double)xh.x, acc[5] += (double)d.y * (double)xh.y, acc[6] += (double)d.z * (double)xh.z,
            acc[7] += (double)d.w * (double)xh.w;
    };
    int m = blockIdx.y * P + ry;
    for (; m + 3 * rows < m_end; m += 4 * rows) {  // four rows in flight, added in the order of the plain loop
        f32x4 d[4], a[4], zz[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const size_t i = (size_t)(m + u * rows) * n4 + c4;
            d[u] = dy[i];
            a[u] = y ? y[i] : d[u];
            zz[u] = z[i];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) add(d[u], a[u], zz[u]);
    }
    for (; m < m_end; m += rows) {
        const size_t i = (size_t)m * n4 + c4;
        add(dy[i], y ? y[i] : dy[i], z[i]);
    }
    bn_block_reduce(acc, cg, rows, N, part);
}

// dbeta, dgamma from the slices' partials (bn_sum_slices); db = 0 exactly (the bias cancels in z - mu)
__global__ __launch_bounds__(256) void bn_bwd_finish_kernel(const double* __restrict__ part, int slices, int N, float* __restrict__ db,
                                                            float* __restrict__ dgamma, float* __restrict__ dbeta) {
    int n;
    double s, q;
    if (!bn_sum_slices(part, slices, N, &n, &s, &q)) return;
    db[n] = 0.f;
    dbeta[n] = (float)s;
    dgamma[n] = (float)q;
}

// The same in two launches (bn_sums_kernel's split).  The local sums into sums [2][N] = (sum dz | sum dz * xhat) and, rounded, into the
// caller's gradient: dbeta and dgamma stay this rank's partial, which the all-reduce of the whole flat gradient completes ...
__global__ __launch_bounds__(256) void bn_bwd_sums_kernel(const double* __restrict__ part, int slices, int N, double* __restrict__ sums,
                                                          float* __restrict__ db, float* __restrict__ dgamma, float* __restrict__ dbeta) {
    int n;
    double s, q;
    if (!bn_sum_slices(part, slices, N, &n, &s, &q)) return;
    sums[n] = s;
    sums[N + n] = q;
    db[n] = 0.f;
    dbeta[n] = (float)s;
    dgamma[n] = (float)q;
}

// ... and the sums over all ranks, rounded as bn_bwd_finish_kernel rounds, into red [2][N] = (dbeta | dgamma): what bn_bwd_apply_kernel reads
__global__ __launch_bounds__(256) void bn_bwd_from_sums_kernel(const double* __restrict__ sums, int N, float* __restrict__ red) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    red[n] = (float)sums[n];
    red[N + n] = (float)sums[N + n];
}

// dz = dy * [y > 0] (y == nullptr: dz = dy) and dzraw = gamma * r * (dz - dbeta / M - xhat * dgamma / M).  dz may be nullptr and may alias dy
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const f32x4* dy, const f32x4* __restrict__ y, const f32x4* __restrict__ z,
                                                           const f32x4* __restrict__ mu, const f32x4* __restrict__ r, const f32x4* __restrict__ gamma,
                                                           const float* __restrict__ dgamma, const float* __restrict__ dbeta, float M, f32x4* dz,
                                                           f32x4* __restrict__ dzraw, long n4, int N4) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const int c = (int)(i % N4);
    f32x4 d = dy[i];
    if (y) d = gate4(d, y[i]);
    const f32x4 xh = (z[i] - mu[c]) * r[c];
    if (dz) dz[i] = d;
    // the caller's gradient buffer is only float-aligned
    const f32x4 dg = {dgamma[4 * c], dgamma[4 * c + 1], dgamma[4 * c + 2], dgamma[4 * c + 3]};
    const f32x4 dbt = {dbeta[4 * c], dbeta[4 * c + 1], dbeta[4 * c + 2], dbeta[4 * c + 3]};
    dzraw[i] = gamma[c] * r[c] * (d - dbt / M - xh * (dg / M));
}

// stats [mean of every channel | variance of every channel] <- momentum * stats + (1 - momentum) * batch, in double, one rounding;
// the batch variance times M / (M - 1) when unbiased, M = B * hw[channel]
__global__ __launch_bounds__(256) void bn_momentum_kernel(float* __restrict__ stats, const float* __restrict__ batch, const int* __restrict__ hw, int B,
                                                          int channels, double momentum, int unbiased) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * channels) return;
    double b = (double)batch[i];
    if (i >= channels && unbiased) {
        const double M = (double)B * (double)hw[i - channels];
        b = b * (M / (M - 1.0));
    }
    stats[i] = (float)(momentum * (double)stats[i] + (1.0 - momentum) * b);
}

// the installed statistics and what the frozen path folds from them: mean, sd = sqrt((double)var + (double)eps) (correctly rounded: the
// host packers take std::sqrt of the same sum) and istd = (float)(1 / sd)
__global__ __launch_bounds__(256) void bn_install_kernel(const float* __restrict__ stats, int channels, float eps, float* __restrict__ keep,
                                                         float* __restrict__ mean, float* __restrict__ istd, double* __restrict__ sd) {
#pragma clang fp contract(off)
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= channels) return;
    const float m = stats[c], v = stats[channels + c];
    keep[c] = m;
    keep[channels + c] = v;
    mean[c] = m;
    const double s = __dsqrt_rn((double)v + (double)eps);
    sd[c] = s;
    istd[c] = (float)(1.0 / s);
}

const f32x4* q4(const float* p) { return reinterpret_cast<const f32x4*>(p); }
f32x4* q4(float* p) { return reinterpret_cast<f32x4*>(p); }

constexpr int VEC = 4;  // channels a thread
bool bad_shape(long M, int N) { return bn_bad_shape(M, N, VEC); }

// the first launch of each reduction; *slices: how many partials the finish adds
hipError_t launch_stats(const float* z, int M, int N, double* part, int* slices, hipStream_t st) {
    if (bad_shape(M, N)) return hipErrorInvalidValue;
    const BnGeom g = bn_geom(M, N, VEC);
    hipLaunchKernelGGL(bn_stats_kernel, dim3(g.gx, g.slices), dim3(256), 0, st, q4(z), M, N, g.cg, g.rows, g.P, part);
    *slices = g.slices;
    return hipGetLastError();
}

hipError_t launch_bwd_reduce(const float* dy, const float* y, const float* z, const float* mu, const float* r, int M, int N, double* part, int* slices,
                             hipStream_t st) {
    if (bad_shape(M, N)) return hipErrorInvalidValue;
    const BnGeom g = bn_geom(M, N, VEC);
    hipLaunchKernelGGL(bn_bwd_reduce_kernel, dim3(g.gx, g.slices), dim3(256), 0, st, q4(dy), q4(y), q4(z), q4(mu), q4(r), M, N, g.cg, g.rows, g.P, part);
    *slices = g.slices;
    return hipGetLastError();
}

}  // namespace

// vec channels a thread: N is whole workgroups of channel groups (N / vec at most 64, or a multiple of 64), which every ResNet-50 layer has
bool bn_bad_shape(long M, int N, int vec) {
    return M < 1 || M > 0x7fffffffL / 2 || N < 64 || N > 2048 || (N <= 64 * vec ? N % 64 != 0 : N % (64 * vec) != 0);
}

BnGeom bn_geom(int M, int N, int vec) {
    BnGeom g{};
    const int nv = N / vec;
    g.cg = std::min(nv, 64);
    g.rows = 256 / g.cg;
    g.gx = nv / g.cg;
    // at least eight rows per thread, about 2048 workgroups at most, and a partial buffer of BN_PART_COLS columns
    int sl = std::max(1, (M + g.rows * 8 - 1) / (g.rows * 8));
    sl = std::min(sl, std::max(1, 2048 / g.gx));
    sl = std::min(sl, std::min(BN_MAX_SLICES, BN_PART_COLS / N));
    g.P = (M + sl - 1) / sl;
    g.slices = (M + g.P - 1) / g.P;
    return g;
}

int bn_slices(int M, int N) { return bad_shape(M, N) ? -1 : bn_geom(M, N, VEC).slices; }

// the second launch of each reduction: from the slices' partials part[slice][2][N], whichever kernel wrote them (encoder_bn_bf16.hip too)
hipError_t bn_finish_stats(const double* part, int slices, int M, int N, float eps, float* mu, float* var, float* r, hipStream_t st) {
    hipLaunchKernelGGL(bn_stats_finish_kernel, dim3(N / 16), dim3(256), 0, st, part, slices, M, N, eps, mu, var, r);
    return hipGetLastError();
}

hipError_t bn_finish_sums(const double* part, int slices, int N, double* sums, hipStream_t st) {
    hipLaunchKernelGGL(bn_sums_kernel, dim3(N / 16), dim3(256), 0, st, part, slices, N, sums);
    return hipGetLastError();
}

hipError_t bn_finish_bwd(const double* part, int slices, int N, float* db, float* dgamma, float* dbeta, hipStream_t st) {
    hipLaunchKernelGGL(bn_bwd_finish_kernel, dim3(N / 16), dim3(256), 0, st, part, slices, N, db, dgamma, dbeta);
    return hipGetLastError();
}

hipError_t bn_finish_bwd_sums(const double* part, int slices, int N, double* sums, float* db, float* dgamma, float* dbeta, hipStream_t st) {
    hipLaunchKernelGGL(bn_bwd_sums_kernel, dim3(N / 16), dim3(256), 0, st, part, slices, N, sums, db, dgamma, dbeta);
    return hipGetLastError();
}

hipError_t bn_launch_stats(const float* z, int M, int N, float eps, double* part, float* mu, float* var, float* r, hipStream_t st) {
    int slices;
    hipError_t e = launch_stats(z, M, N, part, &slices, st);
    return e != hipSuccess ? e : bn_finish_stats(part, slices, M, N, eps, mu, var, r, st);
}

hipError_t bn_launch_stats_sums(const float* z, int M, int N, double* part, double* sums, hipStream_t st) {
    int slices;
    hipError_t e = launch_stats(z, M, N, part, &slices, st);
    return e != hipSuccess ? e : bn_finish_sums(part, slices, N, sums, st);
}

hipError_t bn_launch_stats_from_sums(const double* sums, double M, int N, float eps, float* mu, float* var, float* r, hipStream_t st) {
    if (bad_shape(1, N) || !(M >= 1.0)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bn_stats_from_sums_kernel, grid1(N), dim3(256), 0, st, sums, M, N, eps, mu, var, r);
    return hipGetLastError();
}

hipError_t bn_launch_apply(const float* z, const float* mu, const float* r, const float* gamma, const float* beta, const float* res, int relu, float* y,
                           int M, int N, hipStream_t st) {
    if (bad_shape(M, N)) return hipErrorInvalidValue;
    const long n4 = (long)M * (N / 4);
    hipLaunchKernelGGL(bn_apply_kernel, grid1(n4), dim3(256), 0, st, q4(z), q4(mu), q4(r), q4(gamma), q4(beta), q4(res), relu, q4(y), n4, N / 4);
    return hipGetLastError();
}

hipError_t bn_launch_bwd_reduce(const float* dy, const float* y, const float* z, const float* mu, const float* r, int M, int N, double* part, float* db,
                                float* dgamma, float* dbeta, hipStream_t st) {
    int slices;
    hipError_t e = launch_bwd_reduce(dy, y, z, mu, r, M, N, part, &slices, st);
    return e != hipSuccess ? e : bn_finish_bwd(part, slices, N, db, dgamma, dbeta, st);
}

hipError_t bn_launch_bwd_sums(const float* dy, const float* y, const float* z, const float* mu, const float* r, int M, int N, double* part, double* sums,
                              float* db, float* dgamma, float* dbeta, hipStream_t st) {
    int slices;
    hipError_t e = launch_bwd_reduce(dy, y, z, mu, r, M, N, part, &slices, st);
    return e != hipSuccess ? e : bn_finish_bwd_sums(part, slices, N, sums, db, dgamma, dbeta, st);
}

hipError_t bn_launch_bwd_from_sums(const double* sums, int N, float* red, hipStream_t st) {
    if (bad_shape(1, N)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bn_bwd_from_sums_kernel, grid1(N), dim3(256), 0, st, sums, N, red);
    return hipGetLastError();
}

hipError_t bn_launch_bwd_apply(const float* dy, const float* y, const float* z, const float* mu, const float* r, const float* gamma, const float* dgamma,
                               const float* dbeta, int M, int N, float* dz, float* dzraw, hipStream_t st, double M_all) {
    if (bad_shape(M, N)) return hipErrorInvalidValue;
    const long n4 = (long)M * (N / 4);
    hipLaunchKernelGGL(bn_bwd_apply_kernel, grid1(n4), dim3(256), 0, st, q4(dy), q4(y), q4(z), q4(mu), q4(r), q4(gamma), dgamma, dbeta,
                       M_all > 0.0 ? (float)M_all : (float)M, q4(dz), q4(dzraw), n4, N / 4);
    return hipGetLastError();
}

hipError_t bn_launch_momentum(float* stats, const float* batch, const int* hw, int B, int channels, double momentum, int unbiased, hipStream_t st) {
    hipLaunchKernelGGL(bn_momentum_kernel, grid1(2 * (long)channels), dim3(256), 0, st, stats, batch, hw, B, channels, momentum, unbiased);
    return hipGetLastError();
}

hipError_t bn_launch_install(const float* stats, int channels, float eps, float* keep, float* mean, float* istd, double* sd, hipStream_t st) {
    hipLaunchKernelGGL(bn_install_kernel, grid1(channels), dim3(256), 0, st, stats, channels, eps, keep, mean, istd, sd);
    return hipGetLastError();
}
