// regressor_train.hip -- training the RegressionNetwork (src/models.py:60-74) through the iterative-error-feedback loop of the generator
// update (src/trainer.py:389-401, 481-482): the forward with dropout at the last stage, the gradient of sum_i <grad_thetas[i], theta_i>
// with respect to the three Dense layers and mean theta, the gradient to the features, and the flat <-> live parameter copies.
//
//   x_i = [f | theta_{i-1}]      a1 = drop1_i * relu(x_i W1 + b1)      a2 = drop2_i * relu(a1 W2 + b2)      theta_i = theta_{i-1} + a2 W3 + b3
//
// Data gradients (dz . W^T) are the forward's dense GEMM (run_dense: the 64 x 64 implicit-GEMM kernel, dense_gemv at <= 4 rows): its
// Wt[n][k] operand is then the Keras [in][out] matrix itself (RegTrainWork in hpe_ctx.h).  The ReLU / dropout gate is ONE small
// elementwise launch per layer (reg_gate_kernel), not an epilogue variant: the GEMM kernels and every launch of the inference path stay
// as they are.  The gate of layer 1 also keeps the running sum of dz1 over the stages (the feature block of W1 is hoisted out of the
// loop in both directions) and forms the residual operand g_i + grad_thetas[i - 1] of the theta GEMM.
//
// Weight gradients are ONE launch of reg_wg_gemm_kernel, C[in][out] = sum_r X[r][in] D[r][out] with the stages stacked along r
// (stage-then-row order).  v_mfma_f32_32x32x2_f32 wants A[row][k] and B[k][col] with lanes along row / col; for a fixed r both X[r][.] and
// D[r][.] are contiguous, so every lane reads its operand straight from global memory in one coalesced dword load per k -- no LDS, no
// transposed copy.  One workgroup of four waves per 64 x 64 tile, each wave a 32 x 32 block, the whole K per tile: no split-K, no atomics,
// no fix-up.  Segments of the one grid: dW1f (K = B with the summed dz1: the 2048-wide feature rows are read once, not once per stage;
// 512 tiles), dW1theta (32), dW2 (256), dW3 (32), and one last workgroup for d mean (the column sums of the cotangent reaching the tiled
// mean).  The waves of a segment's first tile row also sum D's columns: the bias gradient.  Rows past K are never read (masked to 0).
//
// Summation order is fixed everywhere (per tile ascending r; bias: even and odd rows ascending, then even + odd; stages added in
// descending order): the same inputs give the same bits.
#include <hip/hip_runtime.h>

#include "hpe_ctx.h"

namespace {

constexpr int F = HPE_FEATURE_DIM, H = 1024, T = HPE_THETA_DIM, LD = THETA_LD;
constexpr int IN1 = F + T;
// the flat layout: dense_0/kernel [2133][1024], dense_0/bias, dense_1/kernel, dense_1/bias, dense_2/kernel [1024][85], dense_2/bias, mean theta
constexpr int OFF_W1 = 0, OFF_B1 = OFF_W1 + IN1 * H, OFF_W2 = OFF_B1 + H, OFF_B2 = OFF_W2 + H * H, OFF_W3 = OFF_B2 + H, OFF_B3 = OFF_W3 + H * T,
              OFF_MEAN = OFF_B3 + T, PARAM_FLOATS = OFF_MEAN + T;
static_assert(PARAM_FLOATS == 3322026, "flat layout of the regressor");

struct RegW {  // every live buffer of the regressor
    float *w1f, *w1t, *w2, *w3, *b1, *b2, *b3, *mean, *w1k, *w2k, *w3k;
};

// src [K][1024] (flat) -> its packed transposes: rows k < k_split to dst_a[n][k] (pitch ld_a), the rest to dst_b[n][k - k_split] (pitch
// ld_b), and the Keras-major copy.  32 x 32 tiles through LDS: both sides coalesced.  block (32, 8)
__global__ __launch_bounds__(256) void reg_set_transpose_kernel(const float* __restrict__ src, int K, float* __restrict__ copy,
                                                                float* __restrict__ dst_a, int ld_a, int k_split, float* __restrict__ dst_b,
                                                                int ld_b) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int k0 = blockIdx.y * 32, n0 = blockIdx.x * 32;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int k = k0 + ty + 8 * j;
        float v = 0.f;
        if (k < K) {
            v = src[(size_t)k * H + n0 + tx];
            copy[(size_t)k * H + n0 + tx] = v;
        }
        tile[ty + 8 * j][tx] = v;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int n = n0 + ty + 8 * j, k = k0 + tx;
        if (k >= K) continue;
        const float v = tile[tx][ty + 8 * j];
        if (k < k_split)
            dst_a[(size_t)n * ld_a + k] = v;
        else
            dst_b[(size_t)n * ld_b + (k - k_split)] = v;
    }
}

// everything but the two big kernels: biases, dense_2 (85 columns: packed [85][1024] and Keras-major with pitch THETA_LD) and mean theta.
// GET reads everything, the two big kernels included, from the Keras-major copies.
template <bool SET>
__global__ __launch_bounds__(256) void reg_params_kernel(RegW w, float* __restrict__ flat, int p0) {
    const int p = p0 + blockIdx.x * 256 + threadIdx.x;
    if (p >= PARAM_FLOATS) return;
    if (p < OFF_B1) {
        if (!SET) flat[p] = w.w1k[p];
    } else if (p < OFF_W2) {
        if (SET) w.b1[p - OFF_B1] = flat[p];
        else flat[p] = w.b1[p - OFF_B1];
    } else if (p < OFF_B2) {
        if (!SET) flat[p] = w.w2k[p - OFF_W2];
    } else if (p < OFF_W3) {
        if (SET) w.b2[p - OFF_B2] = flat[p];
        else flat[p] = w.b2[p - OFF_B2];
    } else if (p < OFF_B3) {
        const int q = p - OFF_W3, k = q / T, n = q - k * T;
        if (SET) {
            const float v = flat[p];
            w.w3k[k * LD + n] = v;
            w.w3[(size_t)n * H + k] = v;
        } else {
            flat[p] = w.w3k[k * LD + n];
        }
    } else if (p < OFF_MEAN) {
        if (SET) w.b3[p - OFF_B3] = flat[p];
        else flat[p] = w.b3[p - OFF_B3];
    } else {
        if (SET) w.mean[p - OFF_MEAN] = flat[p];
        else flat[p] = w.mean[p - OFF_MEAN];
    }
}

// a *= m  (dropout multipliers on the hidden activations of the last stage)
__global__ __launch_bounds__(256) void reg_scale_kernel(float* __restrict__ a, const float* __restrict__ m, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) a[i] *= m[i];
}

// g [S + 1][B][LD]: index 0 zeros, index s + 1 the external cotangent of stage s (ext [S][B][85] or nullptr = zero), padding zero
__global__ __launch_bounds__(256) void reg_cotangent_kernel(const float* __restrict__ ext, float* __restrict__ g, int S, int B) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= (S + 1) * B * LD) return;
    const int row = i / LD, k = i - row * LD;
    g[i] = (ext && row >= B && k < T) ? ext[(size_t)(row - B) * T + k] : 0.f;
}

// dz = da * drop * [a > 0] (TensorFlow's ReLU gradient: zero at z = 0; drop == nullptr: ones).  Layer 1 only: sum (running sum of dz over
// the stages; first: start it) and r = g_hi + g_lo over nr floats (the cotangent reaching theta_i plus the external one of theta_{i-1})
__global__ __launch_bounds__(256) void reg_gate_kernel(const float* __restrict__ da, const float* __restrict__ a, const float* __restrict__ drop,
                                                       float* __restrict__ dz, float* __restrict__ sum, int first, int n,
                                                       const float* __restrict__ g_hi, const float* __restrict__ g_lo, float* __restrict__ r,
                                                       int nr) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        const float v = a[i] > 0.f ? da[i] * (drop ? drop[i] : 1.f) : 0.f;
        dz[i] = v;
        if (sum) sum[i] = first ? v : sum[i] + v;
    }
    if (r && i < nr) r[i] = g_hi[i] + g_lo[i];
}

struct WgSeg {
    const float* x;  // [K][ldx], IN columns used
    const float* d;  // [K][ldd], OUT columns used
    float* c;        // [IN][OUT]
    float* bias;     // [OUT] column sums of d, or nullptr
    int ldx, ldd, IN, OUT, K, tile0, n_ot;
};
constexpr int WG_SEGS = 4;
struct WgArgs {
    WgSeg seg[WG_SEGS];
    const float* g0;  // [B][LD] cotangent reaching the tiled mean
    float* dmean;     // [85]
    int B, n_tiles;
};

__global__ __launch_bounds__(256) void reg_wg_gemm_kernel(WgArgs a) {
    const int t = threadIdx.x, bid = blockIdx.x;
    if (bid == a.n_tiles) {  // d mean: two interleaved row sets per column, each in ascending order, then set 0 + set 1
        __shared__ float part[2][LD];
        if (t < 2 * LD) {
            const int grp = t / LD, col = t - grp * LD;
            float s = 0.f;
            for (int b = grp; b < a.B; b += 2) s += a.g0[(size_t)b * LD + col];
            part[grp][col] = s;
        }
        __syncthreads();
        if (t < T) a.dmean[t] = part[0][t] + part[1][t];
        return;
    }
    WgSeg g = a.seg[0];  // workgroup-uniform selects (a run-time index into the argument struct would go through scratch)
#pragma unroll
    for (int s = 1; s < WG_SEGS; ++s)
        if (bid >= a.seg[s].tile0) g = a.seg[s];
    const int ti = bid - g.tile0;
    const int in0 = (ti / g.n_ot) * 64, out0 = (ti % g.n_ot) * 64;
    const int lane = t & 63, wave = t >> 6, wm = wave >> 1, wn = wave & 1, hi = lane >> 5;
    const int col_a = in0 + wm * 32 + (lane & 31), col_b = out0 + wn * 32 + (lane & 31);
    const bool a_ok = col_a < g.IN, b_ok = col_b < g.OUT;
    // lane l feeds A[row = l & 31][k = l >> 5] and B[k = l >> 5][col = l & 31]: row r + hi of x and of d
    const float* xp = g.x + (size_t)hi * g.ldx + (a_ok ? col_a : 0);
    const float* dp = g.d + (size_t)hi * g.ldd + (b_ok ? col_b : 0);
    const bool own_bias = g.bias != nullptr && in0 == 0 && wm == 0;
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    float bs = 0.f;
    int r = 0;
    for (; r + 16 <= g.K; r += 16) {  // 8 k-steps of 2 rows, all 16 loads issued before the first MFMA
        float av[8], bv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            av[u] = a_ok ? xp[(size_t)(r + 2 * u) * g.ldx] : 0.f;
            bv[u] = b_ok ? dp[(size_t)(r + 2 * u) * g.ldd] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bv[u], acc, 0, 0, 0);
            bs += bv[u];
        }
    }
    for (; r < g.K; r += 2) {  // the k-tail: a row at or past K is not read
        const bool ok = r + hi < g.K;
        const float av = (ok && a_ok) ? xp[(size_t)r * g.ldx] : 0.f;
        const float bv = (ok && b_ok) ? dp[(size_t)r * g.ldd] : 0.f;
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
        bs += bv;
    }
    // accumulator element e of lane l: row (e & 3) + 8 (e >> 2) + 4 (l >> 5), column l & 31
    if (b_ok) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int row = in0 + wm * 32 + (e & 3) + 8 * (e >> 2) + 4 * hi;
            if (row < g.IN) g.c[(size_t)row * g.OUT + col_b] = acc[e];
        }
    }
    if (own_bias) {  // wave-uniform
        const float other = __shfl_xor(bs, 32, 64);
        if (hi == 0 && b_ok) g.bias[col_b] = bs + other;
    }
}

RegW live(hpe_ctx* c) { return RegW{c->w1f, c->w1t, c->w2, c->w3, c->b1, c->b2, c->b3, c->mean_dev, c->rt.w1k, c->rt.w2k, c->rt.w3k}; }

hipError_t dense(hpe_ctx* c, const float* x, int lda, int M, int K, const float* w, int w_rows, int N, const float* shift, const float* res,
                 int ldres, int relu, float* y, int ldy, hipStream_t st) {
    return run_dense(c, x, lda, M, K, w, w_rows, N, c->ones, shift, res, ldres, relu, y, ldy, st, c->rt.partial, c->rt.partial_floats);
}

}  // namespace

int regressor_param_offset(int idx, bool bias) {
    const int w[5] = {OFF_W1, OFF_W2, OFF_W3, OFF_MEAN, PARAM_FLOATS}, b[3] = {OFF_B1, OFF_B2, OFF_B3};
    return bias ? b[idx] : w[idx];
}

// the IEF loop exactly as tail_impl / regress_impl launch it, with every stage's rows kept: rt.th[s + 1] = theta_s, rt.a1[s], rt.a2[s]
hipError_t regressor_train_forward(hpe_ctx* c, const float* features, int B, const float* drop, hipStream_t st) {
    RegTrainWork& w = c->rt;
    const int S = c->cfg.num_stage;
    const size_t nh = (size_t)B * H, nt = (size_t)B * LD;
    HIPE(dense(c, features, F, B, F, c->w1f, 1024, 1024, c->zeros, nullptr, 0, 0, w.p1, 1024, st));
    HIPE(hpe_launch_tile_theta(c->mean_dev, w.th, B, LD, st));
    for (int s = 0; s < S; ++s) {
        const float* prev = w.th + s * nt;
        float *a1 = w.a1 + s * nh, *a2 = w.a2 + s * nh;
        const bool dr = drop && s == S - 1;
        HIPE(dense(c, prev, LD, B, LD, c->w1t, 1024, 1024, c->b1, w.p1, 1024, 1, a1, 1024, st));
        if (dr) hipLaunchKernelGGL(reg_scale_kernel, grid1((long)nh), dim3(256), 0, st, a1, drop, (int)nh);
        HIPE(dense(c, a1, 1024, B, 1024, c->w2, 1024, 1024, c->b2, nullptr, 0, 1, a2, 1024, st));
        if (dr) hipLaunchKernelGGL(reg_scale_kernel, grid1((long)nh), dim3(256), 0, st, a2, drop + nh, (int)nh);
        HIPE(dense(c, a2, 1024, B, 1024, c->w3, 128, T, c->b3, prev, LD, 0, w.th + (s + 1) * nt, LD, st));
    }
    return hipGetLastError();
}

hipError_t regressor_train_backward(hpe_ctx* c, const float* features, int B, const float* drop, const float* grad_thetas, float* grad_flat,
                                    float* grad_features, hipStream_t st) {
    RegTrainWork& w = c->rt;
    const int S = c->cfg.num_stage;
    const size_t nh = (size_t)B * H, nt = (size_t)B * LD;
    HIPE(regressor_train_forward(c, features, B, drop, st));
    hipLaunchKernelGGL(reg_cotangent_kernel, grid1((long)(S + 1) * nt), dim3(256), 0, st, grad_thetas, w.g, S, B);
    for (int i = S - 1; i >= 0; --i) {
        const float* gi = w.g + (i + 1) * nt;  // the total cotangent of theta_i = dz3_i
        float* glo = w.g + i * nt;             // before the theta GEMM: the external cotangent of theta_{i-1} (zeros for i == 0)
        const bool dr = drop && i == S - 1;
        HIPE(dense(c, gi, LD, B, LD, w.w3k, 1024, 1024, w.zeros, nullptr, 0, 0, w.da, 1024, st));
        hipLaunchKernelGGL(reg_gate_kernel, grid1((long)nh), dim3(256), 0, st, w.da, w.a2 + i * nh, dr ? drop + nh : nullptr, w.dz2 + i * nh,
                           (float*)nullptr, 0, (int)nh, (const float*)nullptr, (const float*)nullptr, (float*)nullptr, 0);
        HIPE(dense(c, w.dz2 + i * nh, 1024, B, 1024, w.w2k, 1024, 1024, w.zeros, nullptr, 0, 0, w.da, 1024, st));
        hipLaunchKernelGGL(reg_gate_kernel, grid1((long)nh), dim3(256), 0, st, w.da, w.a1 + i * nh, dr ? drop : nullptr, w.dz1 + i * nh, w.sum1,
                           i == S - 1 ? 1 : 0, (int)nh, gi, (const float*)glo, w.r, (int)nt);
        // g_{i-1} = g_i + ext_{i-1} + dz1_i . W1theta^T  (W1theta = rows 2048.. of the Keras matrix, zero padded to 128 rows)
        HIPE(dense(c, w.dz1 + i * nh, 1024, B, 1024, w.w1k + (size_t)F * H, 128, T, w.zeros, w.r, LD, 0, glo, LD, st));
    }
    if (grad_features) HIPE(dense(c, w.sum1, 1024, B, 1024, w.w1k, F, F, w.zeros, nullptr, 0, 0, grad_features, F, st));
    WgArgs a{};
    const int K = S * B;
    a.seg[0] = WgSeg{features, w.sum1, grad_flat + OFF_W1, nullptr, F, H, F, H, B, 0, H / 64};
    a.seg[1] = WgSeg{w.th, w.dz1, grad_flat + OFF_W1 + (size_t)F * H, grad_flat + OFF_B1, LD, H, T, H, K, 0, H / 64};
    a.seg[2] = WgSeg{w.a1, w.dz2, grad_flat + OFF_W2, grad_flat + OFF_B2, H, H, H, H, K, 0, H / 64};
    a.seg[3] = WgSeg{w.a2, w.g + nt, grad_flat + OFF_W3, grad_flat + OFF_B3, H, LD, H, T, K, 0, (T + 63) / 64};
    int tiles = 0;
    for (int s = 0; s < WG_SEGS; ++s) {
        a.seg[s].tile0 = tiles;
        tiles += ((a.seg[s].IN + 63) / 64) * a.seg[s].n_ot;
    }
    a.g0 = w.g;
    a.dmean = grad_flat + OFF_MEAN;
    a.B = B;
    a.n_tiles = tiles;
    hipLaunchKernelGGL(reg_wg_gemm_kernel, dim3(tiles + 1), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t regressor_params_copy(hpe_ctx* c, float* flat, bool set, hipStream_t st) {
    const RegW w = live(c);
    if (set) {
        hipLaunchKernelGGL(reg_set_transpose_kernel, dim3(H / 32, (IN1 + 31) / 32), dim3(32, 8), 0, st, flat + OFF_W1, IN1, w.w1k, w.w1f, F, F,
                           w.w1t, LD);
        hipLaunchKernelGGL(reg_set_transpose_kernel, dim3(H / 32, H / 32), dim3(32, 8), 0, st, flat + OFF_W2, H, w.w2k, w.w2, H, H, (float*)nullptr,
                           0);
        // b1 and b2 lie before SMALL0: two short launches of the same kernel cover them
        hipLaunchKernelGGL(reg_params_kernel<true>, grid1(H), dim3(256), 0, st, w, flat, OFF_B1);
        hipLaunchKernelGGL(reg_params_kernel<true>, grid1(PARAM_FLOATS - OFF_B2), dim3(256), 0, st, w, flat, OFF_B2);
    } else {
        hipLaunchKernelGGL(reg_params_kernel<false>, grid1(PARAM_FLOATS), dim3(256), 0, st, w, flat, 0);
    }
    return hipGetLastError();
}
