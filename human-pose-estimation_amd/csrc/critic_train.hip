// critic_train.hip -- the gradient of the critic's scores, and of their input gradient, with respect to the critic's WEIGHTS: what the
// WGAN critic update (src/trainer.py:511-583) and its gradient penalty (src/ops.py:153-172) differentiate.  Also the flat parameter
// layout (kernel 0 [in][out], bias 0, kernel 1, ...) and the device-side get / set of the live weights.
//
//   F = sum_n [ sum_c gs[n,c] * scores[n,c] + < t_n , d(sum_c scores[n,c]) / dx_n > ]
//
// The critic is piecewise linear in each input and KCS is free of weights, so with b_l the backward signal of layer l for a cotangent of 1,
// delta_l = gs[n, c(l)] * b_l (every layer of a branch feeds one score column c(l)), and u_l = D_l W_l^T u_{l-1} the tangent pass from u_0 = t,
//
//   dF/dW_l = sum_n ( gs[n,c(l)] * a_{l-1,n} + u_{l-1,n} ) (x) b_{l,n}          dF/db_l = sum_n gs[n,c(l)] * b_{l,n}
//
// Three launches.  (1) critic_wg_rows_kernel: one workgroup per CRITIC_ROWS rows recomputes the forward with critic.hip's loops, runs the
// tangent pass beside it (one weight read feeds both) and writes, per row, the left operands x = gs * a + u of all nine layers (1043
// floats), the signals b (618) and gs (3) into the workspace.  (2) critic_wg_gemm_kernel: per layer X^T . B over the rows as 64 x 64 output
// tiles, rows cut into chunks of WG_CHUNK; fp32 FMA out of LDS (the fp32 matrix instruction has the vector rate on gfx950, and at these
// sizes launch count and latency decide).  (3) critic_wg_finish_kernel adds the chunks' partials in chunk order (skipped for one chunk).
//
// Summation order: inside a chunk one thread owns one weight and adds its rows in ascending order with fmaf; chunks are added in
// ascending order by one thread per weight.  No atomics, nothing reduced across threads: the same inputs give the same bits.  The result
// is a sum over rows, so it depends on N and on the order of the rows.
//
// The layer table, the layouts derived from it and the dense loops are critic_common.h's.  Still repeated: the prologue of
// critic_wg_rows_kernel restates critic.hip's load_tile (three staging loops, KCS = B^T B) with a tangent read beside every input and the
// tangent products inside the KCS sum.  One loader with a functor for those six points was tried: the compiler then schedules the prologue
// of all three kernels differently, and their device code is pinned to what it was.
#include <hip/hip_runtime.h>

#include "critic_common.h"

namespace {

constexpr int ROW_THREADS = 512, GEMM_THREADS = 256;
constexpr int TILE = WG_TILE, KB = 16;  // output tile of the row-reduction GEMM; rows staged in LDS per step

// the tables the gemm and params kernels index at run time (aligned as the plain int arrays they were: the object code is unchanged)
__constant__ __align__(16) Table<NL> L_IN = LAYOUT.in, L_OUT = LAYOUT.out, L_X = LAYOUT.x, L_S = LAYOUT.s, L_COL = LAYOUT.col;
__constant__ __align__(16) Table<NL + 1> L_TILE0 = LAYOUT.tile0, L_W = LAYOUT.w;

// the same, and beside it the tangent tan[r] = sum over k of W[k * ld + o] * us[k][r]: one weight read serves both
__device__ __forceinline__ void dense_col2(const float* __restrict__ W, int ld, int K, int o, float init, const float* xs, const float* us,
                                           float acc[R], float tan[R]) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
        acc[r] = init;
        tan[r] = 0.f;
    }
    const float* w = W + o;
#pragma unroll 4
    for (int k = 0; k < K; ++k) {
        const float wk = w[(size_t)k * ld];
        const float4 x = *reinterpret_cast<const float4*>(xs + k * R);
        const float4 u = *reinterpret_cast<const float4*>(us + k * R);
        acc[0] = fmaf(wk, x.x, acc[0]);
        acc[1] = fmaf(wk, x.y, acc[1]);
        acc[2] = fmaf(wk, x.z, acc[2]);
        acc[3] = fmaf(wk, x.w, acc[3]);
        tan[0] = fmaf(wk, u.x, tan[0]);
        tan[1] = fmaf(wk, u.y, tan[1]);
        tan[2] = fmaf(wk, u.z, tan[2]);
        tan[3] = fmaf(wk, u.w, tan[3]);
    }
}

struct Tangents {
    const float* kcs;     // [., 169]
    const float* joints;  // [., 42]
    const float* betas;   // [., 10]
    const float* Rs;      // [., 207]
    int per_row;          // 0: one vector shared by all rows
};

struct RowTile {  // LDS image of one tile; every [k][R] array is read as float4 per k
    float J[NJF * R], tJ[NJF * R];
    float kcs[NKCS * R], tk[NKCS * R];  // tk: the effective KCS tangent t_kcs + B_t^T B + B^T B_t
    float rot[NROT * R], trot[NROT * R];
    float r1[300 * R], u1[300 * R];  // rotation_dense_1: activations and tangents
    float s2[100 * R];               // rotation_dense_2: signals
    float beta[R][NBETA], tbeta[R][NBETA];
    float g[R][4];  // grad_scores of the tile's rows (zeros without a first-order term)
};

__global__ __launch_bounds__(ROW_THREADS) void critic_wg_rows_kernel(CriticW w, const float* __restrict__ joints, int K,
                                                                     const float* __restrict__ betas, int betas_stride,
                                                                     const float* __restrict__ Rs, long N, const float* __restrict__ gscores,
                                                                     Tangents tg, float* __restrict__ ws) {
    __shared__ __align__(16) RowTile s;
    const int t = threadIdx.x;
    const long row0 = (long)blockIdx.x * R;
    // ---- inputs, tangents and grad_scores of the tile's rows -> LDS (rows past N read as zeros)
    if (t < R * 3) {
        const int r = t / 3, k = t - r * 3;
        s.g[r][k] = (gscores && row0 + r < N) ? gscores[(size_t)(row0 + r) * 3 + k] : 0.f;
    }
    for (int i = t; i < NJF * R; i += ROW_THREADS) {
        const int r = i / NJF, k = i - r * NJF;
        const long row = row0 + r;
        s.J[k * R + r] = row < N ? joints[(size_t)row * K * 3 + k] : 0.f;
        s.tJ[k * R + r] = (tg.joints && row < N) ? tg.joints[(size_t)(tg.per_row ? row : 0) * NJF + k] : 0.f;
    }
    for (int i = t; i < NROT * R; i += ROW_THREADS) {
        const int r = i / NROT, k = i - r * NROT;
        const long row = row0 + r;
        s.rot[k * R + r] = row < N ? Rs[(size_t)row * 216 + 9 + k] : 0.f;
        s.trot[k * R + r] = (tg.Rs && row < N) ? tg.Rs[(size_t)(tg.per_row ? row : 0) * NROT + k] : 0.f;
    }
    for (int i = t; i < NBETA * R; i += ROW_THREADS) {
        const int r = i / NBETA, k = i - r * NBETA;
        const long row = row0 + r;
        s.beta[r][k] = row < N ? betas[(size_t)row * betas_stride + k] : 0.f;
        s.tbeta[r][k] = (tg.betas && row < N) ? tg.betas[(size_t)(tg.per_row ? row : 0) * NBETA + k] : 0.f;
    }
    __syncthreads();
    // ---- KCS = B^T B and its tangent; the left operands of the three first layers that read an input
    for (int i = t; i < NKCS * R; i += ROW_THREADS) {
        const int r = i / NKCS, m = i - r * NKCS;
        const int a = m / NB, b = m - a * NB;
        const int am = BONE_MINUS[a], bm = BONE_MINUS[b];
        const long row = row0 + r;
        float v = 0.f, tv = (tg.kcs && row < N) ? tg.kcs[(size_t)(tg.per_row ? row : 0) * NKCS + m] : 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float Ba = s.J[(a * 3 + c) * R + r] - s.J[(am * 3 + c) * R + r];
            const float Bb = s.J[(b * 3 + c) * R + r] - s.J[(bm * 3 + c) * R + r];
            const float Ta = s.tJ[(a * 3 + c) * R + r] - s.tJ[(am * 3 + c) * R + r];
            const float Tb = s.tJ[(b * 3 + c) * R + r] - s.tJ[(bm * 3 + c) * R + r];
            v = fmaf(Ba, Bb, v);
            tv = fmaf(Ta, Bb, tv);
            tv = fmaf(Ba, Tb, tv);
        }
        s.kcs[m * R + r] = v;
        s.tk[m * R + r] = tv;
        if (row < N) ws[(size_t)row * ROW_LD + X_OF<L_KCS> + m] = fmaf(s.g[r][0], v, tv);
    }
    for (int i = t; i < NJF * R; i += ROW_THREADS) {
        const int r = i / NJF, k = i - r * NJF;
        if (row0 + r < N) ws[(size_t)(row0 + r) * ROW_LD + X_OF<L_JOINTS> + k] = fmaf(s.g[r][0], s.J[k * R + r], s.tJ[k * R + r]);
    }
    for (int i = t; i < NROT * R; i += ROW_THREADS) {
        const int r = i / NROT, k = i - r * NROT;
        if (row0 + r < N) ws[(size_t)(row0 + r) * ROW_LD + X_OF<L_R1> + k] = fmaf(s.g[r][2], s.rot[k * R + r], s.trot[k * R + r]);
    }
    if (t < R * 4) {  // grad_scores; the signal of the three one-output layers is 1
        const int r = t >> 2, k = t & 3;
        if (row0 + r < N) {
            float* o = ws + (size_t)(row0 + r) * ROW_LD;
            if (k < 3)
                o[G_OFF + k] = s.g[r][k];
            else
                o[S_OF<L_COMB>] = o[S_OF<L_S3>] = o[S_OF<L_R3>] = 1.f;
        }
    }
    __syncthreads();
    float acc[R], tan[R], sl1[R] = {0.f, 0.f, 0.f, 0.f};
    // ---- stage A: rotation_dense_1 (threads 0..299, which keep their slopes for stage D); the whole shapes branch, one thread per row
    if (t < 300) {
        dense_col2(w.w[L_R1], 300, NROT, t, w.b[L_R1][t], s.rot, s.trot, acc, tan);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            sl1[r] = slope(acc[r]);
            acc[r] *= sl1[r];
            tan[r] *= sl1[r];
            if (row0 + r < N) ws[(size_t)(row0 + r) * ROW_LD + X_OF<L_R2> + t] = fmaf(s.g[r][2], acc[r], tan[r]);
        }
        put(s.r1, t, acc);
        put(s.u1, t, tan);
    } else if (t >= 320 && t < 320 + R) {
        const int r = t - 320;
        if (row0 + r < N) {
            const float *W1 = w.w[L_S1], *W2 = w.w[L_S2], *W3 = w.w[L_S3];
            const float g = s.g[r][1];
            float* o = ws + (size_t)(row0 + r) * ROW_LD;
            float z1[10], v1[10], z2[5], v2[5], b2[5];
#pragma unroll
            for (int j = 0; j < 10; ++j) {
                float z = w.b[L_S1][j], v = 0.f;
#pragma unroll
                for (int k = 0; k < 10; ++k) {
                    z = fmaf(W1[k * 10 + j], s.beta[r][k], z);
                    v = fmaf(W1[k * 10 + j], s.tbeta[r][k], v);
                }
                z1[j] = z;
                v1[j] = z > 0.f ? v : 0.f;
            }
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                float z = w.b[L_S2][j], v = 0.f;
#pragma unroll
                for (int k = 0; k < 10; ++k) {
                    z = fmaf(W2[k * 5 + j], z1[k] > 0.f ? z1[k] : 0.f, z);
                    v = fmaf(W2[k * 5 + j], v1[k], v);
                }
                z2[j] = z;
                v2[j] = z > 0.f ? v : 0.f;
                b2[j] = z > 0.f ? W3[j] : 0.f;
            }
#pragma unroll
            for (int k = 0; k < 10; ++k) {
                float v = 0.f;
#pragma unroll
                for (int j = 0; j < 5; ++j) v = fmaf(W2[k * 5 + j], b2[j], v);
                o[X_OF<L_S1> + k] = fmaf(g, s.beta[r][k], s.tbeta[r][k]);
                o[X_OF<L_S2> + k] = fmaf(g, z1[k] > 0.f ? z1[k] : 0.f, v1[k]);
                o[S_OF<L_S1> + k] = z1[k] > 0.f ? v : 0.f;
            }
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                o[X_OF<L_S3> + k] = fmaf(g, z2[k] > 0.f ? z2[k] : 0.f, v2[k]);
                o[S_OF<L_S2> + k] = b2[k];
            }
        }
    }
    __syncthreads();
    // ---- stage B: rotation_dense_2 (waves 0-1), kcs_dense (waves 2-3), joints_dense (waves 4-5): combined_dense's / rotation_dense_3's
    // left operand, and the layer's own signal = (weight of the one-output layer) * slope
    {
        const int role = t >> 7, o = t & 127;
        if (role < 3 && o < 100) {
            float wn;
            int col, xo, so;
            if (role == 0) {
                dense_col2(w.w[L_R2], 100, 300, o, w.b[L_R2][o], s.r1, s.u1, acc, tan);
                wn = w.w[L_R3][o];
                col = 2, xo = X_OF<L_R3> + o, so = S_OF<L_R2> + o;
            } else if (role == 1) {
                dense_col2(w.w[L_KCS], 100, NKCS, o, w.b[L_KCS][o], s.kcs, s.tk, acc, tan);
                wn = w.w[L_COMB][o];
                col = 0, xo = X_OF<L_COMB> + o, so = S_OF<L_KCS> + o;
            } else {
                dense_col2(w.w[L_JOINTS], 100, NJF, o, w.b[L_JOINTS][o], s.J, s.tJ, acc, tan);
                wn = w.w[L_COMB][100 + o];
                col = 0, xo = X_OF<L_COMB> + 100 + o, so = S_OF<L_JOINTS> + o;
            }
            float sig[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const float sl = slope(acc[r]);
                sig[r] = wn * sl;
                if (row0 + r < N) {
                    float* q = ws + (size_t)(row0 + r) * ROW_LD;
                    q[xo] = fmaf(s.g[r][col], acc[r] * sl, tan[r] * sl);
                    q[so] = sig[r];
                }
            }
            if (role == 0) put(s.s2, o, sig);
        }
    }
    __syncthreads();
    // ---- stage D: rotation_dense_1's signal, over rotation_dense_2 transposed
    if (t < 300) {
        dense_col(w.wt[L_R2], 300, 100, t, 0.f, s.s2, acc);
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (row0 + r < N) ws[(size_t)(row0 + r) * ROW_LD + S_OF<L_R1> + t] = acc[r] * sl1[r];
    }
}

// One 64 x 64 tile of one layer's [in][out] gradient over one chunk of rows: thread (ty, tx) owns the 4 x 4 weights
// (in0 + 4 ty + i, out0 + 4 tx + j) and adds the rows of the chunk in ascending order; the threads ty == 0 of a layer's first tile
// row also own four biases.  part: [gridDim.y][CRITIC_PARAM_FLOATS]
__global__ __launch_bounds__(GEMM_THREADS) void critic_wg_gemm_kernel(const float* __restrict__ ws, long N, int has_gs,
                                                                      float* __restrict__ part) {
    __shared__ __align__(16) float As[KB][TILE];
    __shared__ __align__(16) float Ds[KB][TILE];
    __shared__ float Gs[KB];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    int l = 0;
    while (l < NL - 1 && (int)blockIdx.x >= L_TILE0[l + 1]) ++l;
    const int IN = L_IN[l], OUT = L_OUT[l];
    const int n_ot = (OUT + TILE - 1) / TILE, ti = (int)blockIdx.x - L_TILE0[l];
    const int in0 = (ti / n_ot) * TILE, out0 = (ti % n_ot) * TILE;
    const long lo = (long)blockIdx.y * CRITIC_WG_CHUNK;
    const long hi = lo + CRITIC_WG_CHUNK < N ? lo + CRITIC_WG_CHUNK : N;
    const float* xs = ws + L_X[l] + in0;
    const float* ds = ws + L_S[l] + out0;
    const float* gs = ws + G_OFF + L_COL[l];
    const bool own_bias = in0 == 0 && ty == 0;
    float acc[4][4] = {}, bias[4] = {0.f, 0.f, 0.f, 0.f};
    for (long r0 = lo; r0 < hi; r0 += KB) {
#pragma unroll
        for (int i = 0; i < KB * TILE / GEMM_THREADS; ++i) {
            const int e = t + GEMM_THREADS * i, rr = e >> 6, cc = e & 63;
            const long row = r0 + rr;
            As[rr][cc] = (row < hi && in0 + cc < IN) ? xs[(size_t)row * ROW_LD + cc] : 0.f;
            Ds[rr][cc] = (row < hi && out0 + cc < OUT) ? ds[(size_t)row * ROW_LD + cc] : 0.f;
        }
        if (t < KB) Gs[t] = (has_gs && r0 + t < hi) ? gs[(size_t)(r0 + t) * ROW_LD] : 0.f;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < KB; ++k) {
            const float4 a = *reinterpret_cast<const float4*>(&As[k][ty * 4]);
            const float4 d = *reinterpret_cast<const float4*>(&Ds[k][tx * 4]);
            const float av[4] = {a.x, a.y, a.z, a.w}, dv[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(av[i], dv[j], acc[i][j]);
            if (own_bias) {
                const float g = Gs[k];
#pragma unroll
                for (int j = 0; j < 4; ++j) bias[j] = fmaf(g, dv[j], bias[j]);
            }
        }
        __syncthreads();
    }
    float* out = part + (size_t)blockIdx.y * CRITIC_PARAM_FLOATS + L_W[l];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int k = in0 + ty * 4 + i;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int o = out0 + tx * 4 + j;
            if (k < IN && o < OUT) out[(size_t)k * OUT + o] = acc[i][j];
        }
    }
    if (own_bias) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int o = out0 + tx * 4 + j;
            if (o < OUT) out[(size_t)IN * OUT + o] = bias[j];
        }
    }
}

// out[p] = the chunks' partials added in chunk order
__global__ __launch_bounds__(256) void critic_wg_finish_kernel(const float* __restrict__ part, int n_chunks, float* __restrict__ out) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= CRITIC_PARAM_FLOATS) return;
    float v = part[p];
    for (int c = 1; c < n_chunks; ++c) v += part[(size_t)c * CRITIC_PARAM_FLOATS + p];
    out[p] = v;
}

// flat <-> live weights.  SET also rebuilds the transposed copies [out][in] that the backward reads.
template <bool SET>
__global__ __launch_bounds__(256) void critic_params_kernel(CriticW w, float* __restrict__ flat) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= CRITIC_PARAM_FLOATS) return;
    int l = 0;
    while (l < NL - 1 && p >= L_W[l + 1]) ++l;
    const int IN = L_IN[l], OUT = L_OUT[l], q = p - L_W[l];
    if (q < IN * OUT) {
        if (SET) {
            const float v = flat[p];
            const int k = q / OUT, o = q - k * OUT;
            const_cast<float*>(w.w[l])[q] = v;
            const_cast<float*>(w.wt[l])[(size_t)o * IN + k] = v;
        } else {
            flat[p] = w.w[l][q];
        }
    } else {
        if (SET)
            const_cast<float*>(w.b[l])[q - IN * OUT] = flat[p];
        else
            flat[p] = w.b[l][q - IN * OUT];
    }
}

}  // namespace

int hpe_critic_wg_chunks(long N) { return (int)((N + CRITIC_WG_CHUNK - 1) / CRITIC_WG_CHUNK); }

size_t hpe_critic_wg_ws_floats(long N) {
    const int nc = hpe_critic_wg_chunks(N);
    return (size_t)N * ROW_LD + (nc > 1 ? (size_t)nc * CRITIC_PARAM_FLOATS : 0);
}

hipError_t hpe_launch_critic_weight_grad(const CriticW& w, const float* joints, int K, const float* betas, int betas_stride, const float* Rs,
                                         long N, const float* grad_scores, const float* t_kcs, const float* t_joints, const float* t_betas,
                                         const float* t_Rs, int tangent_per_row, float* ws, float* grad_params, hipStream_t st) {
    const Tangents tg{t_kcs, t_joints, t_betas, t_Rs, tangent_per_row ? 1 : 0};
    const int nc = hpe_critic_wg_chunks(N);
    float* part = nc > 1 ? ws + (size_t)N * ROW_LD : grad_params;
    hipLaunchKernelGGL(critic_wg_rows_kernel, dim3((unsigned)((N + R - 1) / R)), dim3(ROW_THREADS), 0, st, w, joints, K, betas, betas_stride,
                       Rs, N, grad_scores, tg, ws);
    hipLaunchKernelGGL(critic_wg_gemm_kernel, dim3(N_TILES, (unsigned)nc), dim3(GEMM_THREADS), 0, st, ws, N, grad_scores ? 1 : 0, part);
    if (nc > 1)
        hipLaunchKernelGGL(critic_wg_finish_kernel, dim3((CRITIC_PARAM_FLOATS + 255) / 256), dim3(256), 0, st, part, nc, grad_params);
    return hipGetLastError();
}

hipError_t hpe_launch_critic_params(const CriticW& w, float* flat, bool set, hipStream_t st) {
    const dim3 grid((CRITIC_PARAM_FLOATS + 255) / 256);
    if (set)
        hipLaunchKernelGGL(critic_params_kernel<true>, grid, dim3(256), 0, st, w, flat);
    else
        hipLaunchKernelGGL(critic_params_kernel<false>, grid, dim3(256), 0, st, w, flat);
    return hipGetLastError();
}

int hpe_critic_flat_offset(int idx, bool bias) {  // idx == HPE_NUM_CRITIC_DENSE, bias false: the total, CRITIC_PARAM_FLOATS
    return LAYOUT.w[idx] + (bias ? LAYOUT.in[idx] * LAYOUT.out[idx] : 0);
}
