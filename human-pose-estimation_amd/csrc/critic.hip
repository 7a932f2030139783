// critic.hip -- the reference's CriticNetwork + get_kcs (src/models.py:97-202) and the gradient of its scores with respect to its inputs.
//
// Nine fp32 Dense layers in three branches (table: hpe_critic_layers()).  One launch for the forward, one for the backward: a workgroup
// takes CRITIC_ROWS rows, keeps every activation in LDS (transposed, [k][row], so that one ds_read_b128 serves the tile) and streams the
// weights from L2 in their Keras layout [in][out]: thread o reads W[k][o], coalesced over the outputs, and uses it for every row of the tile.
//
// Summation order: ONE thread owns one output of one layer for all rows of the tile and adds its k terms in ascending k with fmaf, starting
// from the bias.  No k axis is split, nothing is reduced across threads, no atomics: a row's bits do not depend on N, on the tile it lands
// in, or on its slot in that tile (the slots run the same instruction sequence).  The backward recomputes the hidden pre-activations with
// the forward's own loops and walks the transposed weight copies [out][in] (critic_params_kernel<true> of critic_train.hip writes them
// beside the kernels) the same way.
#include <hip/hip_runtime.h>

#include "critic_common.h"

namespace {

constexpr int FWD_THREADS = 384, BWD_THREADS = 512;

struct Tile {  // LDS image of one tile; every [k][R] array is read as float4 per k
    float J[NJF * R];
    float kcs[NKCS * R];
    float rot[NROT * R];
    float r1[300 * R];  // rotation_dense_1 activations; backward: later d L / d z1
    float r2[100 * R];  // rotation_dense_2 activations; backward: d L / d z2
    float h[200 * R];   // [kcs_dense | joints_dense] activations; backward: d L / d z
    float beta[R][NBETA];
    float g[R][4];         // backward: grad_scores of the tile's rows
    float dj[NJF * R];     // backward: joints_dense's share of d L / d J
    float gk[NKCS * R];    // backward: d L / d KCS
    float dB[R][3][NB];    // backward: d L / d B
};

// inputs of the tile's rows -> LDS (rows past N read as zeros), then KCS = B^T B with B = J^T C, its three terms added in coordinate order
__device__ void load_tile(Tile& s, const float* joints, int K, const float* betas, int betas_stride, const float* Rs, long row0, long N,
                          float* kcs_out) {
    const int t = threadIdx.x, nt = blockDim.x;
    for (int i = t; i < NJF * R; i += nt) {
        const int r = i / NJF, k = i - r * NJF;
        const long row = row0 + r;
        s.J[k * R + r] = row < N ? joints[(size_t)row * K * 3 + k] : 0.f;
    }
    for (int i = t; i < NROT * R; i += nt) {
        const int r = i / NROT, k = i - r * NROT;
        const long row = row0 + r;
        s.rot[k * R + r] = row < N ? Rs[(size_t)row * 216 + 9 + k] : 0.f;
    }
    for (int i = t; i < NBETA * R; i += nt) {
        const int r = i / NBETA, k = i - r * NBETA;
        const long row = row0 + r;
        s.beta[r][k] = row < N ? betas[(size_t)row * betas_stride + k] : 0.f;
    }
    __syncthreads();
    for (int i = t; i < NKCS * R; i += nt) {
        const int r = i / NKCS, m = i - r * NKCS;
        const int a = m / NB, b = m - a * NB;
        const int am = BONE_MINUS[a], bm = BONE_MINUS[b];
        float v = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float Ba = s.J[(a * 3 + c) * R + r] - s.J[(am * 3 + c) * R + r];
            const float Bb = s.J[(b * 3 + c) * R + r] - s.J[(bm * 3 + c) * R + r];
            v = fmaf(Ba, Bb, v);
        }
        s.kcs[m * R + r] = v;
        const long row = row0 + r;
        if (kcs_out && row < N) kcs_out[(size_t)row * NKCS + m] = v;
    }
    __syncthreads();
}

// the shapes branch of one row, forward and (GRAD) backward, in one thread: 155 multiply-adds, every loop unrolled into registers
template <bool GRAD>
__device__ __forceinline__ float shapes_branch(const CriticW& w, const float* beta, float g, float* dbeta) {
    const float *W1 = w.w[L_S1], *W2 = w.w[L_S2], *W3 = w.w[L_S3];
    float z1[10], z2[5];
#pragma unroll
    for (int o = 0; o < 10; ++o) {
        float z = w.b[L_S1][o];
#pragma unroll
        for (int k = 0; k < 10; ++k) z = fmaf(W1[k * 10 + o], beta[k], z);
        z1[o] = z;
    }
#pragma unroll
    for (int o = 0; o < 5; ++o) {
        float z = w.b[L_S2][o];
#pragma unroll
        for (int k = 0; k < 10; ++k) z = fmaf(W2[k * 5 + o], z1[k] > 0.f ? z1[k] : 0.f, z);
        z2[o] = z;
    }
    float sc = w.b[L_S3][0];
#pragma unroll
    for (int k = 0; k < 5; ++k) sc = fmaf(W3[k], z2[k] > 0.f ? z2[k] : 0.f, sc);
    if (GRAD) {
        float d2[5], d1[10];
#pragma unroll
        for (int k = 0; k < 5; ++k) d2[k] = z2[k] > 0.f ? g * W3[k] : 0.f;
#pragma unroll
        for (int k = 0; k < 10; ++k) {
            float v = 0.f;
#pragma unroll
            for (int o = 0; o < 5; ++o) v = fmaf(W2[k * 5 + o], d2[o], v);
            d1[k] = z1[k] > 0.f ? v : 0.f;
        }
#pragma unroll
        for (int k = 0; k < 10; ++k) {
            float v = 0.f;
#pragma unroll
            for (int o = 0; o < 10; ++o) v = fmaf(W1[k * 10 + o], d1[o], v);
            dbeta[k] = v;
        }
    }
    return sc;
}

__global__ __launch_bounds__(FWD_THREADS) void critic_fwd_kernel(CriticW w, const float* __restrict__ joints, int K,
                                                                 const float* __restrict__ betas, int betas_stride,
                                                                 const float* __restrict__ Rs, long N, float* __restrict__ scores,
                                                                 float* __restrict__ kcs_out) {
    __shared__ __align__(16) Tile s;
    const int t = threadIdx.x;
    const long row0 = (long)blockIdx.x * R;
    load_tile(s, joints, K, betas, betas_stride, Rs, row0, N, kcs_out);
    float acc[R];
    // stage A: rotation_dense_1 (threads 0..299); the shapes branch, one thread per row (wave 5)
    if (t < 300) {
        dense_col(w.w[L_R1], 300, NROT, t, w.b[L_R1][t], s.rot, acc);
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] *= slope(acc[r]);
        put(s.r1, t, acc);
    } else if (t >= 320 && t < 320 + R) {
        const int r = t - 320;
        const float sc = shapes_branch<false>(w, s.beta[r], 0.f, nullptr);
        if (row0 + r < N) scores[(size_t)(row0 + r) * 3 + 1] = sc;
    }
    __syncthreads();
    // stage B: rotation_dense_2 (waves 0-1), kcs_dense (waves 2-3), joints_dense (waves 4-5)
    {
        const int role = t >> 7, o = t & 127;
        if (o < 100) {
            if (role == 0) {
                dense_col(w.w[L_R2], 100, 300, o, w.b[L_R2][o], s.r1, acc);
#pragma unroll
                for (int r = 0; r < R; ++r) acc[r] *= slope(acc[r]);
                put(s.r2, o, acc);
            } else if (role == 1) {
                dense_col(w.w[L_KCS], 100, NKCS, o, w.b[L_KCS][o], s.kcs, acc);
#pragma unroll
                for (int r = 0; r < R; ++r) acc[r] *= slope(acc[r]);
                put(s.h, o, acc);
            } else {
                dense_col(w.w[L_JOINTS], 100, NJF, o, w.b[L_JOINTS][o], s.J, acc);
#pragma unroll
                for (int r = 0; r < R; ++r) acc[r] *= slope(acc[r]);
                put(s.h, 100 + o, acc);
            }
        }
    }
    __syncthreads();
    // stage C: the two one-output layers, one thread each for the whole tile (waves 0 and 1)
    if (t == 0) {
        dense_col(w.w[L_COMB], 1, 200, 0, w.b[L_COMB][0], s.h, acc);
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (row0 + r < N) scores[(size_t)(row0 + r) * 3] = acc[r];
    } else if (t == 64) {
        dense_col(w.w[L_R3], 1, 100, 0, w.b[L_R3][0], s.r2, acc);
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (row0 + r < N) scores[(size_t)(row0 + r) * 3 + 2] = acc[r];
    }
}

__global__ __launch_bounds__(BWD_THREADS) void critic_bwd_kernel(CriticW w, const float* __restrict__ joints, int K,
                                                                 const float* __restrict__ betas, int betas_stride,
                                                                 const float* __restrict__ Rs, long N, const float* __restrict__ gscores,
                                                                 float* __restrict__ gjoints, float* __restrict__ gbetas,
                                                                 float* __restrict__ gRs, float* __restrict__ gkcs) {
    __shared__ __align__(16) Tile s;
    const int t = threadIdx.x;
    const long row0 = (long)blockIdx.x * R;
    if (t < R * 3) {
        const int r = t / 3, k = t - r * 3;
        s.g[r][k] = gscores ? (row0 + r < N ? gscores[(size_t)(row0 + r) * 3 + k] : 0.f) : 1.f;
    }
    load_tile(s, joints, K, betas, betas_stride, Rs, row0, N, nullptr);
    float acc[R], sl1[R] = {0.f, 0.f, 0.f, 0.f};
    // stage A: as the forward; thread o keeps the slope of its rotation_dense_1 output for stage D
    if (t < 300) {
        dense_col(w.w[L_R1], 300, NROT, t, w.b[L_R1][t], s.rot, acc);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            sl1[r] = slope(acc[r]);
            acc[r] *= sl1[r];
        }
        put(s.r1, t, acc);
    } else if (t >= 320 && t < 320 + R) {
        const int r = t - 320;
        float db[NBETA];
        (void)shapes_branch<true>(w, s.beta[r], s.g[r][1], db);
        if (gbetas && row0 + r < N) {
#pragma unroll
            for (int k = 0; k < NBETA; ++k) gbetas[(size_t)(row0 + r) * NBETA + k] = db[k];
        }
    }
    __syncthreads();
    // stage B: the second hidden layers again, but what is kept is d L / d z = grad_score * (weight of the one-output layer) * slope(z)
    {
        const int role = t >> 7, o = t & 127;
        if (role < 3 && o < 100) {
            float wn;
            int col;
            if (role == 0) {
                dense_col(w.w[L_R2], 100, 300, o, w.b[L_R2][o], s.r1, acc);
                wn = w.w[L_R3][o];
                col = 2;
            } else if (role == 1) {
                dense_col(w.w[L_KCS], 100, NKCS, o, w.b[L_KCS][o], s.kcs, acc);
                wn = w.w[L_COMB][o];
                col = 0;
            } else {
                dense_col(w.w[L_JOINTS], 100, NJF, o, w.b[L_JOINTS][o], s.J, acc);
                wn = w.w[L_COMB][100 + o];
                col = 0;
            }
#pragma unroll
            for (int r = 0; r < R; ++r) acc[r] = s.g[r][col] * wn * slope(acc[r]);
            put(role == 0 ? s.r2 : s.h, role == 2 ? 100 + o : o, acc);
        }
    }
    __syncthreads();
    // stage D: d L / d z1 (threads 0..299, over rotation_dense_2 transposed); d L / d KCS (threads 320..488, over kcs_dense transposed)
    if (t < 300) {
        dense_col(w.wt[L_R2], 300, 100, t, 0.f, s.r2, acc);
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] *= sl1[r];
        put(s.r1, t, acc);
    } else if (t >= 320 && t < 320 + NKCS) {
        const int m = t - 320;
        dense_col(w.wt[L_KCS], NKCS, 100, m, 0.f, s.h, acc);
        put(s.gk, m, acc);
        if (gkcs) {
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (row0 + r < N) gkcs[(size_t)(row0 + r) * NKCS + m] = acc[r];
        }
    }
    __syncthreads();
    // stage E: d L / d Rs (threads 0..206); joints_dense's share of d L / d J (wave 4); d L / d B = B (G + G^T) (waves 5-7)
    if (t < NROT) {
        dense_col(w.wt[L_R1], NROT, 300, t, 0.f, s.r1, acc);
        if (gRs) {
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (row0 + r < N) {
                    gRs[(size_t)(row0 + r) * 216 + 9 + t] = acc[r];
                    if (t < 9) gRs[(size_t)(row0 + r) * 216 + t] = 0.f;  // the root rotation is not an input
                }
        }
    } else if (t >= 256 && t < 256 + NJF) {
        const int m = t - 256;
        dense_col(w.wt[L_JOINTS], NJF, 100, m, 0.f, s.h + 100 * R, acc);
        put(s.dj, m, acc);
    } else if (t >= 320 && t < 320 + R * 3 * NB) {
        const int i = t - 320;
        const int r = i / (3 * NB), c = (i - r * 3 * NB) / NB, b = i % NB;
        float v = 0.f;
        for (int a = 0; a < NB; ++a) {
            const float Ba = s.J[(a * 3 + c) * R + r] - s.J[(BONE_MINUS[a] * 3 + c) * R + r];
            v = fmaf(Ba, s.gk[(a * NB + b) * R + r] + s.gk[(b * NB + a) * R + r], v);
        }
        s.dB[r][c][b] = v;
    }
    __syncthreads();
    // stage F: d L / d J = joints_dense's share + (d L / d B) C^T: + bone j (j < 13), - every bone b whose minus end is joint j, b ascending
    if (gjoints) {
        for (int i = t; i < R * K * 3; i += BWD_THREADS) {
            const int r = i / (K * 3), m = i - r * K * 3;
            if (row0 + r >= N) continue;
            float v = 0.f;
            if (m < NJF) {
                const int j = m / 3, c = m - j * 3;
                v = s.dj[m * R + r];
                if (j < NB) v += s.dB[r][c][j];
                for (int b = 0; b < NB; ++b)
                    if (BONE_MINUS[b] == j) v -= s.dB[r][c][b];
            }
            gjoints[(size_t)(row0 + r) * K * 3 + m] = v;  // joints 14..K-1 are not inputs
        }
    }
}

// The live weights, one buffer: per layer kernel [in][out] | its transpose [out][in] | bias, every block on a 16-byte boundary
struct Live {
    size_t w[NL], wt[NL], b[NL], total;
};
constexpr Live make_live() {
    Live v{};
    size_t off = 0;
    for (int l = 0; l < NL; ++l) {
        const size_t kernel = (size_t)(LAYOUT.in[l] * LAYOUT.out[l] + 3) / 4 * 4, bias = (size_t)(LAYOUT.out[l] + 3) / 4 * 4;
        v.w[l] = off;
        v.wt[l] = off + kernel;
        v.b[l] = off + 2 * kernel;
        off += 2 * kernel + bias;
    }
    v.total = off;
    return v;
}
constexpr Live LIVE = make_live();

}  // namespace

const CriticLayerSpec* hpe_critic_layers() { return LAYERS; }

size_t hpe_critic_live_floats() { return LIVE.total; }

CriticW hpe_critic_live_view(const float* buf) {
    CriticW w{};
    for (int l = 0; l < NL; ++l) {
        w.w[l] = buf + LIVE.w[l];
        w.wt[l] = buf + LIVE.wt[l];
        w.b[l] = buf + LIVE.b[l];
    }
    return w;
}

hipError_t hpe_launch_critic(const CriticW& w, const float* joints, int K, const float* betas, int betas_stride, const float* Rs, long N,
                             float* scores, float* kcs, hipStream_t st) {
    const unsigned grid = (unsigned)((N + R - 1) / R);
    hipLaunchKernelGGL(critic_fwd_kernel, dim3(grid), dim3(FWD_THREADS), 0, st, w, joints, K, betas, betas_stride, Rs, N, scores, kcs);
    return hipGetLastError();
}

hipError_t hpe_launch_critic_backward(const CriticW& w, const float* joints, int K, const float* betas, int betas_stride, const float* Rs,
                                      long N, const float* grad_scores, float* grad_joints, float* grad_betas, float* grad_Rs,
                                      float* grad_kcs, hipStream_t st) {
    const unsigned grid = (unsigned)((N + R - 1) / R);
    hipLaunchKernelGGL(critic_bwd_kernel, dim3(grid), dim3(BWD_THREADS), 0, st, w, joints, K, betas, betas_stride, Rs, N, grad_scores,
                       grad_joints, grad_betas, grad_Rs, grad_kcs);
    return hipGetLastError();
}
