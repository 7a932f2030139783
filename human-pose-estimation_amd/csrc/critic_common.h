// critic_common.h -- what critic.hip and critic_train.hip share: the one C++ statement of the critic's nine Dense layers, every layout
// derived from it (flat parameters, workspace row, tile schedule of the weight-gradient reduction), and the small device helpers of the
// row-tile kernels.  Included by those two files only: everything here has internal linkage, one copy per translation unit.
#pragma once
#include <hip/hip_runtime.h>

#include "hpe_internal.h"

namespace {

constexpr int R = CRITIC_ROWS;
static_assert(R == 4, "the tile is read as one float4 per k");
constexpr int NJ = 14, NB = 13, NJF = 42, NKCS = 169, NROT = 207, NBETA = 10;
constexpr int NL = HPE_NUM_CRITIC_DENSE;
constexpr int WG_TILE = 64;  // output tile of the weight gradient's row-reduction GEMM

// Three branches of three layers; branch l / 3 feeds score column l / 3.  The activations (leaky ReLU 0.2 after kcs_dense, joints_dense,
// rotation_dense_1/2; ReLU after shapes_dense_1/2; none after the three one-output layers) are in the kernels.
constexpr CriticLayerSpec LAYERS[NL] = {
    {"kcs_dense", NKCS, 100},       {"joints_dense", NJF, 100},     {"combined_dense", 200, 1},
    {"shapes_dense_1", NBETA, 10},  {"shapes_dense_2", 10, 5},      {"shapes_dense_3", 5, 1},
    {"rotation_dense_1", NROT, 300}, {"rotation_dense_2", 300, 100}, {"rotation_dense_3", 100, 1},
};
enum { L_KCS = 0, L_JOINTS = 1, L_COMB = 2, L_S1 = 3, L_S2 = 4, L_S3 = 5, L_R1 = 6, L_R2 = 7, L_R3 = 8 };

template <int N>
struct Table {  // an int array that can be copied, so that a __constant__ table is initialised from its constexpr twin
    int v[N];
    constexpr int operator[](int i) const { return v[i]; }
};

struct Layout {
    Table<NL> in, out;
    Table<NL + 1> w;      // flat parameters: kernel l [in][out] at w[l], bias l right behind it; w[NL]: the total
    Table<NL> x, s;       // workspace row: left operands of the nine layers | signals of the nine layers | grad_scores (3)
    int nx, g_off, row;   // end of the left operands; grad_scores; floats per row
    Table<NL + 1> tile0;  // first WG_TILE x WG_TILE tile of layer l's [in][out] gradient; tile0[NL]: the tile count
    Table<NL> col;        // the score column layer l feeds
};

constexpr Layout make_layout() {
    Layout t{};
    int w = 0, x = 0, tiles = 0;
    for (int l = 0; l < NL; ++l) {
        const int in = LAYERS[l].in, out = LAYERS[l].out;
        t.in.v[l] = in;
        t.out.v[l] = out;
        t.w.v[l] = w;
        w += in * out + out;
        t.x.v[l] = x;
        x += in;
        t.tile0.v[l] = tiles;
        tiles += ((in + WG_TILE - 1) / WG_TILE) * ((out + WG_TILE - 1) / WG_TILE);
        t.col.v[l] = l / 3;
    }
    t.w.v[NL] = w;
    t.tile0.v[NL] = tiles;
    t.nx = x;
    for (int l = 0; l < NL; ++l) {
        t.s.v[l] = x;
        x += LAYERS[l].out;
    }
    t.g_off = x;
    t.row = x + 3;
    return t;
}
constexpr Layout LAYOUT = make_layout();

constexpr int NX = LAYOUT.nx, G_OFF = LAYOUT.g_off, ROW_LD = LAYOUT.row, N_TILES = LAYOUT.tile0[NL];
template <int L>
constexpr int X_OF = LAYOUT.x[L];  // workspace offset of layer L's left operand
template <int L>
constexpr int S_OF = LAYOUT.s[L];  // ... of its signal

// The layouts as they were when they were written out by hand: a change to the table that moves one of them has to be meant.
template <int N>
constexpr bool same(const Table<N>& t, const int (&v)[N]) {
    for (int i = 0; i < N; ++i)
        if (t[i] != v[i]) return false;
    return true;
}
static_assert(LAYOUT.w[NL] == CRITIC_PARAM_FLOATS && ROW_LD == CRITIC_WG_ROW_FLOATS && N_TILES == 47, "critic layout totals");
static_assert(same(LAYOUT.w, {0, 17000, 21300, 21501, 21611, 21666, 21672, 84072, 114172, 114273}), "flat parameter offsets");
static_assert(same(LAYOUT.x, {0, 169, 211, 411, 421, 431, 436, 643, 943}) && NX == 1043, "workspace row: left operands");
static_assert(same(LAYOUT.s, {1043, 1143, 1243, 1244, 1254, 1259, 1260, 1560, 1660}) && G_OFF == 1661, "workspace row: signals");
static_assert(same(LAYOUT.tile0, {0, 6, 8, 12, 13, 14, 15, 35, 45, 47}), "tile schedule");
static_assert(same(LAYOUT.col, {0, 0, 0, 1, 1, 1, 2, 2, 2}), "score columns");

// precompute_C_matrix (src/models.py:97-112): bone b = joint b - joint BONE_MINUS[b]
__constant__ int BONE_MINUS[NB] = {1, 2, 8, 9, 3, 4, 7, 8, 12, 12, 9, 10, 13};

__device__ __forceinline__ float slope(float z) { return z > 0.f ? 1.f : 0.2f; }  // tf.nn.leaky_relu, alpha 0.2

// acc[r] = init + sum over k (ascending) of W[k * ld + o] * xs[k][r]
__device__ __forceinline__ void dense_col(const float* __restrict__ W, int ld, int K, int o, float init, const float* xs, float acc[R]) {
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = init;
    const float* w = W + o;
#pragma unroll 8
    for (int k = 0; k < K; ++k) {
        const float wk = w[(size_t)k * ld];
        const float4 x = *reinterpret_cast<const float4*>(xs + k * R);
        acc[0] = fmaf(wk, x.x, acc[0]);
        acc[1] = fmaf(wk, x.y, acc[1]);
        acc[2] = fmaf(wk, x.z, acc[2]);
        acc[3] = fmaf(wk, x.w, acc[3]);
    }
}

__device__ __forceinline__ void put(float* xs, int o, const float v[R]) {
    *reinterpret_cast<float4*>(xs + o * R) = make_float4(v[0], v[1], v[2], v[3]);
}

}  // namespace
