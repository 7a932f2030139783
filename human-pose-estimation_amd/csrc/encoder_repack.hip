// encoder_repack.hip -- hpe_encoder_set_params_dev: the flat device parameters of the encoder (kernel HWIO | bias | gamma | beta per layer)
// into every packing an fp32 context holds, in stream order: no host copy, no synchronisation, no allocation, capturable.
//
// The host packers of hpe_finalize.hip and pack_dx_weights (encoder_train.hip) stay what hpe_finalize, the bf16 contexts and
// hpe_encoder_set_params run, and they are the reference: every kernel here must write the bits they write.  Each packing is a gather
// with the OUTPUT index as the thread index, so the stores are coalesced and the scattered side is the reads (94 MB, L2-friendly: a
// workgroup that transposes reads each line it touches completely).  The permutations and the bf16 split are exact.  The folded values
// (BatchNorm scale / shift, the dual-source weights, both Winograd forms) are computed in double by the __host__ __device__ helpers of
// hpe_ctx.h the host packers call too: the same operations in the same order with contraction off, and fp64 + * / are correctly rounded on
// gfx950.  The one sqrt is not taken here: hpe_encoder_train_reserve stores sqrt(var + eps) per channel, in double (EncTrainWork::sd),
// and hpe_encoder_set_stats_dev rewrites it on the device with a correctly rounded sqrt (encoder_bn.hip) before it reruns the two
// kernels that fold the statistics (encoder_repack_stats_launch).
//
// One launch per form, not per layer: a form's grid is the concatenation of its layers' workgroups, and RepackForm says which layer a
// workgroup belongs to (a scan of at most 53 workgroup-uniform entries).  The table is built once, by hpe_encoder_train_reserve, from the
// pointers of the finalized context: a form a context does not hold (pointer NULL) is not in it.  Seven launches and one copy in all.
#include <hip/hip_runtime.h>

#include <string>

#include "hpe_ctx.h"

namespace {

struct RepackLayer {
    float *w, *scale, *shift, *wino_u, *wino4_u, *dxw;
    unsigned short* w_split;
    // wino_split: wino_u is followed by ConvLayer::wino_u_split in the same allocation (pack_wino_weights; wino_u_split_of in hpe_ctx.h is the
    // one place that says where).  A flag beside kh, not a pointer: sizeof(RepackTable) sizes the device update's reserve, and
    // tests/encoder_train_ref.py restates that size.
    short kh, wino_split;
    int cin, cout, n_pad, k_pad;
    int off[4];  // kernel, bias, gamma, beta in the flat layout
    int stat;    // first channel in EncTrainWork::mean / sd
};

struct RepackDual {  // a conv_block's [s2c W2c | s1 W1]
    float *w, *shift;
    unsigned short* split;
    int i2c, i1, K1, K2, N, n_pad;
};

enum { F_WT, F_BN, F_WINO, F_WINO4, F_DXW, F_DUAL, F_COUNT };

struct RepackForm {
    int n;                               // segments
    int item[HPE_NUM_CONV];              // the layer (F_DUAL: the RepackDual) of segment s
    unsigned block0[HPE_NUM_CONV + 1];   // its first workgroup; [n] = the grid
};

struct RepackTable {
    RepackLayer L[HPE_NUM_CONV];
    RepackDual D[4];
    RepackForm F[F_COUNT];
};

constexpr int TILE_N = 32, TILE_K = 64;  // a transposing workgroup: 64 consecutive k per wave (the stores), 8 rows n per thread

// the item of workgroup b of form f and b's index inside that item (workgroup-uniform)
__device__ inline int find_item(const RepackForm& f, unsigned b, unsigned* local) {
    int s = 0;
    while (s + 1 < f.n && f.block0[s + 1] <= b) ++s;
    *local = b - f.block0[s];
    return f.item[s];
}

__device__ inline void store_split(unsigned short* d, size_t piece, float x) {
    unsigned short h[3];
    bf16_split3(x, h);
    d[0] = h[0];
    d[piece] = h[1];
    d[2 * piece] = h[2];
}

// ConvLayer::w = Wt[n_pad][k_pad] (the inverse of conv_wt_k: k -> the row of the [K][cout] HWIO matrix), zero in the padding, and w_split
__global__ __launch_bounds__(256) void repack_wt_kernel(const RepackTable* __restrict__ T, const float* __restrict__ flat) {
    unsigned lb;
    const int idx = find_item(T->F[F_WT], blockIdx.x, &lb);
    const RepackLayer& L = T->L[idx];
    const int kt_n = (L.k_pad + TILE_K - 1) / TILE_K;
    const int nt = lb / kt_n, kt = lb - nt * kt_n;
    const int k = kt * TILE_K + (threadIdx.x & 63);
    if (k >= L.k_pad) return;
    long row = -1;  // conv1: k = kh * 32 + kw * 4 + ci, 8 px x 4 ch per kernel row (pixel 7 and channel 3 are zero weights)
    if (idx == 0) {
        const int kh = k >> 5, kw = (k & 31) >> 2, ci = k & 3;
        if (kh < 7 && kw < 7 && ci < 3) row = (kh * 7 + kw) * 3 + ci;
    } else if (k < L.kh * L.kh * L.cin) {
        row = k;
    }
    const float* src = flat + L.off[0];
    const int n0 = nt * TILE_N + (threadIdx.x >> 6) * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int n = n0 + j;
        if (n >= L.n_pad) break;
        const float v = (row >= 0 && n < L.cout) ? src[row * L.cout + n] : 0.f;
        L.w[(size_t)n * L.k_pad + k] = v;
        if (L.w_split) store_split(L.w_split + (size_t)n * 3 * L.k_pad + k, L.k_pad, v);
    }
}

// scale / shift of every channel (bn_fold)
__global__ __launch_bounds__(256) void repack_bn_kernel(const RepackTable* __restrict__ T, const float* __restrict__ flat,
                                                        const float* __restrict__ mean, const double* __restrict__ sd) {
    unsigned lb;
    const RepackLayer& L = T->L[find_item(T->F[F_BN], blockIdx.x, &lb)];
    const int n = lb * 256 + threadIdx.x;
    if (n >= L.cout) return;
    double scale, shift;
    bn_fold_sd(flat[L.off[2] + n], flat[L.off[1] + n], mean[L.stat + n], flat[L.off[3] + n], sd[L.stat + n], &scale, &shift);
    L.scale[n] = (float)scale;
    L.shift[n] = (float)shift;
}

// conv1's fused-stem weights, the three bf16 pieces [3][64][7][32] of Wt[n][k = kh * 32 + kw * 4 + ci] (zero for kw = 7 and ci = 3)
__global__ __launch_bounds__(256) void repack_stem_kernel(unsigned short* __restrict__ stem_w, const float* __restrict__ kernel) {
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= 64 * 224) return;
    const int n = o / 224, k = o - n * 224;
    const int kh = k >> 5, kw = (k & 31) >> 2, ci = k & 3;
    float v = 0.f;
    if (kw < 7 && ci < 3) v = kernel[((kh * 7 + kw) * 3 + ci) * 64 + n];
    store_split(stem_w + o, 64 * 224, v);
}

// both Winograd forms: one thread per (ci, n), consecutive threads along the [64 n][4 ci] inner block of the layouts, so each of the
// T * T stores of a workgroup is 1 KB contiguous.  T = 4: F(2x2,3x3), T = 6: F(4x4,3x3)
template <int TT>
__global__ __launch_bounds__(256) void repack_wino_kernel(const RepackTable* __restrict__ T, const float* __restrict__ flat) {
    unsigned lb;
    const RepackLayer& L = T->L[find_item(T->F[TT == 4 ? F_WINO : F_WINO4], blockIdx.x, &lb)];
    const int c4 = L.cin / 4;
    const int nb = lb / c4, cb = lb - nb * c4;
    const int n = nb * 64 + (threadIdx.x >> 2), ci = cb * 4 + (threadIdx.x & 3);
    const float* src = flat + L.off[0];
    double g[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) g[a][b] = src[(((size_t)a * 3 + b) * L.cin + ci) * L.cout + n];
    float* out = TT == 4 ? L.wino_u + wino_u_base(n, ci, L.cin) : L.wino4_u + wino4_u_base(n, ci, L.cin);
    constexpr size_t step = TT == 4 ? 512 : 256;
#pragma unroll
    for (int xi = 0; xi < TT; ++xi)
#pragma unroll
        for (int nu = 0; nu < TT; ++nu) {
            double gx[3], gn[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                gx[a] = TT == 4 ? wino_g(xi, a) : wino4_g(xi, a);
                gn[a] = TT == 4 ? wino_g(nu, a) : wino4_g(nu, a);
            }
            const float u = wino_elem(gx, gn, g);
            out[(size_t)(xi * TT + nu) * step] = u;
            if (TT == 4 && L.wino_split)
                store_split(wino_u_split_of(L.wino_u, L.cin, L.cout) + wino_us_base(n, ci, L.cin) + (size_t)(xi * 4 + nu) * 512, WINO_US_PIECE, u);
        }
}

// EncTrainWork::dxw = Wt[cin padded to 128][(flipped tap, cout)]: reads and stores both run along cout
__global__ __launch_bounds__(256) void repack_dxw_kernel(const RepackTable* __restrict__ T, const float* __restrict__ flat) {
    unsigned lb;
    const RepackLayer& L = T->L[find_item(T->F[F_DXW], blockIdx.x, &lb)];
    const int taps = L.kh * L.kh, K = taps * L.cout;
    const unsigned o = lb * 256 + threadIdx.x;  // < 2^23: the largest operand is 512 x 9 x 512
    const int ci = (int)(o / (unsigned)K), r = (int)(o - (unsigned)ci * K);
    if (ci >= ((L.cin + 127) / 128) * 128) return;
    const int t = r / L.cout, n = r - t * L.cout;
    L.dxw[o] = ci < L.cin ? flat[L.off[0] + ((size_t)(taps - 1 - t) * L.cin + ci) * L.cout + n] : 0.f;
}

// w_dual = [s2c W2c | s1 W1] as Wt[n_pad][K1 + K2] with the scales folded in (double product, one rounding), its split, and
// shift_dual = shift2c + shift1 (pack_dual_weights)
__global__ __launch_bounds__(256) void repack_dual_kernel(const RepackTable* __restrict__ T, const float* __restrict__ flat,
                                                          const float* __restrict__ mean, const double* __restrict__ sd) {
#pragma clang fp contract(off)
    unsigned lb;
    const RepackDual& D = T->D[find_item(T->F[F_DUAL], blockIdx.x, &lb)];
    const int K = D.K1 + D.K2;
    const int kt_n = (K + TILE_K - 1) / TILE_K;
    const int nt = lb / kt_n, kt = lb - nt * kt_n;
    const int k = kt * TILE_K + (threadIdx.x & 63);
    if (k >= K) return;
    const RepackLayer &L2 = T->L[D.i2c], &L1 = T->L[D.i1];
    const RepackLayer& L = k < D.K1 ? L2 : L1;
    const float* src = flat + L.off[0] + (size_t)(k < D.K1 ? k : k - D.K1) * D.N;
    const int n0 = nt * TILE_N + (threadIdx.x >> 6) * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int n = n0 + j;
        if (n >= D.n_pad) break;
        float v = 0.f;
        if (n < D.N) {
            double inv, shift;
            bn_fold_sd(flat[L.off[2] + n], flat[L.off[1] + n], mean[L.stat + n], flat[L.off[3] + n], sd[L.stat + n], &inv, &shift);
            v = (float)(inv * (double)src[n]);
            if (k == 0) {  // this thread's side is branch2c
                double inv1, shift1;
                bn_fold_sd(flat[L1.off[2] + n], flat[L1.off[1] + n], mean[L1.stat + n], flat[L1.off[3] + n], sd[L1.stat + n], &inv1, &shift1);
                D.shift[n] = (float)(shift + shift1);
            }
        }
        D.w[(size_t)n * K + k] = v;
        if (D.split) store_split(D.split + (size_t)n * 3 * K + k, K, v);
    }
}

unsigned blocks_of(int form, const ConvSpec& s, const ConvLayer& L, int idx) {
    switch (form) {
        case F_WT: return (unsigned)(L.n_pad / TILE_N) * ((L.k_pad + TILE_K - 1) / TILE_K);
        case F_BN: return (unsigned)(s.cout + 255) / 256;
        case F_WINO: return L.wino_u ? (unsigned)(s.cin / 4) * (s.cout / 64) : 0;
        case F_WINO4: return L.wino4_u ? (unsigned)(s.cin / 4) * (s.cout / 64) : 0;
        case F_DXW: return (unsigned)((conv_dxw_floats(idx) + 255) / 256);
    }
    return 0;
}

int check_debug(hpe_ctx* c, int idx, int which) {
    if (!c) return fail(HPE_ERR_INVALID, "null ctx");
    if (idx < 0 || idx >= HPE_NUM_CONV || which < 0 || which >= HPE_PACK_COUNT) return fail(HPE_ERR_INVALID, "hpe_debug_encoder_packing: idx or which out of range");
    if (c->dead) return fail(HPE_ERR_STATE, "hpe_finalize failed on this ctx: destroy it and create a new one");
    if (!c->finalized) return fail(HPE_ERR_STATE, "hpe_finalize() has not been called");
    if (!c->have_encoder) return fail(HPE_ERR_STATE, "encoder weights were not loaded before hpe_finalize");
    if (c->bf16) return fail(HPE_ERR_STATE, "hpe_debug_encoder_packing needs an fp32 context");
    return HPE_OK;
}

// the buffer of (idx, which) and its bytes; nullptr / 0: this context does not hold it
const void* packing_of(hpe_ctx* c, int idx, int which, size_t* bytes) {
    const ConvSpec& s = specs()[idx];
    const ConvLayer& L = c->conv[idx];
    const size_t wt = (size_t)L.n_pad * L.k_pad, dual = (size_t)round_up(s.cout, 128) * L.k_dual, u = (size_t)s.cin * s.cout;
    const void* p = nullptr;
    size_t n = 0;
    switch (which) {
        case HPE_PACK_W: p = L.w, n = wt * 4; break;
        case HPE_PACK_W_SPLIT: p = L.w_split, n = wt * 3 * 2; break;
        case HPE_PACK_WINO_U: p = L.wino_u, n = u * 16 * 4; break;
        case HPE_PACK_WINO4_U: p = L.wino4_u, n = u * 36 * 4; break;
        case HPE_PACK_STEM_W: p = L.stem_w, n = (size_t)3 * 64 * 224 * 2; break;
        case HPE_PACK_SCALE: p = L.scale, n = (size_t)s.cout * 4; break;
        case HPE_PACK_SHIFT: p = L.shift, n = (size_t)s.cout * 4; break;
        case HPE_PACK_W_DUAL: p = L.w_dual, n = dual * 4; break;
        case HPE_PACK_W_DUAL_SPLIT: p = L.w_dual_split, n = dual * 3 * 2; break;
        case HPE_PACK_SHIFT_DUAL: p = L.shift_dual, n = (size_t)s.cout * 4; break;
        case HPE_PACK_DXW: p = c->et.dxw[idx], n = conv_dxw_floats(idx) * 4; break;
        case HPE_PACK_FLAT:
            if (c->et.flat) p = c->et.flat + layout().off[idx][0];
            n = ((size_t)s.kh * s.kw * s.cin * s.cout + 3 * (size_t)s.cout) * 4;
            break;
    }
    *bytes = p ? n : 0;
    return *bytes ? p : nullptr;
}

}  // namespace

size_t encoder_repack_reserve_floats() { return (sizeof(RepackTable) + 3) / 4; }

int encoder_repack_reserve(hpe_ctx* c) {
    RepackTable t{};
    for (int i = 0; i < HPE_NUM_CONV; ++i) {
        const ConvSpec& s = specs()[i];
        const ConvLayer& L = c->conv[i];
        RepackLayer& r = t.L[i];
        r.w = L.w;
        r.scale = L.scale;
        r.shift = L.shift;
        r.wino_u = L.wino_u;
        r.wino_split = L.wino_u_split != nullptr;
        r.wino4_u = L.wino4_u;
        r.dxw = c->et.dxw[i];
        r.w_split = L.w_split ? static_cast<unsigned short*>(L.w_split) : L.w_stream;  // (w_stream: w_split itself, or the same image behind w)
        r.kh = s.kh;
        r.cin = s.cin;
        r.cout = s.cout;
        r.n_pad = L.n_pad;
        r.k_pad = L.k_pad;
        for (int w = 0; w < 4; ++w) r.off[w] = layout().off[i][w];
        r.stat = layout().stat[i];
        // what the kernels take for granted: square kernels, whole [64][4] blocks in the Winograd layouts, whole row tiles
        if (s.kh != s.kw || L.n_pad % TILE_N != 0 || ((L.wino_u || L.wino4_u) && (s.cin % 8 != 0 || s.cout % 64 != 0)))
            return fail(HPE_ERR_STATE, std::string("encoder repack: unexpected geometry of ") + s.name);
    }
    for (int f = 0; f < F_DUAL; ++f) {
        RepackForm& F = t.F[f];
        unsigned b = 0;
        for (int i = 0; i < HPE_NUM_CONV; ++i) {
            const unsigned nb = blocks_of(f, specs()[i], c->conv[i], i);
            if (!nb) continue;
            F.item[F.n] = i;
            F.block0[F.n++] = b;
            b += nb;
        }
        F.block0[F.n] = b;
    }
    {
        RepackForm& F = t.F[F_DUAL];
        unsigned b = 0;
        for (const ResBlock& blk : blocks()) {
            if (!blk.first || !c->conv[blk.i2c].w_dual) continue;
            const ConvLayer& L2 = c->conv[blk.i2c];
            RepackDual& d = t.D[F.n];
            d.w = L2.w_dual;
            d.shift = L2.shift_dual;
            d.split = L2.w_dual_split ? static_cast<unsigned short*>(L2.w_dual_split) : L2.w_dual_stream;  // (as RepackLayer::w_split)
            d.i2c = blk.i2c;
            d.i1 = blk.i1;
            d.K1 = L2.k1_dual;
            d.K2 = L2.k_dual - L2.k1_dual;
            d.N = specs()[blk.i2c].cout;
            d.n_pad = round_up(d.N, 128);
            F.item[F.n] = F.n;
            F.block0[F.n++] = b;
            b += (unsigned)(d.n_pad / TILE_N) * ((L2.k_dual + TILE_K - 1) / TILE_K);
        }
        F.block0[F.n] = b;
    }
    float* p = nullptr;
    int rc = dev_alloc(c, &p, encoder_repack_reserve_floats(), false);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(p, &t, sizeof(t), hipMemcpyHostToDevice));
    c->et.repack = p;
    // the grids, kept on the host side of the table
    static_assert(F_COUNT <= 8, "grid array");
    for (int f = 0; f < F_COUNT; ++f) c->et.repack_grid[f] = t.F[f].block0[t.F[f].n];
    return HPE_OK;
}

hipError_t encoder_repack_launch(hpe_ctx* c, const float* flat, hipStream_t st) {
    const EncTrainWork& w = c->et;
    const RepackTable* T = static_cast<const RepackTable*>(w.repack);
    const unsigned* grid = w.repack_grid;
    if (grid[F_WT]) hipLaunchKernelGGL(repack_wt_kernel, dim3(grid[F_WT]), dim3(256), 0, st, T, flat);
    if (grid[F_BN]) hipLaunchKernelGGL(repack_bn_kernel, dim3(grid[F_BN]), dim3(256), 0, st, T, flat, w.mean, w.sd);
    if (c->conv[0].stem_w)
        hipLaunchKernelGGL(repack_stem_kernel, grid1(64 * 224), dim3(256), 0, st, static_cast<unsigned short*>(c->conv[0].stem_w),
                           flat + layout().off[0][0]);
    if (grid[F_WINO]) hipLaunchKernelGGL(repack_wino_kernel<4>, dim3(grid[F_WINO]), dim3(256), 0, st, T, flat);
    if (grid[F_WINO4]) hipLaunchKernelGGL(repack_wino_kernel<6>, dim3(grid[F_WINO4]), dim3(256), 0, st, T, flat);
    if (grid[F_DXW]) hipLaunchKernelGGL(repack_dxw_kernel, dim3(grid[F_DXW]), dim3(256), 0, st, T, flat);
    if (grid[F_DUAL]) hipLaunchKernelGGL(repack_dual_kernel, dim3(grid[F_DUAL]), dim3(256), 0, st, T, flat, w.mean, w.sd);
    HIPE(hipGetLastError());
    return hipMemcpyAsync(w.flat, flat, (size_t)layout().total * sizeof(float), hipMemcpyDeviceToDevice, st);
}

hipError_t encoder_repack_stats_launch(hpe_ctx* c, hipStream_t st) {
    const EncTrainWork& w = c->et;
    const RepackTable* T = static_cast<const RepackTable*>(w.repack);
    const unsigned* grid = w.repack_grid;
    if (grid[F_BN]) hipLaunchKernelGGL(repack_bn_kernel, dim3(grid[F_BN]), dim3(256), 0, st, T, w.flat, w.mean, w.sd);
    if (grid[F_DUAL]) hipLaunchKernelGGL(repack_dual_kernel, dim3(grid[F_DUAL]), dim3(256), 0, st, T, w.flat, w.mean, w.sd);
    return hipGetLastError();
}

#pragma GCC visibility push(default)
extern "C" {

long long hpe_debug_encoder_packing_bytes(hpe_ctx* c, int idx, int which) {
    if (!c || idx < 0 || idx >= HPE_NUM_CONV || which < 0 || which >= HPE_PACK_COUNT) return 0;
    if (c->dead || !c->finalized || !c->have_encoder || c->bf16) return 0;
    size_t n;
    packing_of(c, idx, which, &n);
    return (long long)n;
}

int hpe_debug_encoder_packing(hpe_ctx* c, int idx, int which, void* dst, void* stream) {
    int rc = check_debug(c, idx, which);
    if (rc) return rc;
    if (!dst) return fail(HPE_ERR_INVALID, "null dst_dev");
    size_t n;
    const void* p = packing_of(c, idx, which, &n);
    if (!p) return fail(HPE_ERR_STATE, "hpe_debug_encoder_packing: this context does not hold that form of that layer");
    DeviceGuard g(c->cfg.device);
    HIP_TRY(hipMemcpyAsync(dst, p, n, hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
    return HPE_OK;
}

}  // extern "C"
#pragma GCC visibility pop
