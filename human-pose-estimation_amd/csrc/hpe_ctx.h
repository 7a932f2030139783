// hpe_ctx.h -- the context behind the C ABI of include/hpe.h and what its translation units share: the layer table, the per-layer
// weights, error reporting, device selection and allocation helpers.  hpe_plan.hip resolves the plan and routes every conv launch,
// hpe_finalize.hip packs the weights and sizes the workspaces, hpe_encoder.hip holds the launch sequences, hpe_api.hip the extern "C" entry points.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/hpe.h"
#include "bf16_split.h"
#include "hpe_internal.h"
#include "hpe_plan.h"

// sets the thread-local message of hpe_last_error() and returns code
int fail(int code, const std::string& msg);

#define HIP_TRY(expr)                                                                                             \
    do {                                                                                                          \
        hipError_t _e = (expr);                                                                                   \
        if (_e != hipSuccess)                                                                                     \
            return fail(HPE_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e) + " (" __FILE__ ":" +      \
                                         std::to_string(__LINE__) + ")");                                         \
    } while (0)

struct ConvSpec {
    char name[24];
    char bn[24];
    int kh, kw, cin, cout, stride, hin, hout;
};

// ResNet-50 v1 layer table, Keras names / order [2a, 2b, 2c, (1)] per block.
const std::vector<ConvSpec>& specs();

// One bottleneck block of that table: the indices of its layers.  first: a conv_block (projection shortcut i1, else i1 = -1), last: the
// last block of its stage; in: the layer whose output is the block's input (the previous block's i2c), -1 = the max-pooled map
struct ResBlock {
    int stage;
    bool first, last;
    int i2a, i2b, i2c, i1;
    int in;
};
const std::vector<ResBlock>& blocks();  // 16 entries, built by the loop that builds specs()

inline int round_up(int x, int m) { return ((x + m - 1) / m) * m; }

struct ConvLayer {
    // Host staging (Keras layouts).  kernel is released by hpe_finalize.  bias / gamma / beta go STALE after hpe_encoder_set_params_dev:
    // after hpe_finalize nothing reads them but hpe_encoder_train_reserve (once, before any device update can run) and
    // hpe_encoder_set_params, which overwrites all of them first.  mean / var change only through hpe_encoder_set_stats_dev, on the device:
    // hpe_encoder_set_params copies the installed statistics back here before it folds.
    std::vector<float> kernel, bias, gamma, beta, mean, var;
    bool loaded = false;
    float* w = nullptr;  // device, packed [n_pad][k_pad] (fp32) or bf16 [n_pad][k_pad16] in bf16 mode
    float* scale = nullptr;
    float* shift = nullptr;
    // *_branch2c of a conv_block only: [scale2c * W2c | scale1 * W1] concatenated along k and the summed shifts -- the expand
    // convolution and the projection shortcut as one dual-source GEMM (GEMM_DUAL)
    float* w_dual = nullptr;
    float* shift_dual = nullptr;
    int k_dual = 0, k1_dual = 0;
    // plan option f32_split: the fp32 weights of the 1x1 layers split exactly into three bf16 pieces, [n_pad][3][k] (conv_gemm_f32s.hip)
    void* w_split = nullptr;
    void* w_dual_split = nullptr;
    // what conv_stream_f32s.hip reads, held by the layers stream1x1_layer() names: w_split where the layer has that packing, else the same
    // [n_pad][3][k] image derived behind w in w's allocation (w_stream_of) -- not a packing of its own; written by hpe_finalize and the repack kernel
    unsigned short* w_stream = nullptr;
    unsigned short* w_dual_stream = nullptr;  // the same for the dual-source launch: w_dual_split, or its image behind w_dual
    void* stem_w = nullptr;   // conv1 only: weights in the k enumeration of stem_fused.hip (bf16 [64][7][32]; fp32: its three bf16 pieces [3][64][7][32])
    float* wino_u = nullptr;  // device, G g G^T in the blocked layout of conv_wino.hip (3x3 layers on the Winograd path only)
    // derived from wino_u, not a packing of its own: its three bf16 pieces in the operand order of wino_fused_split_kernel (wino_us_base),
    // behind wino_u in the same allocation; held by the layers of the fused F(2x2,3x3) path (maps from wino_fused_min_hw on), written by
    // hpe_finalize and by the repack kernel
    unsigned short* wino_u_split = nullptr;
    float* wino4_u = nullptr;  // device, the F(4x4,3x3) G g G^T in the blocked layout of conv_wino4.hip (layers selected by wino_f4)
    int n_pad = 0, k_pad = 0;
};

// The k index of tap (kh, kw, ci) of layer idx in its packed weights Wt[n][k]: (kh, kw, cin) with cin fastest; conv1 has one 32-wide
// group per kernel row, 8 px x 4 ch (the 8th pixel and the 4th channel are zero weights)
inline int conv_wt_k(int idx, int kh, int kw, int ci) {
    const ConvSpec& s = specs()[idx];
    return idx == 0 ? kh * 32 + kw * 4 + ci : (kh * s.kw + kw) * s.cin + ci;
}

// ... and the length of that k axis: whole k-slabs of the GEMM kernels, 32 floats or 64 bf16 (the bf16 stem slab s holds kernel rows (2s, 2s + 1))
inline int conv_k_pad(int idx, bool bf16) { return round_up(idx == 0 ? 7 * 32 : specs()[idx].kh * specs()[idx].kw * specs()[idx].cin, bf16 ? 64 : 32); }

// The packing rules the host packers (hpe_finalize.hip, encoder_train.hip) and the repack kernels (encoder_repack.hip) share.  Every
// floating-point helper fixes its operation order and turns contraction off, so that both sides round alike.

// first element of (cout n, cin ci) in the F(2x2,3x3) weights [cout/64][cin/8][16][2][64][4]; element (xi, nu) is (xi * 4 + nu) * 512 further
__host__ __device__ inline size_t wino_u_base(int n, int ci, int cin) {
    return ((((size_t)(n >> 6) * (cin / 8) + (ci >> 3)) * 16) * 2 + ((ci >> 2) & 1)) * 256 + (size_t)(n & 63) * 4 + (ci & 3);
}
// ... in the split F(2x2,3x3) weights, bf16 [cout/64][cin/8][piece 3][16][64][8]: element (xi, nu) is (xi * 4 + nu) * 512 further, piece j is
// j * WINO_US_PIECE further
constexpr size_t WINO_US_PIECE = 16 * 64 * 8;
__host__ __device__ inline size_t wino_us_base(int n, int ci, int cin) {
    return ((size_t)(n >> 6) * (cin / 8) + (ci >> 3)) * 3 * WINO_US_PIECE + (size_t)(n & 63) * 8 + (ci & 7);
}
// the derived ConvLayer::w_stream: behind the n_pad * k_pad floats of w, in w's allocation
inline unsigned short* w_stream_of(float* w, int n_pad, int k_pad) { return reinterpret_cast<unsigned short*>(w + (size_t)n_pad * k_pad); }
// where that buffer lives: behind the 16 * cin * cout floats of wino_u, in wino_u's allocation (packer and repack kernel both ask here)
__host__ __device__ inline unsigned short* wino_u_split_of(float* wino_u, int cin, int cout) {
    return reinterpret_cast<unsigned short*>(wino_u + (size_t)16 * cin * cout);
}
// ... and in the F(4x4,3x3) weights [cout/64][cin/4][36][64][4]; element (xi, nu) is (xi * 6 + nu) * 256 further
__host__ __device__ inline size_t wino4_u_base(int n, int ci, int cin) {
    return (((size_t)(n >> 6) * (cin / 4) + (ci >> 2)) * 36) * 256 + (size_t)(n & 63) * 4 + (ci & 3);
}
// rows of G: F(2x2,3x3) [1 0 0; .5 .5 .5; .5 -.5 .5; 0 0 1], F(4x4,3x3) [1/4 0 0; -1/6 -1/6 -1/6; -1/6 1/6 -1/6; 1/24 1/12 1/6; 1/24 -1/12 1/6; 0 0 1]
__host__ __device__ inline double wino_g(int xi, int a) {
    constexpr double G[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
    return G[xi][a];
}
__host__ __device__ inline double wino4_g(int xi, int a) {
    constexpr double G4[6][3] = {{0.25, 0, 0}, {-1.0 / 6, -1.0 / 6, -1.0 / 6}, {-1.0 / 6, 1.0 / 6, -1.0 / 6},
                                 {1.0 / 24, 1.0 / 12, 1.0 / 6}, {1.0 / 24, -1.0 / 12, 1.0 / 6}, {0, 0, 1}};
    return G4[xi][a];
}
// element (xi, nu) of U = G g G^T from rows gx = G[xi], gn = G[nu]: in double, a and b ascending, one rounding to float
__host__ __device__ inline float wino_elem(const double gx[3], const double gn[3], const double g[3][3]) {
#pragma clang fp contract(off)
    double u = 0.0;
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) u += gx[a] * gn[b] * g[a][b];
    return (float)u;
}

// BatchNorm with the moving statistics folded into the layer: y = scale * conv(x, W) + shift, the conv bias inside shift.  In double;
// sd = sqrt((double)var + (double)eps), taken on the host (the statistics are fixed: hpe_encoder_train_reserve keeps sd on the device)
__host__ __device__ inline void bn_fold_sd(float gamma, float bias, float mean, float beta, double sd, double* scale, double* shift) {
#pragma clang fp contract(off)
    *scale = (double)gamma / sd;
    *shift = ((double)bias - (double)mean) * *scale + (double)beta;
}
inline double bn_sd(const ConvLayer& L, int n, float eps) { return std::sqrt((double)L.var[n] + (double)eps); }
inline void bn_fold(const ConvLayer& L, int n, float eps, double* scale, double* shift) {
    bn_fold_sd(L.gamma[n], L.bias[n], L.mean[n], L.beta[n], bn_sd(L, n, eps), scale, shift);
}
// ... and what the gamma gradient of the encoder's backward divides by
inline float bn_istd(const ConvLayer& L, int n, float eps) { return (float)(1.0 / std::sqrt((double)L.var[n] + (double)eps)); }

struct DenseLayer {
    std::vector<float> kernel, bias;
    bool loaded = false;
};

constexpr int STEM_HP = 230;  // 224 + 2*3
constexpr int STEM_WP = 232;  // 224 + 2*3 + 2 (8th tap column of the last window, zero weights)
constexpr int THETA_LD = 96;  // theta rows padded to 3 k-slabs of 32
// Winograd V workspace: image-major with this per-image pitch; a chunk of >= 32 images starting at image i0 owns
// [i0 * pitch, (i0 + n) * pitch): n * 802816 floats of transformed tiles (16 * tiles * C <= 802816 per image for every
// 3x3 layer) + up to 63 padding tiles * 16 * 512 = 516096 floats <= n * 16384
constexpr size_t WINO_V_PITCH = 802816 + 16384;
constexpr size_t WINO_V_SLACK = 524288;


// Regressor training (regressor_train.hip).  The backward multiplies by the transposed kernels, and for the dense GEMM's Wt[n][k] operand
// the transpose of a packed weight is the Keras [in][out] matrix itself: w1k / w2k / w3k hold it
// (regressor_params_copy writes them beside the packed copies, for hpe_finalize as for hpe_regressor_set_params_dev).  Everything else is workspace for max_batch rows and num_stage stages
// that no other entry point touches.
struct RegTrainWork {
    float *w1k = nullptr;  // [2048 + 128][1024]: dense_0/kernel, rows 2133.. zero (the theta block is an 85-row operand padded to two 64-row tiles)
    float *w2k = nullptr;  // [1024][1024]
    float *w3k = nullptr;  // [1024][THETA_LD]: dense_2/kernel, columns 85.. zero
    float *p1 = nullptr;   // [B][1024] features . W1[:2048]
    float *a1 = nullptr, *a2 = nullptr;    // [S][B][1024] hidden activations (after dropout)
    float *th = nullptr;   // [S + 1][B][THETA_LD]: tiled mean, then theta of every stage
    float *g = nullptr;    // [S + 1][B][THETA_LD]: cotangent reaching theta_{i-1} at index i (index 0: the tiled mean's)
    float *r = nullptr;    // [B][THETA_LD] residual operand of the theta GEMM
    float *da = nullptr;   // [B][1024] ungated data gradient
    float *dz1 = nullptr, *dz2 = nullptr;  // [S][B][1024]
    float *sum1 = nullptr; // [B][1024] sum over the stages of dz1
    float *zeros = nullptr;    // 2048 zeros (shift of the bias-free GEMMs)
    float *partial = nullptr;  // split-K workspace of its Dense launches
    size_t partial_floats = 0;
};

// Encoder training (encoder_train.hip), allocated by hpe_encoder_train_reserve for B images: nothing of it exists in an inference context.
// flat and dxw follow the live parameters: hpe_encoder_set_params uploads them from the host, hpe_encoder_set_params_dev rewrites them on
// the device with every packing of ConvLayer (encoder_repack.hip); mean / istd / sd are written by the reserve and rewritten by
// hpe_encoder_set_stats_dev; the repack table is written once, by the reserve
typedef unsigned short bf16e;  // a bf16 element as the host carries it: a pointer type of its own, so no fp32 launcher takes a bf16 buffer
typedef bf16e* mx16;
typedef const bf16e* cmx16;
// The activation and cotangent buffers of the training walks, once per element type (float: the fp32 walks, bf16e: the mixed ones)
template <class T>
struct EncActs {
    T *stash = nullptr;   // every layer's post-activation output, then the max-pooled map; layer-major, B images each
    T *zstash = nullptr;  // batch statistics only: every layer's raw output conv(x, W) + b, laid out as the stash (without the pooled map)
    T *g0 = nullptr, *g1 = nullptr;  // [B][802816] block cotangents (ping-pong)
    T *sbig = nullptr;    // [B][802816] dz * s of the wide layers (branch2c, branch1)
    T *t0 = nullptr, *t1 = nullptr, *ssmall = nullptr;  // [B][200704] bottleneck cotangents / low-resolution data gradients / dz * s
};
struct EncTrainWork {
    int B = 0;        // reserved batch (0: not reserved)
    int stash_B = 0;  // batch of the training forward that last filled the stash
    float *flat = nullptr;   // the live parameters in the flat layout (kernel HWIO | bias | gamma | beta per layer)
    float *mean = nullptr, *istd = nullptr;  // moving_mean and 1 / sqrt(moving_variance + eps) of every layer's channels, layer after layer
    double *sd = nullptr;    // sqrt((double)moving_variance + (double)eps) of the same channels: what bn_fold divides by (encoder_repack.hip)
    void *repack = nullptr;  // the device-side layer table of hpe_encoder_set_params_dev (encoder_repack.hip), built once by the reserve
    unsigned repack_grid[8] = {};  // workgroups of each of its launches (0: the context holds nothing of that form)
    EncActs<float> f32;  // hpe_encoder_train_reserve (zstash: hpe_encoder_train_reserve_batchnorm)
    EncActs<bf16e> b16;  // hpe_encoder_train_reserve_mixed (zstash: hpe_encoder_train_reserve_batchnorm_mixed)
    template <class T>
    EncActs<T>& acts() {
        if constexpr (std::is_same<T, float>::value) {
            return f32;
        } else {
            return b16;
        }
    }
    float *partial = nullptr;  // [slices][K][N] of the weight gradient in flight
    size_t partial_floats = 0;
    float *dsh = nullptr;    // [128][2048] column sums of dz per slice
    float *wgp = nullptr;    // <W, G> per 4-row chunk, [K / 4][N] of the layer in flight
    float *zeros = nullptr;  // 2048 zeros (shift of the data-gradient GEMMs)
    float *feat = nullptr;   // [B][2048] features of the backward's own forward
    float *dxw[HPE_NUM_CONV] = {};  // data-gradient operands Wt[cin][k], beside the forward's packings
    // BatchNorm with batch statistics (encoder_bn.hip), allocated by hpe_encoder_train_reserve_batchnorm only
    int bn_B = 0;       // its reserved batch (0: not reserved)
    int bn_stat_B = 0;  // batch of the batch-statistics forward that last filled a zstash and bn_batch (0: none has run)
    float *bn_batch = nullptr;  // [mu | var | r] of that forward, `channels` floats each, then 3 x 2048 floats for the one-layer debug calls
    float *bn_stats = nullptr;  // the installed moving statistics [mean of every channel | variance of every channel]
    double *bn_part = nullptr;  // [slices][2][N] partial column sums of the reduction in flight (2 * BN_PART_COLS doubles)
    int *bn_hw = nullptr;       // hout * hout of every channel's layer (the M of hpe_encoder_update_stats)
    // Data-parallel training (hpe_encoder_set_reduce): the hook that adds the ranks' column sums and the batch of all ranks together.
    // The sums it reduces ([2][N] doubles, then the reduced dbeta | dgamma as [2][N] floats) live at the front of wgp: the weight
    // gradient's scratch, which in stream order is idle from a layer's reduction to its elementwise launch
    hpe_reduce_fn reduce = nullptr;
    void *reduce_user = nullptr;
    int reduce_G = 0;
    int reduce_failed = -1;  // the layer at which the hook reported a failure during the walk in flight (-1: none)
    int bn_stat_G = 0;       // the batch the statistics in bn_batch were taken over: bn_stat_B, or reduce_G where the hook ran
    // Mixed precision (encoder_grad_bf16.hip), allocated by hpe_encoder_train_reserve_mixed only, beside b16.
    // partial / dsh / wgp / flat / mean / istd / feat / zeros above are shared with the fp32 walks
    int mx_B = 0;        // its reserved batch (0: not reserved)
    int mx_stash_B = 0;  // batch of the mixed forward that last filled b16.stash
    bf16e *mx_padded = nullptr;  // [B][STEM_HP][STEM_WP][4] the padded input, the 4th channel zero
    bf16e *mx_w[HPE_NUM_CONV] = {};    // RNE of ConvLayer::w, Wt[n_pad][conv_k_pad(idx, true)]; the k padding is zero from the reserve on
    bf16e *mx_dxw[HPE_NUM_CONV] = {};  // RNE of dxw
    void *mx_cast = nullptr;  // the device table of the cast launch that opens every mixed call: MX_CAST_SEGS segments
    // ... with batch statistics (encoder_bn_bf16.hip), allocated by hpe_encoder_train_reserve_batchnorm_mixed only
    int mxbn_B = 0;         // its reserved batch (0: not reserved)
    int mx_zstash_B = 0;    // batch of the mixed batch-statistics forward that last filled b16.zstash: RNE(conv(x16, W16) + b)
    bool bn_stat_mixed = false;  // the forward that last filled bn_batch was a mixed one: f32.zstash does not hold its raw outputs
};
constexpr int MX_CAST_SEGS = 2 * HPE_NUM_CONV - 1;  // segment idx: mx_w[idx]; segment HPE_NUM_CONV - 1 + idx (idx >= 1): mx_dxw[idx]
struct MxCastSeg {
    const float* src;     // rows of src_pitch floats
    bf16e* dst;           // rows of dst_pitch >= src_pitch bf16; columns past src_pitch are not written
    int src_pitch, dst_pitch;
    long quads;           // rows * src_pitch / 4
};
constexpr int BN_MAX_SLICES = 512;     // pixel slices of one BatchNorm reduction
constexpr int BN_PART_COLS = 262144;   // slices * channels of one reduction, at most
constexpr int WG_MAX_SLICES = 128;         // pixel slices of one weight gradient (what the fix-up adds per element)
constexpr int WG_WGP_FLOATS = 1152 * 512;  // <W, G> per 4-row chunk: K / 4 x N of the largest kernel (3x3, 512 -> 512)
static_assert(WG_WGP_FLOATS >= 3 * 2 * 2048, "the reduce buffers of data-parallel training fit the weight gradient's scratch");
// floats of layer idx's data-gradient operand: rows = input channels padded to 128, k = (flipped tap, output channel); conv1 has none
inline size_t conv_dxw_floats(int idx) {
    const ConvSpec& s = specs()[idx];
    return idx == 0 ? 0 : (size_t)round_up(s.cin, 128) * s.kh * s.kw * s.cout;
}
// Where each layer sits in the flat parameters, in the per-channel statistics arrays and in the stash (encoder_train.hip)
struct EncLayout {
    int off[HPE_NUM_CONV][4];    // kernel, bias, gamma, beta
    int stat[HPE_NUM_CONV];      // offset into the per-channel statistics arrays
    size_t stash[HPE_NUM_CONV];  // per-image offset of the layer's output in the stash
    size_t stash_pool, stash_per_image;
    int total, channels;
};
const EncLayout& layout();

struct hpe_ctx {
    HpeConfig cfg{};
    bool finalized = false;
    bool dead = false;  // hpe_finalize failed part-way: everything it had allocated was released, the ctx can only be destroyed
    HpePlan plan;       // every option that chooses a kernel or a launch shape: resolved once, in hpe_finalize (hpe_plan.h)
    bool bf16 = false;  // encoder_dtype == 1
    bool have_encoder = false, have_regressor = false, have_smpl = false;
    ConvLayer conv[HPE_NUM_CONV];
    DenseLayer dense[HPE_NUM_DENSE];
    // SMPL host staging
    bool smpl_loaded = false, mean_loaded = false;
    std::vector<float> h_vt, h_sd, h_pd, h_jreg, h_w, h_kreg;
    std::vector<int> h_par;
    int num_kp = 19;
    float h_mean[HPE_THETA_DIM];
    // device: regressor
    float *w1f = nullptr, *w1t = nullptr, *w2 = nullptr, *w3 = nullptr, *b1 = nullptr, *b2 = nullptr, *b3 = nullptr;
    float *ones = nullptr, *zeros = nullptr, *mean_dev = nullptr;
    EncTrainWork et{};  // encoder training (encoder_train.hip)
    RegTrainWork rt{};  // regressor training (regressor_train.hip): Keras-major weight copies and a workspace of its own
    // device: SMPL
    SmplDev smpl{};
    SmplWork work{};
    SmplBwdWork bwd{};  // hpe_smpl_backward
    float* smpl_basis_src = nullptr;  // [11][V*3]: v_template | shapedirs^T
    // device: activations
    float *padded = nullptr, *X0 = nullptr, *X1 = nullptr, *T1 = nullptr, *T2 = nullptr, *SC = nullptr;
    float *feat = nullptr, *P1 = nullptr, *H1 = nullptr, *H2 = nullptr, *thA = nullptr, *thB = nullptr;
    // device: critic (hpe_load_critic; valid before and after hpe_finalize, released with the rest of the device state)
    float* critic_buf = nullptr;  // hpe_critic_live_floats() floats: the live layout of critic.hip
    CriticW critic{};
    bool have_critic = false;
    float* critic_ws = nullptr;  // hpe_critic_weight_grad's workspace (hpe_critic_wg_ws_floats), grown outside capture
    size_t critic_ws_floats = 0;
    float* loss_ws = nullptr;
    size_t loss_ws_floats = 0;
    std::vector<void*> allocs;
    // batch-chunk streams
    float* partial = nullptr;  // split-K workspace (small grids only run unchunked on the caller's stream)
    size_t partial_floats = 0;
    float* wino_v = nullptr;  // Winograd input-transform workspace (nullptr: direct convolution everywhere)
    float* wino_ws = nullptr;       // stream-K parking space, one slot of n_cu workgroups per chunk stream (nullptr: plain grid)
    unsigned* wino_flags = nullptr;
    unsigned* dev_err = nullptr;  // device error word (bit 0: a stream-K wait timed out -> wrong output), see hpe_device_status
    unsigned wino_epoch = 0;
    int n_cu = 0;
    bool loss_attr_done = false;  // per-device kernel attributes of the loss kernels set (hpe_finalize, or the first loss call of a loss-only ctx)
    unsigned long long* loss_counter = nullptr;  // hpe_debug_set_loss_counter
    hipStream_t aux[3]{};
    hipEvent_t ev_fork{}, ev_join[3]{};
    // software pipeline across calls (hpe_forward_pipelined): the regressor + SMPL tail of batch k runs on `tail_st` while the
    // caller's stream already runs the encoder of batch k+1; features alternate between two buffers, the Dense layers of the tail
    // have their own split-K workspace
    hipStream_t tail_st{};
    hipEvent_t ev_enc{}, ev_tail{}, ev_feat_free[2]{};
    bool feat_free_valid[2] = {false, false};
    bool tail_pending = false;
    unsigned pipe_idx = 0;
    float* feat_alt = nullptr;
    int co_running = 1;    // chunk streams of the encoder call being enqueued (launch-size rules of the F(4x4) kernels)
    float* w4_split = nullptr;  // F(4x4) C-axis split workspaces + counters (4 x hpe_wino4_split_ws_floats: one per chunk-stream slot)
    float* partial_tail = nullptr;
    size_t partial_tail_floats = 0;
    bool dense_on_tail = false;  // set while a pipelined tail is being enqueued: run_dense then uses partial_tail
    // timing
    int timing = 0;
    hipEvent_t ev[8]{};
    // encoder span of every timed call since hpe_enable_timing (ring of the last SPAN_RING calls): hpe_get_span_stats
    static constexpr int SPAN_RING = 64;
    hipEvent_t span0[SPAN_RING]{}, span1[SPAN_RING]{};
    unsigned span_n = 0;
    hipEvent_t cev0[HPE_NUM_CONV]{}, cev1[HPE_NUM_CONV]{};
    hipEvent_t lev0[16]{}, lev1[16]{}, lev_all[2]{};  // hpe_val_losses: around each stage's pixel -> vertex search / the whole call
    int loss_timed_stages = 0;
    bool ev_ok = false, timed_valid = false, conv_timed_valid = false;
};

struct DeviceGuard {
    int prev = -1;
    bool changed = false;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) == hipSuccess && prev != dev) changed = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() {
        if (changed) (void)hipSetDevice(prev);
    }
};

int dev_alloc(hpe_ctx* c, float** p, size_t n_floats, bool zero);
int upload(hpe_ctx* c, float** p, const std::vector<float>& h);
// fp32 Wt[rows][K] -> bf16 [rows][3][K]: w = w0 + w1 + w2 exactly (finite weights), each piece rounded to nearest even (conv_gemm_f32s.hip)
int upload_split(hpe_ctx* c, void** p, const std::vector<float>& wt, int rows, int K);

#define HIPE(expr)                               \
    do {                                         \
        hipError_t _e = (expr);                  \
        if (_e != hipSuccess) return _e;         \
    } while (0)

enum { NEED_ENC = 1, NEED_REG = 2, NEED_SMPL = 4 };
int check_ready(hpe_ctx* c, int B, int need);

// hpe_finalize.hip
int finalize_impl(hpe_ctx* c);
void release_device_state(hpe_ctx* c);  // release everything a (possibly partial) hpe_finalize created
// pack the conv layers again from their host staging (kernel / bias / gamma / beta refilled by the caller) into the device buffers
// hpe_finalize allocated: no pointer changes.  Synchronous.
int repack_encoder(hpe_ctx* c);

// hpe_encoder.hip: launch what the route says.  wino_v: the launch's slice of the Winograd V workspace, slot: its chunk stream.
// scale / shift: the epilogue's per-channel vectors, nullptr = the layer's folded BatchNorm (the batch-statistics forward passes ones and
// the conv bias: every packing of the weights is unscaled)
hipError_t run_conv(hpe_ctx* c, int idx, const ConvRoute& r, const float* x, int B, const float* res, int relu, float* y, hipStream_t st,
                    float* wino_v = nullptr, int slot = 0, const float* scale = nullptr, const float* shift = nullptr);
// one layer on NHWC input, alone on the device, as hpe_debug_conv and the training forward launch it: asks the route and converts the
// input to channel-slab major (through T1) when the route reads that
hipError_t run_dual(hpe_ctx* c, int i2c, int i1, const ConvRoute& r, const float* t2, const float* x, int B, float* y, hipStream_t st);
hipError_t run_conv_nhwc(hpe_ctx* c, int idx, const float* x, int B, const float* res, int relu, float* y, hipStream_t st,
                         const float* scale = nullptr, const float* shift = nullptr);
hipError_t run_chain(hpe_ctx* c, int i2c, bool first, const float* t2, const float* res, int B, float* t3, float* u1, hipStream_t st,
                     bool u1_slab8 = false);
hipError_t run_stream_chain(hpe_ctx* c, int i2c, bool first, const float* t2, const float* x, int B, float* t3, float* u1, hipStream_t st,
                            bool u1_slab8, int rows = 0);
hipError_t encoder_impl(hpe_ctx* c, const float* images, int B, float* features, int ldfeat, hipStream_t st);
// partial == nullptr: the ctx's split-K workspace (the tail's own while a tail is being enqueued)
hipError_t run_dense(hpe_ctx* c, const float* x, int lda, int M, int K, const float* w, int w_rows, int N, const float* scale, const float* shift,
                     const float* res, int ldres, int relu, float* y, int ldy, hipStream_t st, float* partial = nullptr, size_t partial_floats = 0);
hipError_t regress_impl(hpe_ctx* c, const float* th_prev, float* th_next, int B, hipStream_t st);
hipError_t features_proj(hpe_ctx* c, const float* features, int B, hipStream_t st);
hipError_t tail_impl(hpe_ctx* c, const float* feat, int B, const HpeOutputs* stage_outs, int n_outs, hipStream_t ts, hipEvent_t feat_free);
hipError_t join_tail(hpe_ctx* c, hipStream_t st);  // wait on `st` for a pipelined call's tail, if one is pending
int forward_impl(hpe_ctx* c, const float* images, int B, const HpeOutputs* stage_outs, int n_outs, hipStream_t st, bool pipelined);

// encoder_repack.hip: the flat device parameters into every packing the ctx holds, in stream order
size_t encoder_repack_reserve_floats();            // what encoder_repack_reserve allocates beyond the statistics (the layer table)
int encoder_repack_reserve(hpe_ctx* c);            // builds the device-side layer table from the ctx's pointers; et.sd / et.mean / et.dxw exist
hipError_t encoder_repack_launch(hpe_ctx* c, const float* flat_dev, hipStream_t st);

// the two of them that fold the statistics (scale / shift, the dual-source weights), from the ctx's own flat copy: hpe_encoder_set_stats_dev
hipError_t encoder_repack_stats_launch(hpe_ctx* c, hipStream_t st);

// encoder_bn.hip / encoder_bn_bf16.hip: BatchNorm with batch statistics around a layer's raw output z [M][N] (N a multiple of 64, at most
// 2048), each launcher overloaded on the element type of the tensors z / y / res / dy / dz / dzraw.  The statistics, gamma, beta and the
// gradients are fp32 in both; the bf16 first stages write partials in the fp32 layout, so one set of finish launches runs behind both.
// part: 2 * BN_PART_COLS doubles.  mu / var / r / gamma / beta are 16-byte aligned; dgamma / dbeta / db need not be
struct BnGeom {
    int cg;    // channel groups (of vec channels, one 16-byte load) per workgroup: min(N / vec, 64)
    int rows;  // row lanes per workgroup: 256 / cg
    int gx;    // workgroups along N
    int P;     // pixels per slice
    int slices;
};
BnGeom bn_geom(int M, int N, int vec);          // vec: channels a thread, 4 (fp32) or 8 (bf16)
bool bn_bad_shape(long M, int N, int vec);      // a shape the launchers refuse: N is not whole workgroups of channel groups
int bn_slices(int M, int N);  // pixel slices of the fp32 reductions (-1: a shape they do not take)
hipError_t bn_launch_stats(const float* z, int M, int N, float eps, double* part, float* mu, float* var, float* r, hipStream_t st);
hipError_t bn_launch_stats(cmx16 z, int M, int N, float eps, double* part, float* mu, float* var, float* r, hipStream_t st);
hipError_t bn_launch_apply(const float* z, const float* mu, const float* r, const float* gamma, const float* beta, const float* res, int relu, float* y,
                           int M, int N, hipStream_t st);
hipError_t bn_launch_apply(cmx16 z, const float* mu, const float* r, const float* gamma, const float* beta, cmx16 res, int relu, mx16 y, int M, int N,
                           hipStream_t st);
hipError_t bn_launch_bwd_reduce(const float* dy, const float* y, const float* z, const float* mu, const float* r, int M, int N, double* part, float* db,
                                float* dgamma, float* dbeta, hipStream_t st);
hipError_t bn_launch_bwd_reduce(cmx16 dy, cmx16 y, cmx16 z, const float* mu, const float* r, int M, int N, double* part, float* db, float* dgamma,
                                float* dbeta, hipStream_t st);
// M_all > 0: the rows the statistics were taken over (all ranks'), where that is more than the M rows held here
hipError_t bn_launch_bwd_apply(const float* dy, const float* y, const float* z, const float* mu, const float* r, const float* gamma, const float* dgamma,
                               const float* dbeta, int M, int N, float* dz, float* dzraw, hipStream_t st, double M_all = 0.0);
hipError_t bn_launch_bwd_apply(cmx16 dy, cmx16 y, cmx16 z, const float* mu, const float* r, const float* gamma, const float* dgamma, const float* dbeta,
                               int M, int N, mx16 dz, mx16 dzraw, hipStream_t st, double M_all = 0.0);
// The two reductions cut where the ranks of data-parallel training meet: the local column sums into sums [2][N] doubles (which the caller
// adds over the ranks, in place), then the finish from the sums.  The backward's first half also writes the LOCAL db (= 0), dgamma and
// dbeta; its second half rounds the summed (dbeta | dgamma) into red [2][N] floats for bn_launch_bwd_apply
hipError_t bn_launch_stats_sums(const float* z, int M, int N, double* part, double* sums, hipStream_t st);
hipError_t bn_launch_stats_sums(cmx16 z, int M, int N, double* part, double* sums, hipStream_t st);
hipError_t bn_launch_stats_from_sums(const double* sums, double M_all, int N, float eps, float* mu, float* var, float* r, hipStream_t st);
hipError_t bn_launch_bwd_sums(const float* dy, const float* y, const float* z, const float* mu, const float* r, int M, int N, double* part, double* sums,
                              float* db, float* dgamma, float* dbeta, hipStream_t st);
hipError_t bn_launch_bwd_sums(cmx16 dy, cmx16 y, cmx16 z, const float* mu, const float* r, int M, int N, double* part, double* sums, float* db,
                              float* dgamma, float* dbeta, hipStream_t st);
hipError_t bn_launch_bwd_from_sums(const double* sums, int N, float* red, hipStream_t st);
// the second launch of each reduction alone, from partials part[slice][2][N] in that layout
hipError_t bn_finish_stats(const double* part, int slices, int M, int N, float eps, float* mu, float* var, float* r, hipStream_t st);
hipError_t bn_finish_sums(const double* part, int slices, int N, double* sums, hipStream_t st);
hipError_t bn_finish_bwd(const double* part, int slices, int N, float* db, float* dgamma, float* dbeta, hipStream_t st);
hipError_t bn_finish_bwd_sums(const double* part, int slices, int N, double* sums, float* db, float* dgamma, float* dbeta, hipStream_t st);
hipError_t bn_launch_momentum(float* stats, const float* batch, const int* hw, int B, int channels, double momentum, int unbiased, hipStream_t st);
hipError_t bn_launch_install(const float* stats, int channels, float eps, float* keep, float* mean, float* istd, double* sd, hipStream_t st);

// encoder_grad.hip / encoder_grad_bf16.hip: the launches of the encoder's backward, overloaded on the element type of the activations and
// cotangents (bf16e: the mixed-precision walks -- bf16 products with fp32 accumulation, fp32 gradients of the fp32 master weights)
// pixels per slice (whole groups of `group` pixels: 8 for the fp32 kernel, 16 for the bf16 one) and the slice count of layer idx's weight
// gradient at batch B; the floats of its partial buffer for every batch up to B
void wg_slicing(int idx, int B, int group, int* P, int* slices);
size_t wg_partial_floats(int B);
hipError_t wg_finish(hpe_ctx* c, int idx, int n_kc, int slices, float* grad_layer, hipStream_t st);  // the finish launch both precisions share
hipError_t mx_cast_launch(hpe_ctx* c, int first, int segs, hipStream_t st);  // segments [first, first + segs) of the cast table
// y = RNE(act(s * conv(x, W16) + shift (+ res))) through the bf16 route of the layer; idx 0 reads the padded bf16 input
// scale / shift: in place of the layer's folded BatchNorm (the batch-statistics walk: a unit scale and the bias)
hipError_t mx_conv_forward(hpe_ctx* c, int idx, cmx16 x, int B, cmx16 res, int relu, mx16 y, hipStream_t st, const float* scale = nullptr,
                           const float* shift = nullptr);
// layer idx's convolution, alone on the device, at the precision of its tensors
inline hipError_t layer_conv(hpe_ctx* c, int idx, const float* x, int B, const float* res, int relu, float* y, hipStream_t st,
                             const float* scale = nullptr, const float* shift = nullptr) {
    return run_conv_nhwc(c, idx, x, B, res, relu, y, st, scale, shift);
}
inline hipError_t layer_conv(hpe_ctx* c, int idx, cmx16 x, int B, cmx16 res, int relu, mx16 y, hipStream_t st, const float* scale = nullptr,
                             const float* shift = nullptr) {
    return mx_conv_forward(c, idx, x, B, res, relu, y, st, scale, shift);
}
// dz = dy * [y > 0] (y == nullptr: no activation), dzs = dz * s (bf16: rounded to nearest even).  dz / dzs may be nullptr; dz may alias
// dy.  n elements, N channels
void gate(const float* dy, const float* y, const float* s, float* dz, float* dzs, long n, int N, hipStream_t st);
void gate(cmx16 dy, cmx16 y, const float* s, mx16 dz, mx16 dzs, long n, int N, hipStream_t st);
// the weight gradient of layer idx and what hangs on it, into the fp32 grad_layer = [kernel | bias | gamma | beta]: three launches.  x: the
// layer's input; for idx 0 the images (fp32) or the padded bf16 input.  bn (batch statistics): dz is dzraw, dW = G with a unit scale, and
// the finish is not launched -- bias, gamma and beta come from bn_launch_bwd_reduce
hipError_t weight_grad(hpe_ctx* c, int idx, const float* x, const float* dz, int B, float* grad_layer, hipStream_t st, bool bn = false);
hipError_t weight_grad(hpe_ctx* c, int idx, cmx16 x, cmx16 dz, int B, float* grad_layer, hipStream_t st, bool bn = false);
// out [M][cin] = dzs [M][cout] . W^T (+ res) on the map of the layer's OUTPUT (a stride-2 layer: the low-resolution map)
hipError_t data_grad(hpe_ctx* c, int idx, const float* dzs, int B, const float* res, float* out, hipStream_t st);
hipError_t data_grad(hpe_ctx* c, int idx, cmx16 dzs, int B, cmx16 res, mx16 out, hipStream_t st);
void scatter2(const float* lo, float* hi, int B, int H, int C, hipStream_t st);  // lo [B][H][H][C] -> the even pixels of hi [B][2H][2H][C]
void scatter2(cmx16 lo, mx16 hi, int B, int H, int C, hipStream_t st);
void avgpool_bwd(const float* dy, float* dx, int B, int HW, int C, hipStream_t st);
void avgpool_bwd(const float* dy, mx16 dx, int B, int HW, int C, hipStream_t st);  // dx = RNE(dy / HW)
void maxpool_bwd(const float* x, const float* dy, float* dx, int B, int H, int C, hipStream_t st);  // x [B][H][H][C], the pool's input
void maxpool_bwd(cmx16 x, cmx16 dy, mx16 dx, int B, int H, int C, hipStream_t st);

// the three glue launches of the training forward at the precision of their tensors (encoder_ops.hip, conv_gemm_bf16.hip)
inline hipError_t enc_pad_input(const float* img, float* out, int B, int H, int W, int Hp, int Wp, hipStream_t st) {
    return hpe_launch_pad_input(img, out, B, H, W, Hp, Wp, st);
}
inline hipError_t enc_pad_input(const float* img, mx16 out, int B, int H, int W, int Hp, int Wp, hipStream_t st) {
    return hpe_launch_pad_input_bf16(img, out, B, H, W, Hp, Wp, st);
}
inline hipError_t enc_maxpool(const float* x, float* y, int B, int H, int C, hipStream_t st) { return hpe_launch_maxpool(x, y, B, H, C, st); }
inline hipError_t enc_maxpool(cmx16 x, mx16 y, int B, int H, int C, hipStream_t st) { return hpe_launch_maxpool_bf16(x, y, B, H, C, st); }
inline hipError_t enc_avgpool(const float* x, float* y, int B, int HW, int C, int ldy, hipStream_t st) {
    return hpe_launch_avgpool(x, y, B, HW, C, ldy, st);
}
inline hipError_t enc_avgpool(cmx16 x, float* y, int B, int HW, int C, int ldy, hipStream_t st) {
    return hpe_launch_avgpool_bf16(x, y, B, HW, C, ldy, st);
}

// regressor_train.hip
int regressor_param_offset(int idx, bool bias);  // idx 3: mean theta; idx 4 (bias false): the total
hipError_t regressor_train_forward(hpe_ctx* c, const float* features, int B, const float* drop, hipStream_t st);  // fills rt.a1 / a2 / th
hipError_t regressor_train_backward(hpe_ctx* c, const float* features, int B, const float* drop, const float* grad_thetas, float* grad_flat,
                                    float* grad_features, hipStream_t st);
hipError_t regressor_params_copy(hpe_ctx* c, float* flat, bool set, hipStream_t st);
