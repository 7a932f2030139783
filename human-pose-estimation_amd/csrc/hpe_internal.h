// hpe_internal.h -- shared declarations of libhpe_hip.so (not part of the C ABI; see include/hpe.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "../../include/hpe.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));  // accumulator of v_mfma_f32_32x32x2_f32

// XCD-aware bijective remap of a workgroup id onto `total` logical ids: the workgroups of one XCD (bid, bid + 8, ...: they share an L2) walk
// consecutive logical ids, so that neighbouring tiles (the N tiles of one A row panel, ...) fetch their shared operand from HBM once
// (Id: int, or blockIdx.x's unsigned -- the type decides the shift the kernel was compiled with)
template <typename Id>
__device__ __forceinline__ int xcd_remap(Id bid, int total) {
    const int xcd = bid & 7;
    const int q = total >> 3, rr = total & 7;
    return (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + (bid >> 3);
}

inline dim3 grid1(long n) { return dim3((unsigned)((n + 255) / 256)); }  // one thread per element, 256 a block

// GEMM_DUAL: two A sources summed into one accumulator (K concatenated): k-slabs [0, k1_slabs) come from the dense matrix x
// (row pitch lda), the rest from the strided NHWC tensor x2 (geometry in Hi / Wi / Cin / Ho / Wo / stride) -- the last 1x1
// convolution of a ResNet conv_block and its projection shortcut as ONE launch (weights concatenated along k, BN scales folded in)
enum GemmMode { GEMM_DENSE = 0, GEMM_STRIDED = 1, GEMM_CONV3 = 2, GEMM_STEM = 3, GEMM_DUAL = 4 };
enum GemmTile { TILE_128x128 = 0, TILE_128x64 = 1, TILE_64x64 = 2, TILE_64x128 = 3, TILE_128x128_W8 = 4, TILE_128x64_W8 = 5, TILE_256x128_W8 = 6,
                TILE_P8_256x256 = 7 /* bf16 only: the phase-interleaved 8-wave kernel of conv_gemm_bf16_p8.hip */ };

// Arguments of the implicit-GEMM kernel (conv_gemm.hip).  All offsets are in floats.
struct GemmArgs {
    const float* x;      // A source: activations (NHWC) or a dense [M, lda] matrix
    const float* w;      // packed weights Wt[n][k], row pitch ldw, w_rows rows (zero padded)
    const float* scale;  // [N]
    const float* shift;  // [N]
    const float* res;    // optional residual [M, ldres]
    float* y;            // [M, ldy]
    int M, N, K;         // K is a multiple of 32 (weights are zero padded along k)
    int lda, ldw, ldy, ldres, w_rows;
    int relu;
    int Hi, Wi, Cin, Ho, Wo, stride, cin_slabs;
    int n_mtiles, n_ntiles;  // filled by the launcher
    int split_k;             // filled by the launcher (> 1: small grid cut along K, reduced by the fix-up kernel)
    float* partial;          // split-K workspace of the launching stream, partial_floats floats; nullptr disables splitting
    size_t partial_floats;
    const float* zero;       // >= 16 B of zeros in global memory (source of out-of-image taps for the LDS-DMA path)
    void* reserved;   // unused (was the diagnostics buffer of the removed register-staged kernel): keeps the kernel-argument offsets, and so the
                      // device code of every GEMM kernel, as they were
    const float* x2;  // GEMM_DUAL: second A source (strided NHWC)
    int k1_slabs;     // GEMM_DUAL: k-slabs taken from x
    int res_prefetch;  // filled by the launcher: 8-wave tiles read their residual rows before the main loop (0: in the epilogue)
    int y_slab8;  // 1: y is written channel-slab major, y[(n / 8) * M + m][n % 8] (the layout the fused Winograd kernel reads); needs N % 8 == 0
    int w_piece;  // hpe_launch_gemm_f32s: element offset of bf16 piece j = 1, 2 inside a weight row (piece j of Wt[n][k] at w + n * ldw + j * w_piece + k)
};

// splitk_min_slabs (>= 2): k-slabs per slice when a small grid is cut along K; split_k_out (host, optional) receives the split_k the
// launcher chose (1 = whole tiles, 0 = the contract rejected the arguments and nothing was launched)
hipError_t hpe_launch_gemm(GemmArgs p, int mode, int tile, int splitk_min_slabs, hipStream_t st, int* split_k_out = nullptr);
// conv_gemm_f32s.hip: the same fp32 GEMM (GEMM_DENSE / GEMM_STRIDED / GEMM_DUAL, whole tiles, no split-K) on the bf16 matrix cores: p.w points to
// bf16 weights split exactly into three pieces on the host (w = w0 + w1 + w2, offsets in bf16 elements, ldw and w_piece multiples of 8), A is
// split the same way in registers; the six products with i + j <= 2 are summed in fp32.  Tiles TILE_128x128 (4 waves), TILE_128x128_W8,
// TILE_256x128_W8
hipError_t hpe_launch_gemm_f32s(GemmArgs p, int mode, int tile, hipStream_t st);
// conv_stream_f32s.hip: the dense split-bf16 GEMM with a residual for K = 64 / 128 and N % 128 == 0 as persistent workgroups that hold their
// weights in registers and stream 32-row A tiles (p.w, p.ldw, p.w_piece as for hpe_launch_gemm_f32s; mode GEMM_DENSE: p.res is required).  max_walkers > 0
// caps the workgroups per 128-cout slice (the outputs do not depend on it)
// mode GEMM_DUAL: no residual, k = 0 .. 63 from x, 64 .. 127 from x2 [M][Cin = 64] (stride 1, Ho = Hi): the conv_block of stage 2
bool hpe_stream_f32s_supported(int M, int N, int K);
bool hpe_stream_f32s_dual_supported(int M, int N, int K1, int K2, int stride, int Hi, int Ho);
hipError_t hpe_launch_stream_f32s(GemmArgs p, int mode, int max_walkers, hipStream_t st);
int hpe_stream_device_cus();  // CUs of the device, asked once per process
// conv_stream_chain_f32s.hip: the expand 1x1 of a stage-2 block chained with the next block's reduce 1x1 in one persistent launch, both on the
// bf16 matrix cores (the weights are the layers' fp32 weights, split inside the kernel): t3 = relu(scaleA (wA . [t2 | x]) + shiftA) with
// C2 = 64 channels of x as the second A source (conv_block form, folded weights), or t3 = relu(scaleA (wA . t2) + shiftA + x) with x the
// residual [M][256] (C2 = 0); u1 = relu(scaleB (wB . t3) + shiftB), row-major or channel-slab major (u1_slab8).  M % 32 == 0, C = 64, C4 = 256,
// CP = 64; anything else is refused (hipErrorInvalidValue, nothing is launched).  max_walkers > 0 caps the grid (the outputs do not depend on it)
struct StreamChainArgs {
    const float *t2, *x, *wA, *wB, *scaleA, *shiftA, *scaleB, *shiftB;
    float *t3, *u1;
    int M, ldwA, ldwB, u1_slab8;
};
bool hpe_stream_chain_f32s_supported(int M, int C, int C4, int CP, int C2);
hipError_t hpe_launch_stream_chain_f32s(const StreamChainArgs& p, int C, int C4, int CP, int C2, int max_walkers, hipStream_t st);

// conv_wino.hip: 3x3/s1 SAME convolution as Winograd F(2x2,3x3); U = G g G^T blocked [N/64][C/8][16][2][64][4], V workspace of
// hpe_wino_v_floats(B, H, W, C) floats; C % 32 == 0, N % 64 == 0
size_t hpe_wino_v_floats(int B, int H, int W, int C);
hipError_t hpe_wino_init_device();  // per-device kernel attributes; call with the target device current
// optional persistent stream-K scheduling of the GEMM: n_wg workgroups (one per CU), ws = n_wg * HPE_WINO_WS_FLOATS floats and
// flags = n_wg zero-initialised words owned by the launching stream, epoch unique per launch (never 0)
#define HPE_WINO_WS_FLOATS 65536
struct WinoStreamK {
    float* ws;
    unsigned* flags;
    unsigned epoch;
    int n_wg;
    unsigned* err;  // device error word (bit 0 set when a wait timed out), may be nullptr
};
hipError_t hpe_launch_wino_conv3(const float* x, int lda, const float* U, const float* scale, const float* shift, float* y, int ldy,
                                 int B, int H, int W, int C, int N, int relu, float* V, const WinoStreamK* sk, hipStream_t st);

// fused-transform variant (56x56 / 28x28 maps): xs is channel-slab major [C/8][B*H*W][8] (GemmArgs::y_slab8 of the producer)
hipError_t hpe_launch_wino_fused_conv3(const float* xs, const unsigned short* Us, const float* scale, const float* shift, const float* zero16, float* y,
                                       int ldy, int B, int H, int W, int C, int N, int relu, hipStream_t st);
int hpe_wino_fused_items(int B, int H, int W, int N);  // work items of that launch, 0 if the geometry is not supported
hipError_t hpe_launch_nhwc_to_slab8(const float* x, float* xs, long M, int C, hipStream_t st);

// conv_wino4.hip: the same convolution as Winograd F(4x4,3x3); U = G g G^T blocked [N/64][C/4][36][64][4], V workspace of
// hpe_wino4_v_floats(B, H, W, C) floats (blocked [tiles/32][C/4][36][32][4]); C % 32 == 0, N % 64 == 0; co_running = batch chunks
// launching the same layer on other streams at the same time (picks between the 64- and the 32-cout GEMM: the 32-cout one below n32_below
// workgroups on the device); abl: ablation mask of diagnostics builds (-DHPE_ABLATION), 0 otherwise
size_t hpe_wino4_v_floats(int B, int H, int W, int C);
int hpe_wino4_items(int B, int H, int W, int N);  // workgroups of the GEMM launch
hipError_t hpe_wino4_init_device();
hipError_t hpe_launch_wino4_conv3(const float* x, int lda, const float* U, const float* scale, const float* shift, float* y, int ldy, int B,
                                  int H, int W, int C, int N, int relu, float* V, hipStream_t st, int co_running, float* split_ws, int n32_below, int abl);
// split_ws: hpe_wino4_split_ws_floats() floats whose LAST 256 (unsigned counters) are zero, owned by launches that are alone on the device
// (nullptr: the C axis is never cut)
size_t hpe_wino4_split_ws_floats();

// fused-transform F(4x4,3x3) (56x56 / 28x28 maps): xs is channel-slab major [C/8][B*H*W][8] (GemmArgs::y_slab8 of the producer)
hipError_t hpe_launch_wino4_fused_conv3(const float* xs, const float* U, const float* scale, const float* shift, const float* zero16, float* y,
                                        int ldy, int B, int H, int W, int C, int N, int relu, hipStream_t st);
int hpe_wino4_fused_items(int B, int H, int W, int N);  // workgroups of that launch, 0 if the geometry is not supported

// conv_gemm_bf16.hip (x / w / res / y of GemmArgs point to bf16 data; offsets are in bf16 elements; K % 64 == 0)
hipError_t hpe_launch_gemm_bf16(GemmArgs p, int mode, int tile, hipStream_t st);
// conv_gemm_bf16_p8.hip: 256 x 256 x 64 tile, 8 waves, phase-interleaved main loop, split-K through p.partial (DENSE / STRIDED / CONV3 / DUAL)
hipError_t hpe_launch_gemm_bf16_p8(GemmArgs p, int mode, hipStream_t st, int* split_k_out = nullptr);
// conv_chain_bf16.hip: t3 = relu(bn(W2c . t2) + res) and u1 = relu(bn'(W2a' . t3)) in one launch (the last 1x1 of identity block i and the
// first 1x1 of identity block i + 1); all tensors bf16, row-major [M, channels], weights packed [n][k]
struct ChainArgs {
    const __bf16* t2;   // [M, C]
    const __bf16* res;  // [M, 4C]  (identity block; nullptr in the conv_block form)
    const __bf16* x2;   // [M, C2]  conv_block form: the block input, second A source of the expand GEMM (nullptr otherwise)
    const __bf16* w2c;  // [4C][ldw2c]
    const __bf16* w2a;  // [C'][ldw2a]
    const float *scaleA, *shiftA;  // [4C]
    const float *scaleB, *shiftB;  // [C']
    __bf16* t3;  // [M, 4C]
    __bf16* u1;  // [M, C']
    int M, ldw2c, ldw2a;
};
// conv3_halo_bf16.hip: 3x3 / stride 1 / SAME, bf16, activation tile + halo resident in LDS (the 9 taps read one staged image)
struct Halo3Args {
    const __bf16* x;     // [M, Cin] NHWC, M = B * HW * HW
    const __bf16* w;     // packed [N][ldw], k = tap * Cin + c
    const float* scale;  // [N]
    const float* shift;  // [N]
    __bf16* y;           // [M, N]
    int M, N, ldw, relu;
    int n_ntiles;        // filled by the launcher
    int two;             // map sizes (bit mask: 1 = 7x7, 2 = 14x14, 4 = 28x28) on the two-workgroups-per-CU form (64 channels per workgroup, one image buffer)
};
bool hpe_halo3_bf16_supported(int HW, int Cin, int N);
hipError_t hpe_launch_halo3_bf16(const Halo3Args& p, int HW, int Cin, hipStream_t st);

bool hpe_chain_bf16_supported(int C, int C4, int CP, int C2);
hipError_t hpe_launch_chain_bf16(const ChainArgs& p, int C, int C4, int CP, int C2, hipStream_t st);
hipError_t hpe_chain_bf16_occupancy(int out[3]);
// conv_chain_f32.hip: the same chained launch in fp32 (identity blocks of stage 2, C = 64; opt-in).  u1_slab8: u1 is written channel-slab
// major, u1[(n / 8) * M + m][n % 8] (what the fused Winograd 3x3 kernel of the next block reads)
struct ChainArgsF32 {
    const float *t2, *res, *w2c, *w2a, *scaleA, *shiftA, *scaleB, *shiftB;
    float *t3, *u1;
    int M, ldw2c, ldw2a, u1_slab8;
};
bool hpe_chain_f32_supported(int C, int C4, int CP);
hipError_t hpe_launch_chain_f32(const ChainArgsF32& p, int C, int C4, int CP, hipStream_t st);
hipError_t hpe_chain_f32_occupancy(int* out);
hipError_t hpe_launch_f32_to_bf16(const float* x, void* y, long n, hipStream_t st);  // round to nearest even
hipError_t hpe_launch_bf16_to_f32(const void* x, float* y, long n, hipStream_t st);
hipError_t hpe_launch_pad_input_bf16(const float* img, void* out, int B, int H, int W, int Hp, int Wp, hipStream_t st);
hipError_t hpe_launch_maxpool_bf16(const void* x, void* y, int B, int H, int C, hipStream_t st);
hipError_t hpe_launch_avgpool_bf16(const void* x, float* y, int B, int HW, int C, int ldy, hipStream_t st);

// stem_fused.hip: conv1_pad + conv1 + bn_conv1 + ReLU + pool1_pad + max-pool in one kernel; img [B,224,224,3] fp32 ->
// y [B,56,56,64] (fp32, or bf16 when bf16 != 0).  w: bf16 [64][7][32] (k = kh * 32 + kw * 4 + c, other slots zero);
// for fp32 output the three exact bf16 pieces of the fp32 weights in that order, [3][64][7][32].  R pooled rows per workgroup, 56 % R == 0, R <= 8.
hipError_t hpe_launch_stem_fused(const float* img, const void* w, const float* scale, const float* shift, void* y, int B, int R, int bf16,
                                 hipStream_t st);
hipError_t hpe_stem_fused_init_device();
int hpe_stem_fused_pick_rows(int B);

// encoder_ops.hip
hipError_t hpe_launch_pad_input(const float* img, float* out, int B, int H, int W, int Hp, int Wp, hipStream_t st);
hipError_t hpe_launch_maxpool(const float* x, float* y, int B, int H, int C, hipStream_t st);
hipError_t hpe_launch_avgpool(const float* x, float* y, int B, int HW, int C, int ldy, hipStream_t st);
// Dense layer at M <= 4 rows (one launch, no split-K): wt packed [n][K], K % 4 == 0
hipError_t hpe_launch_dense_gemv(const float* x, int lda, int M, int K, const float* wt, int N, const float* scale, const float* shift, const float* res,
                                 int ldres, int relu, float* y, int ldy, hipStream_t st);
hipError_t hpe_launch_tile_theta(const float* mean85, float* theta, int B, int ld, hipStream_t st);
hipError_t hpe_launch_copy_theta(const float* src, int lds, float* dst, int ldd, int B, int n, hipStream_t st);

// smpl.hip
struct SmplDev {
    // constants (device)
    const float* v_template;  // [V*3]
    const float* shapedirs;   // [10][V*3]
    const float* posedirs;    // [207][V*3]
    const float* weights;     // [V][24]
    const float* kp_reg;      // [V][KP_PITCH] (zero padded columns)
    const float* j_reg;       // [V][KP_PITCH]
    const float* j_basis;     // [11][24][3]  J of (v_template, shapedirs[0..9]) -- from the regress kernel
    const int* parents;       // [24]
    const int* depth;         // [24]
    int num_kp;
    int max_depth;
};
#define SMPL_V 6890
#define SMPL_KP_PITCH 24
#define SMPL_IMG_TILE 8
#define SMPL_SMALL_B 8  // batches up to this size take the latency path of smpl.hip

struct SmplWork {
    float* pfT;   // [207][Bpad]  pose feature, transposed
    float* betaT; // [10][Bpad]
    float* A;     // [Bpad][24][12]
    float* cams;  // [Bpad][4] (s, tx, ty, 0)
    float* verts_tmp; // [Bpad][V][3] used when the caller does not want verts but wants joints
    float* kp_part;   // [SMPL_SMALL_B][108][72] keypoint-regressor partials of the small-batch path (nullptr: always the large-batch kernels)
    int Bpad;
};

struct HpeOutputs;
hipError_t hpe_launch_smpl(const SmplDev& d, const SmplWork& w, const float* theta, int ldtheta, int B, const HpeOutputs* o,
                           hipStream_t st);
hipError_t hpe_launch_joint_regress(const float* X, const float* reg, int n, int K, float* out, const float* cams,
                                    float* kp2d, hipStream_t st);
hipError_t hpe_launch_orth_proj(const float* X, const float* cam, int B, int P, float sx, float sy, int pixels, float* out,
                                hipStream_t st);

// smpl_bwd.hip: the gradient of hpe_launch_smpl with respect to theta.  Its workspace is its own (a backward call reads nothing a
// forward call left behind): the forward's per-image operands recomputed from theta, and the per-(vertex tile, image) partial sums
#define SMPL_BWD_PART 512  // floats per partial: dA 288 | d pose_feature 207 | d beta 10 | camera sums 3 | 4 unused
struct SmplBwdWork {
    float* pfT;    // [207][Bpad]
    float* betaT;  // [10][Bpad]
    float* A;      // [Bpad][24][12]
    float* cams;   // [Bpad][4]
    float* rjg;    // [Bpad][24][24]  R (9) | J (3) | G (12) per joint
    float* gj;     // [Bpad][24][5]   cotangent reaching joints (3) | g_kp2d (2) per keypoint
    float* part;   // hpe_smpl_bwd_part_floats(Bpad)
    int Bpad;
};
size_t hpe_smpl_bwd_part_floats(int Bpad);
// g: cotangents of the forward outputs (nullptr = zero); grad_theta [B][85] is written
hipError_t hpe_launch_smpl_backward(const SmplDev& d, const SmplBwdWork& w, const float* theta, int B, const HpeOutputs* g,
                                    float* grad_theta, hipStream_t st);

// critic.hip: CriticNetwork + get_kcs (src/models.py:97-202), forward and the gradient of the scores with respect to the inputs
#define CRITIC_ROWS 4  // rows per workgroup
struct CriticLayerSpec {
    const char* name;  // Keras layer name
    int in, out;       // kernel [in][out]
};
const CriticLayerSpec* hpe_critic_layers();  // HPE_NUM_CRITIC_DENSE entries, the order of hpe_critic_layer_name()
struct CriticW {  // device pointers into the ctx's one critic buffer
    const float* w[HPE_NUM_CRITIC_DENSE];   // kernel [in][out] (the Keras layout)
    const float* wt[HPE_NUM_CRITIC_DENSE];  // its transpose [out][in], read by the backward
    const float* b[HPE_NUM_CRITIC_DENSE];   // bias [out]
};
// the ctx's one critic buffer (per layer kernel | transposed kernel | bias, 16-byte aligned blocks, the padding zero): its size and the
// pointers into a buffer of that layout.  hpe_launch_critic_params(set) is the one writer of its contents.
size_t hpe_critic_live_floats();
CriticW hpe_critic_live_view(const float* buf);
// joints [N][K][3] (the first 14 are read), betas: 10 floats per row, betas_stride floats apart, Rs [N][24][3][3] (the root is skipped);
// scores [N][3], kcs [N][169] or nullptr.  One launch, no workspace.
hipError_t hpe_launch_critic(const CriticW& w, const float* joints, int K, const float* betas, int betas_stride, const float* Rs, long N,
                             float* scores, float* kcs, hipStream_t st);
// grad_scores [N][3] or nullptr (= ones); any output may be nullptr.  grad_joints [N][K][3] is the total derivative (the KCS path folded
// in), grad_kcs [N][169] the partial one with KCS held as an independent input.  One launch, stateless: the hidden layers are recomputed.
hipError_t hpe_launch_critic_backward(const CriticW& w, const float* joints, int K, const float* betas, int betas_stride, const float* Rs,
                                      long N, const float* grad_scores, float* grad_joints, float* grad_betas, float* grad_Rs,
                                      float* grad_kcs, hipStream_t st);

// critic_train.hip: d F / d (critic weights) for F = sum_n [ sum_c grad_scores[n,c] scores[n,c] + <t_n, d(sum_c scores[n,c]) / dx_n> ],
// as one flat buffer (kernel 0 [in][out], bias 0, kernel 1, ...), and the flat <-> live weights copies
#define CRITIC_PARAM_FLOATS 114273  // sum over the nine layers of in * out + out; these three are checked against the table in critic_common.h
#define CRITIC_WG_ROW_FLOATS 1664   // workspace floats per row: left operands of the nine layers 1043 | signals 618 | grad_scores 3
#define CRITIC_WG_CHUNK 64          // rows per partial sum
int hpe_critic_wg_chunks(long N);
size_t hpe_critic_wg_ws_floats(long N);  // N rows + one flat partial per chunk (none for a single chunk)
int hpe_critic_flat_offset(int idx, bool bias);  // idx == HPE_NUM_CRITIC_DENSE (bias false): the total
// grad_scores [N][3] or nullptr (no first-order term); tangents t_kcs [.][169], t_joints [.][42], t_betas [.][10], t_Rs [.][207] or
// nullptr, one row shared by all rows (tangent_per_row 0) or one per row; ws: hpe_critic_wg_ws_floats(N); grad_params is overwritten.
// Three launches (two when N <= CRITIC_WG_CHUNK); fixed summation order, no atomics.
hipError_t hpe_launch_critic_weight_grad(const CriticW& w, const float* joints, int K, const float* betas, int betas_stride, const float* Rs,
                                         long N, const float* grad_scores, const float* t_kcs, const float* t_joints, const float* t_betas,
                                         const float* t_Rs, int tangent_per_row, float* ws, float* grad_params, hipStream_t st);
// set: flat -> the ctx's kernels, their transposed copies and biases; else the live weights -> flat.  One launch.
hipError_t hpe_launch_critic_params(const CriticW& w, float* flat, bool set, hipStream_t st);

// losses.hip
hipError_t hpe_launch_kp_loss(const float* gt, const float* pred, int n, float* out, hipStream_t st);
// d loss / d pred [n][2] = grad_loss * vis * sign(pred - gt) / (2 * #visible); grad_loss: one device float or nullptr (= 1)
hipError_t hpe_launch_kp_loss_backward(const float* gt, const float* pred, int n, const float* grad_loss, float* grad_pred, hipStream_t st);
hipError_t hpe_losses_init_device();  // per-device kernel attributes of the loss kernels
size_t hpe_mesh_loss_ws_floats(int B, int H, int W, int P);
// a2b_mode: 0 cell-grid search (default), 1 VALU full search, 2 matrix-core full search; counter: optional 2 x u64 (MFMAs issued
// by the grid / full search)
hipError_t hpe_launch_mesh_loss(const float* seg, const float* v2d, int B, int H, int W, int P, float* ws, float* out,
                                hipStream_t st, int a2b_mode, unsigned long long* counter);
// the same in two halves: silhouette compaction + bitmap (once per step), then the searches of one vertex set (once per IEF stage)
hipError_t hpe_launch_mesh_loss_prepare(const float* seg, int B, int H, int W, int P, float* ws, hipStream_t st);
// (ev_a2b0 / ev_a2b1: optional events recorded around the pixel -> vertex search, the dominant kernel of the loss)
hipError_t hpe_launch_mesh_loss_search(const float* v2d, int B, int H, int W, int P, float* ws, float* out, hipStream_t st,
                                       hipEvent_t ev_a2b0, hipEvent_t ev_a2b1, int a2b_mode, unsigned long long* counter);

// the loss and d loss / d v2d [B][P][2] (for a cotangent of 1) from one pair of searches; nn_pix [B][H*W] / nn_vert [B][P] (optional)
// receive the neighbours used.  Same workspace (its tail holds the integer sign counters).
hipError_t hpe_launch_mesh_loss_grad(const float* seg, const float* v2d, int B, int H, int W, int P, float* ws, float* out, float* grad,
                                     int* nn_pix, int* nn_vert, hipStream_t st, int a2b_mode, unsigned long long* counter);

// prepost.hip
hipError_t hpe_launch_preprocess_u8(const unsigned char* img, int H, int W, int C, int newH, int newW, int start_x, int start_y,
                                    int margin, float* out, int S, hipStream_t st);
// batch of frames in one launch: frame b at img + (table ? table[b].offset : b * H * W * C); table == nullptr: all frames share the
// geometry in `uni`
struct PreprocFrame {
    long long offset;
    int H, W, newH, newW, start_x, start_y;
};
hipError_t hpe_launch_preprocess_u8_batch(const unsigned char* img, const PreprocFrame* table_dev, PreprocFrame uni, int B, int C, int margin,
                                          float* out, int S, hipStream_t st);
hipError_t hpe_launch_shift_verts(const float* verts, const float* cam, int B, int P, float flength, float img_size, float* out,
                                  hipStream_t st);

// render.hip: batched mesh rasteriser (SMPLRenderer, DESIGN.md "Renderer").  One record per (image, vertex):
struct RenderVert {
    int U, V;      // projected position in 1/256 px (rint(256 u), rint(256 v))
    int valid;     // 0: non-finite, outside [near, far] or outside the +-16384 px guard band (its faces are dropped)
    int pad;
    float iz;      // 1 / z
    float r, g, b; // lit vertex colour (albedo * sum of the three Lambertian point lights), not clamped
};
struct RenderArgs {
    const float* verts;        // [B,P,3] camera-space vertices
    const float* cam;          // [B,3] (f, px, py); nullptr: (500, W/2, H/2)
    const int* faces;          // [Fn,3]
    const int* adj_off;        // [P+1] vertex -> face CSR
    const int* adj_face;       // [3 Fn]
    RenderVert* rec;           // [B,P]
    uint2* box;                // [B,Fn]
    float* center;             // [B,4] (rotation only)
    const unsigned char* bg;   // [B,H,W,3] or nullptr (white)
    unsigned char* out;        // [B,H,W,C]
    int* out_face;             // test hook: [B,H,W] winning face (-1 uncovered) instead of the image
    float* out_z;              // test hook: [B,H,W] its depth
    int B, P, Fn, H, W, C;
    int rotate;
    float R[9];                // row-major, V' = (V - c) R + c
    float znear, zfar;
    float albedo[3];
    float light[9];            // three light positions (already rotated by Ry(120 deg))
    float light_color[3];
};
// stage 0: vertex records only; 1: the whole render (image, or face / depth buffers when out_face is set)
hipError_t hpe_launch_render(const RenderArgs& a, int stage, hipStream_t st);
