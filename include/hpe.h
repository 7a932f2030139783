/*
 * hpe.h -- C ABI of libhpe_hip.so: the MI355X (gfx950) implementation of the per-image forward hot
 * path of maxpit/human-pose-estimation (ResNet-50 v1 encoder -> 3-stage iterative SMPL-parameter
 * regressor -> SMPL linear blend skinning -> orthographic reprojection).
 *
 * The reference has NO plugin / operator / FFI interface: the Python class
 * `Predictor` (reference: src/predictor.py:26-163) *is* the interface.  This header is therefore the
 * boundary a maintainer's ctypes binding would call from `Predictor.__init__` / `Predictor.predict`;
 * every entry point cites the reference code it replaces.  INTEGRATION.md shows that binding.
 *
 * Conventions
 *   - plain C: pointers + sizes, int return codes (HPE_OK == 0), no exceptions cross the ABI,
 *     `hpe_last_error()` returns a thread-local message for the last failing call.
 *   - "host" pointers are read during the call and not retained; "dev" pointers are HIP device
 *     pointers owned by the caller (e.g. torch tensors' data_ptr()).  All tensors are dense float32.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).  No call synchronises the
 *     device except hpe_create / hpe_load_* / hpe_finalize / hpe_destroy / hpe_get_timings / hpe_device_status,
 *     and hpe_mesh_loss / hpe_mesh_loss_grad / hpe_val_losses ONCE when they meet a problem larger than the loss workspace
 *     hpe_finalize sized (max_batch images of 224 x 224, 6890 vertices): that call synchronises, frees the
 *     old workspace and allocates the larger one (such a call cannot be captured into a hipGraph).
 *   - a hpe_finalize that fails on the device (e.g. out of memory) releases everything it had allocated
 *     and leaves the ctx dead: every later call returns HPE_ERR_STATE, only hpe_destroy is valid.
 *   - one ctx per device; a ctx is not re-entrant (the reference is not either: SMPL.J_transformed is
 *     mutated per call, src/tf_smpl/batch_smpl.py:135).
 *   - theta layout (kept from the reference, src/predictor.py:136-138):
 *         [ s, tx, ty | 72 axis-angle (root first) | 10 betas ]  = 85 floats.
 */
#ifndef HPE_H_
#define HPE_H_

#ifdef __cplusplus
extern "C" {
#endif

#define HPE_OK 0
#define HPE_ERR_INVALID 1   /* bad argument / shape */
#define HPE_ERR_HIP 2       /* a HIP runtime call failed */
#define HPE_ERR_STATE 3     /* call order violated (e.g. forward before finalize) */
#define HPE_ERR_NO_DEVICE 4 /* no gfx950 device visible */
#define HPE_ERR_REDUCE 5    /* the reduce hook of hpe_encoder_set_reduce reported a failure */

#define HPE_NUM_CONV 53      /* ResNet-50 v1 conv layers, order of hpe_conv_layer_name() */
#define HPE_NUM_DENSE 3      /* RegressionNetwork: 2133->1024->1024->85 */
#define HPE_NUM_CRITIC_DENSE 9 /* CriticNetwork (src/models.py:158-202), order of hpe_critic_layer_name() */
#define HPE_NUM_VERTS 6890
#define HPE_NUM_JOINTS 24
#define HPE_NUM_BETAS 10
#define HPE_NUM_POSE_BASIS 207
#define HPE_THETA_DIM 85
#define HPE_FEATURE_DIM 2048
#define HPE_MAX_KP 24
#define HPE_IMG_SIZE 224

typedef struct hpe_ctx hpe_ctx;

typedef struct HpeConfig {
    int struct_size; /* sizeof(HpeConfig) of the header the caller was built with; written by hpe_config_init, checked by hpe_create
                      * (HPE_ERR_INVALID on a mismatch: the struct has grown every round, a short or zero-initialised one is refused) */
    int device;     /* HIP device ordinal */
    int max_batch;  /* workspace is sized for this many images per call (<= 1024) */
    int num_stage;  /* IEF iterations; reference default 3 (src/config.py:39) */
    float bn_eps;   /* BatchNorm epsilon: 1e-3 (keras_applications 1.0.8) or 1.001e-5 (tf.keras >= 2.2) */
    int encoder_dtype; /* 0 = fp32 MFMA (default), 1 = bf16 MFMA with fp32 accumulate (config 4) */
    /* Plan options that change WHICH kernels run (and therefore the rounding of the result, never its meaning).  -1 = the
     * default: the environment variable named on the right if it is set, else the built-in value.  Fill the struct with
     * hpe_config_init() first; two contexts with different options can live in one process.  Every option, the environment-only
     * ones of INTEGRATION.md section 4 included, is resolved once per context in hpe_finalize (a context used for the loss operators
     * only: at its first loss call); the environment is not read after that. */
    int n_streams;         /* HPE_STREAMS          concurrent batch-chunk streams of the encoder, 1..4 (2) */
    int dual_gemm;         /* HPE_DUAL             conv_block expand + projection shortcut as one dual-source GEMM (1) */
    int stem_fused;        /* HPE_STEM_FUSED       conv1 + BN + ReLU + max-pool as one kernel (1); 0 = pad / im2col GEMM / pool */
    int wino_min_c;        /* HPE_WINO_MINC        3x3 layers with >= this many channels run as Winograd (128); 0 = direct conv everywhere */
    int wino_min_items;    /* HPE_WINO_MIN_ITEMS   ... when the launch has >= this many work items (128) */
    int wino_fused;        /* HPE_WINO_FUSED       input transform fused into the Winograd GEMM on the large maps (1) */
    int wino_fused_min_hw; /* HPE_WINO_FUSED_MINHW smallest map side on the fused path (28) */
    int mesh_a2b;          /* HPE_MESH_A2B         pixel -> vertex search of the mesh loss: 0 cell grid (default), 1 VALU full
                            *                      search, 2 matrix-core full search */
    int wino_f4;           /* HPE_WINO_F4          map sizes whose 3x3 layers run as Winograd F(4x4,3x3) instead of F(2x2,3x3) / direct: bit mask
                            *                      1 = 7x7, 2 = 14x14, 4 = 28x28, 8 = 56x56 maps (7) */
    int wino4_fused;       /* HPE_WINO4_FUSED      map sizes (4 = 28x28, 8 = 56x56) whose F(4x4) layers transform their input inside the GEMM kernel
                            *                      (no V round trip; takes precedence over wino_f4 for those maps) */
    int bf16_p8;           /* HPE_BF16_P8          bf16 layer kinds on the 256 x 256 phase-interleaved GEMM kernel (N % 256 == 0, K >= 512 only):
                            *                      1 the 3x3 layers of stage 4, 2 those of stage 5, 4 1x1 / strided layers, 8 the dual-source
                            *                      launch of res5a, 16 the other dual-source launches.  A 3x3 layer whose map size is in halo3
                            *                      runs on the halo-resident kernel whatever bits 1-2 say: clear halo3 to use them */
    int wino4_ksplit;      /* HPE_WINO4_KSPLIT     small F(4x4) launches cut their channel axis into 2-4 parts that are added in part order
                            *                      (1); 0 = never (one summation order per output whatever the batch) */
    int chain_fuse;        /* HPE_CHAIN            bf16 encoder: stages (1 = stage 2, 2 = stage 3) whose identity blocks run res*_branch2c + add +
                            *                      ReLU and the NEXT block's res*_branch2a + ReLU as one launch: the 4C-wide block output is
                            *                      written once and not read back; 4 = the same for res2a (branch2c + branch1 + add + ReLU, the
                            *                      dual-source GEMM, + res2b_branch2a) (7); same bf16 rounding points as the separate launches.
                            *                      fp32 encoder: 8 = res2b_branch2c + add + ReLU and res2c_branch2a + ReLU as one launch
                            *                      (conv_chain_f32.hip) (8); 16 = bf16 stage 4 too (one 128-pixel workgroup per CU; a
                            *                      measured tie, off); 0 = one launch per layer */
    int halo3;             /* HPE_HALO3            bf16 encoder: map sizes whose 3x3 layers run on the halo-resident kernel (conv3_halo_bf16.hip:
                            *                      the activation tile + halo staged in LDS once per 64 input channels, the 9 taps read it at 9
                            *                      row shifts) instead of the implicit GEMM: bit mask as wino_f4 (1 = 7x7 ... 8 = 56x56) (15); same
                            *                      operands and rounding points, fp32 summation order differs.  Takes precedence over bf16_p8
                            *                      bits 1-2 on the 3x3 layers of the selected maps */
    int f32_split;         /* HPE_F32_SPLIT        fp32 encoder: stages (1 = stage 2, 2 = stage 3, 4 = stage 4, 8 = stage 5) whose 1x1 / strided /
                            *                      dual-source layers run on the bf16 matrix cores with both operands split exactly into three bf16
                            *                      pieces (conv_gemm_f32s.hip: fp32-exact products, fp32 accumulation; whole-tile launches only, small
                            *                      grids keep the fp32 kernel) (14); 0 = the fp32 MFMA everywhere */
} HpeConfig;

/* defaults: struct_size = sizeof(HpeConfig), device 0, max_batch 8, num_stage 3, bn_eps 1e-3, fp32, every plan option -1.
 * ALWAYS start from this call: hpe_create refuses a struct whose struct_size is not the library's. */
void hpe_config_init(HpeConfig* cfg);

/* SMPL constants as the reference holds them after SMPL.__init__ (src/tf_smpl/batch_smpl.py:31-81),
 * as dense host arrays in the pickle's own layouts. */
typedef struct HpeSmplModel {
    const float* v_template;   /* [6890,3] */
    const float* shapedirs;    /* [6890,3,10] */
    const float* posedirs;     /* [6890,3,207] */
    const float* J_regressor;  /* [24,6890]  (the sparse matrix, densified) */
    const float* weights;      /* [6890,24] */
    const float* kp_regressor; /* [num_kp,6890]  cocoplus_regressor (or its first 14 rows for 'lsp') */
    const int* parents;        /* [24] kintree_table[0] as int32, parents[0] == -1, parents[i] < i */
    int num_kp;                /* 19 (cocoplus, the reference default) or 14 (lsp) */
} HpeSmplModel;

/* Device output pointers of one IEF stage.  Any pointer may be NULL (that output is not written). */
typedef struct HpeOutputs {
    float* verts;          /* [B,6890,3]    generated_verts   (src/predictor.py:155) */
    float* joints;         /* [B,num_kp,3]  generated_joints  (src/predictor.py:154) */
    float* cams;           /* [B,3]         generated_cams    (src/predictor.py:156) */
    float* theta;          /* [B,85] */
    float* J_transformed;  /* [B,24,3]      smpl.J_transformed (src/tf_smpl/batch_smpl.py:135) */
    float* kp2d;           /* [B,num_kp,2]  batch_orth_proj_idrot(joints, cams) (src/trainer.py:274) */
    float* verts2d;        /* [B,6890,2]    reproject_vertices(verts, cams, [224,224]) (src/trainer.py:285) */
    float* Rs;             /* [B,24,3,3]    rotation matrices (third return of SMPL.__call__) */
} HpeOutputs;

const char* hpe_last_error(void);
const char* hpe_version(void);

/* Keras layer name of conv `idx` ("conv1", "res2a_branch2a", ... ) and of its BatchNorm. */
const char* hpe_conv_layer_name(int idx);
const char* hpe_bn_layer_name(int idx);
/* geometry of conv `idx`: out[0..6] = KH, KW, Cin, Cout, stride, Hin, Hout */
int hpe_conv_layer_geometry(int idx, int out[7]);

/* -- lifetime: replaces Predictor.__init__ (src/predictor.py:27-86) minus renderer/optimizers/critic -- */
int hpe_create(const HpeConfig* cfg, hpe_ctx** out);
int hpe_destroy(hpe_ctx* ctx);

/* SMPL(pkl_path) constants (src/predictor.py:55 -> src/tf_smpl/batch_smpl.py:26-86). */
int hpe_load_smpl(hpe_ctx* ctx, const HpeSmplModel* host_model);
/* One Keras Conv2D + its BatchNorm, Keras layouts: kernel HWIO [KH,KW,Cin,Cout], bias/gamma/beta/
 * moving_mean/moving_variance [Cout] (EncoderNetwork weights, src/models.py:35-41; restored from the
 * checkpoint's `feature_extractor`, src/predictor.py:79-86). */
int hpe_load_conv(hpe_ctx* ctx, int idx, const float* kernel_hwio, const float* bias, const float* gamma,
                  const float* beta, const float* moving_mean, const float* moving_variance);
/* One Keras Dense of RegressionNetwork: kernel [in,out], bias [out] (src/models.py:60-74). */
int hpe_load_dense(hpe_ctx* ctx, int idx, const float* kernel_in_out, const float* bias);
/* mean theta [85] (load_mean_param, src/predictor.py:88-110 / checkpoint's `inital_theta`). */
int hpe_load_mean_theta(hpe_ctx* ctx, const float* mean85);
/* Pack weights for the kernels, fold BN into per-channel scale/shift, precompute the joint-regressor
 * basis on the device.  Must be called after all hpe_load_* and before any compute call. */
int hpe_finalize(hpe_ctx* ctx);

/* -- the hot path: replaces the body of Predictor.predict (src/predictor.py:114-158) --------------
 * images_dev [B,224,224,3] NHWC float32 in [-1,1].  stage_outs[i] (i < n_outs) receives IEF stage
 * (num_stage - n_outs + i): n_outs == 1 gives the reference's `predict` result (last stage only, SMPL
 * of the earlier stages -- dead work in the reference -- is skipped); n_outs == num_stage gives what
 * Trainer.val_step consumes (src/trainer.py:242-298). */
int hpe_forward(hpe_ctx* ctx, const float* images_dev, int B, const HpeOutputs* stage_outs, int n_outs, void* stream);

/* The same forward, software-pipelined ACROSS calls for steady-state serving: the encoder of this batch is enqueued on `stream`,
 * its regressor + SMPL tail (a chain of small, latency-bound launches) on the ctx's own tail stream behind an event, so that the
 * NEXT call's encoder overlaps it.  The outputs of a call are complete only after hpe_join(ctx, s) has made stream `s` wait for
 * the tail (or after work enqueued on hpe_tail_stream(ctx) itself, e.g. hpe_val_losses or a collective on the outputs).
 * Successive tails are ordered among themselves; the caller must not reuse an output buffer before joining the call that
 * wrote it.  Per-batch latency is that of hpe_forward; throughput gains the tail time (fp32 3 %, bf16 encoder 10 %). */
int hpe_forward_pipelined(hpe_ctx* ctx, const float* images_dev, int B, const HpeOutputs* stage_outs, int n_outs, void* stream);
int hpe_join(hpe_ctx* ctx, void* stream);
/* The regressor + SMPL half of hpe_forward alone: features_dev [B,2048] (what hpe_encoder wrote) -> stage_outs as in hpe_forward
 * (src/predictor.py:126-148).  With hpe_encoder it lets a caller software-pipeline batches inside ONE stream-ordered step that a
 * hipGraph can capture -- fork; hpe_tail(features of batch k) on a side stream || hpe_encoder(images of batch k+1); join --
 * where hpe_forward_pipelined keeps its tail stream outside the caller's ordering and cannot be captured.  Uses the tail's own
 * split-K workspace, so it may run concurrently with hpe_encoder of the same ctx (and with nothing else of it). */
int hpe_tail(hpe_ctx* ctx, const float* features_dev, int B, const HpeOutputs* stage_outs, int n_outs, void* stream);
/* the ctx's tail stream (hipStream_t) for enqueuing consumers of a pipelined call's outputs without stalling `stream` */
void* hpe_tail_stream(hpe_ctx* ctx);

/* -- operators of the path, individually (same kernels as hpe_forward) -------------------------- */
/* image_feature_extractor.predict(images) (src/predictor.py:125): -> features_dev [B,2048] */
int hpe_encoder(hpe_ctx* ctx, const float* images_dev, int B, float* features_dev, void* stream);
/* one IEF step: theta_out = theta_prev + generator3d([features | theta_prev]) (src/predictor.py:129-133).
 * theta_prev_dev == NULL means tile(mean_var) (src/predictor.py:126). */
int hpe_regress_stage(hpe_ctx* ctx, const float* features_dev, const float* theta_prev_dev, int B, float* theta_out_dev,
                      void* stream);
/* self.smpl(shapes, poses, get_skin=True) + proj_fn on theta rows [B,85] (src/predictor.py:136-141). */
int hpe_smpl(hpe_ctx* ctx, const float* theta_dev, int B, const HpeOutputs* outs, void* stream);
/* gradient of hpe_smpl: grad_outs holds the cotangent of each forward output (NULL = zero); grad_theta_dev [B,85] is written.
 * It is what Trainer.train_step backpropagates through SMPL.__call__ and batch_orth_proj_idrot (src/trainer.py:383-505): the exact
 * derivative of hpe_smpl's arithmetic with respect to [ s, tx, ty | 72 axis-angle | 10 betas ]; the cams / theta cotangents pass
 * through.  Stateless (theta in, everything else recomputed into a workspace of its own, sized by hpe_finalize: no preceding hpe_smpl
 * is needed), no synchronisation, no allocation, capturable; fixed summation order: the same inputs give the same bits. */
int hpe_smpl_backward(hpe_ctx* ctx, const float* theta_dev, int B, const HpeOutputs* grad_outs, float* grad_theta_dev, void* stream);
/* batch_orth_proj_idrot (src/tf_smpl/projection.py:23-33): X [B,P,3], cam [B,3] -> out [B,P,2] */
int hpe_orth_proj(const float* X_dev, const float* cam_dev, int B, int P, float* out_dev, void* stream);
/* reproject_vertices (src/tf_smpl/projection.py:45-56): out = (proj + 1) * 0.5 * im_size */
int hpe_reproject_vertices(const float* verts_dev, const float* cam_dev, int B, int P, float im_w, float im_h, float* out_dev,
                           void* stream);
/* kp_reprojection_loss (src/ops.py:35-47): kp_gt [B,K,3], kp_pred [B,K,2] -> out_dev[0] = sum(vis*|d|),
 * out_dev[1] = 2*#visible (the SUM_BY_NONZERO_WEIGHTS denominator), out_dev[2] = loss (0 if nothing visible).
 * Numerator and count are returned separately so that ranks can all-reduce them before dividing. */
int hpe_kp_loss(const float* kp_gt_dev, const float* kp_pred_dev, int B, int K, float* out_dev, void* stream);
/* gradient of hpe_kp_loss w.r.t. kp_pred: grad_loss_dev is one device float (NULL = 1); grad_kp_pred_dev [B,K,2] =
 * grad_loss * vis * sign(pred - gt) / (2 * #visible), zero where pred == gt and everywhere when nothing is visible.  A NaN
 * difference gives a NaN gradient, as it gives a NaN loss: a bad record shows in the gradient, where hpe_grad_stats counts it. */
int hpe_kp_loss_backward(const float* kp_gt_dev, const float* kp_pred_dev, int B, int K, const float* grad_loss_dev,
                         float* grad_kp_pred_dev, void* stream);
/* mesh_reprojection_loss (src/ops.py:117-137) forward: seg_dev [B,H,W] (>0 = silhouette), verts2d_dev
 * [B,P,2] pixels -> out_dev[0] = sum_i bidirectional_dist_i / (3 + P).  workspace from the ctx.
 * Nearest neighbours (find_nearest_neighbors, src/ops.py:60-71) are exact: the argmin of the expanded squared distance
 * -2 a.b + |a|^2 + |b|^2 evaluated in fp32, ties to the lowest index as tf.argmin; any H, W, P (the pixel -> vertex search
 * prunes by a cell grid over the vertices when they fit its LDS image, else -- and for meshes concentrated in a few cells --
 * it evaluates every pair; the two give the same neighbours). */
int hpe_mesh_loss(hpe_ctx* ctx, const float* seg_dev, const float* verts2d_dev, int B, int H, int W, int P, float* out_dev,
                  void* stream);
/* mesh_reprojection_loss and its gradient with respect to verts2d in one call (one pair of searches serves both).
 * out_dev[0] = the loss as hpe_mesh_loss; grad_verts2d_dev [B,P,2] = dL/dverts2d (for an upstream cotangent of 1);
 * nn_pix_dev [B,H,W] int32 and nn_vert_dev [B,P] int32 receive the neighbours used (either may be NULL).
 * The nearest neighbours are argmins and carry no gradient (tf.gather on tf.argmin), so with A the silhouette pixels and B the vertices
 *   (3 + P) dL/dB_v = (B_v - A_nn(v)) / |B_v - A_nn(v)|_2  -  sum over the pixels a whose nearest vertex is v of sign(A_a - B_v)
 * (componentwise sign, sign(0) = 0).  nn_pix[b][y][x] = the nearest vertex of a silhouette pixel, -1 off the silhouette;
 * nn_vert[b][v] = y * W + x of vertex v's nearest silhouette pixel, -1 when the silhouette is empty.
 * Deliberate deviations from TensorFlow's gradient: a vertex lying exactly on its nearest pixel gets 0 from the first term
 * (tf.norm's gradient is NaN there), as hpe_kp_loss_backward defines sign(0) = 0; an image with an empty silhouette contributes
 * nothing to the loss and gets an all-zero gradient.
 * The second term is accumulated as integers, so the gradient does not depend on execution order: the same inputs give the same bits.
 * Same rules as hpe_mesh_loss: any H, W, P, a ctx that was never finalized will do, the searches follow the ctx's plan (mesh_a2b),
 * arguments are checked before any launch, the workspace is the loss workspace (which grows -- and synchronises -- only for a
 * geometry larger than the one hpe_finalize sized); no allocation or synchronisation otherwise, capturable.
 * grad_verts2d_dev == NULL is refused (HPE_ERR_INVALID): hpe_mesh_loss is the loss-only call. */
int hpe_mesh_loss_grad(hpe_ctx* ctx, const float* seg_dev, const float* verts2d_dev, int B, int H, int W, int P,
                       float* out_dev, float* grad_verts2d_dev, int* nn_pix_dev, int* nn_vert_dev, void* stream);

/* -- the critic: CriticNetwork + get_kcs (src/models.py:97-202), the learned prior of the generator loss (src/trainer.py:300-313) ------
 * Nine fp32 Dense layers, Keras layer names and kernel shapes [in, out]:
 *   0 kcs_dense 169x100 (leaky ReLU 0.2)   1 joints_dense 42x100 (leaky)      2 combined_dense 200x1 on [kcs_dense | joints_dense]
 *   3 shapes_dense_1 10x10 (ReLU)          4 shapes_dense_2 10x5 (ReLU)       5 shapes_dense_3 5x1
 *   6 rotation_dense_1 207x300 (leaky)     7 rotation_dense_2 300x100 (leaky) 8 rotation_dense_3 100x1
 * scores = [combined_dense, shapes_dense_3, rotation_dense_3] per row.  KCS = B^T B [13,13] with B = J^T C [3,13], J the first 14
 * joints and C the bone matrix of precompute_C_matrix (src/models.py:97-112); the reference's N x 13 x 13 x N tensordot + diag_part
 * (src/models.py:123-139) is this Gram matrix per row.  The rotation input is Rs[1:], the joints input J, both flattened row-major. */
/* Keras layer name of critic Dense `idx`; its kernel shape out[0..1] = in, out */
const char* hpe_critic_layer_name(int idx);
int hpe_critic_layer_shape(int idx, int out[2]);
/* Keras layouts, host pointers: kernel[i] [in,out], bias[i] [out] (the checkpoint's `discriminator`, src/trainer.py:193-198) */
typedef struct HpeCriticModel {
    const float* kernel[HPE_NUM_CRITIC_DENSE];
    const float* bias[HPE_NUM_CRITIC_DENSE];
} HpeCriticModel;
/* self.critic_network = CriticNetwork() + its restore (src/trainer.py:120,193-198).  Valid before or after hpe_finalize (the critic needs
 * nothing of the encoder, like the loss operators); synchronises; the ctx owns a device copy, released by hpe_destroy and by a failed
 * hpe_finalize; loading again replaces the weights. */
int hpe_load_critic(hpe_ctx* ctx, const HpeCriticModel* host_model);
/* critic_network([get_kcs(joints), joints[:, :14], shapes, Rs[:, 1:]]) (src/trainer.py:300-308): joints_dev [N,K,3] with
 * 14 <= K <= HPE_MAX_KP (the first 14 joints are read), betas_dev 10 floats per row, betas_stride (>= 10) floats apart (theta + 75 with
 * stride 85 works in place), Rs_dev [N,24,3,3] as HpeOutputs.Rs (the root is skipped) -> scores_dev [N,3]; kcs_dev [N,13,13] or NULL.
 * Any N >= 1.  One launch; no allocation, no synchronisation, capturable; arguments are checked before the launch.  Fixed summation
 * order: the same inputs give the same bits, and a row's result depends neither on N nor on the row's position.
 * HPE_ERR_STATE without a loaded critic, HPE_ERR_INVALID for a NULL ctx or a bad shape. */
int hpe_critic(hpe_ctx* ctx, const float* joints_dev, int K, const float* betas_dev, int betas_stride, const float* Rs_dev, int N,
               float* scores_dev, float* kcs_dev, void* stream);
/* Gradient of hpe_critic's scores with respect to its inputs -- what the generator loss backpropagates (src/trainer.py:383-505) and what
 * the gradient penalty differentiates (tf.gradients(out_interpolated, [kcs, joints, shapes, Rs]), src/trainer.py:566-570).
 * grad_scores_dev [N,3] or NULL (all ones).  Outputs, any of which may be NULL (all four NULL: HPE_ERR_INVALID): grad_joints_dev [N,K,3]
 * (joints 14..K-1 get zeros), grad_betas_dev [N,10] dense, grad_Rs_dev [N,24,3,3] (the root gets zeros), grad_kcs_dev [N,13,13].
 * grad_kcs is the partial derivative with KCS held as an independent input; grad_joints is always the total one, the KCS path folded in:
 * dL/dB = B (G + G^T), dL/dJ = (dL/dB C^T)^T with G = dL/dKCS.  Stateless (the hidden layers are recomputed); launch rules, summation
 * order and error codes as hpe_critic. */
int hpe_critic_backward(hpe_ctx* ctx, const float* joints_dev, int K, const float* betas_dev, int betas_stride, const float* Rs_dev, int N,
                        const float* grad_scores_dev, float* grad_joints_dev, float* grad_betas_dev, float* grad_Rs_dev,
                        float* grad_kcs_dev, void* stream);

/* -- critic training: gradients with respect to the critic's weights (the critic update, src/trainer.py:511-583) -------------
 * All nine layers' parameters as ONE flat fp32 buffer of hpe_critic_param_floats() floats: kernel 0 [in,out], bias 0, kernel 1, ...
 * in hpe_critic_layer_name order.  hpe_critic_param_offset(idx, is_bias): the first float of layer idx's kernel (is_bias 0) or bias;
 * -1 for a bad index. */
int hpe_critic_param_floats(void);
int hpe_critic_param_offset(int idx, int is_bias);
/* Weight gradient of
 *     F = sum_n [ sum_c grad_scores[n,c] * scores[n,c] + < t_n , d(sum_c scores[n,c]) / dx_n > ]
 * where x = [kcs, joints[:, :14], shapes, Rs[:, 1:]] and d(...)/dx is exactly hpe_critic_backward's output for grad_scores = ones
 * (grad_kcs the partial, grad_joints the total derivative): the list tf.gradients(out_interpolated, [kcs, joints, shapes, Rs])
 * penalises (src/trainer.py:566-572, src/ops.py:153-172).  The first term serves critic_tape.gradient of the WGAN term
 * (src/trainer.py:546,578), the second the gradient penalty: with the tangent t = d penalty / d (mean gradient) / N shared by all
 * rows it is the penalty's weight gradient in the reference's form (the norm of the batch mean); one tangent per row gives the
 * per-row form of the WGAN-GP paper.  The critic is piecewise linear, so no second derivative of an activation is involved, and the
 * tangent term contributes exactly zero to every bias.
 * Inputs as hpe_critic.  grad_scores_dev [N,3] or NULL (no first-order term).  Tangents, each may be NULL (zero): tangent_kcs_dev
 * [.,13,13], tangent_joints_dev [.,14,3] (14 joints whatever K), tangent_betas_dev [.,10] dense, tangent_Rs_dev [.,23,3,3] (without the
 * root).  tangent_per_row 0: each tangent is ONE row shared by all N rows; otherwise each has N rows.  grad_scores and all four
 * tangents NULL: HPE_ERR_INVALID.  grad_params_dev [hpe_critic_param_floats()] is overwritten.
 * Stateless (the hidden layers are recomputed).  Three launches; no synchronisation, capturable, and no allocation while the ctx's
 * workspace holds hpe_critic_weight_grad_ws_floats(N) floats: a call that needs more grows it after a device synchronisation (not
 * inside a capture; hpe_critic_reserve(ctx, N) does that ahead of time).  No floating-point atomics; rows are summed in a fixed order
 * (chunks of 64 rows in row order, chunks in chunk order): the same inputs give the same bits.  The result is a sum over rows, so
 * unlike hpe_critic's it depends on N and on the order of the rows.  Error codes as hpe_critic. */
long long hpe_critic_weight_grad_ws_floats(int N);
int hpe_critic_reserve(hpe_ctx* ctx, int N);
int hpe_critic_weight_grad(hpe_ctx* ctx, const float* joints_dev, int K, const float* betas_dev, int betas_stride, const float* Rs_dev,
                           int N, const float* grad_scores_dev, const float* tangent_kcs_dev, const float* tangent_joints_dev,
                           const float* tangent_betas_dev, const float* tangent_Rs_dev, int tangent_per_row, float* grad_params_dev,
                           void* stream);
/* The live weights <-> the flat layout, on the device (critic_optimizer.apply_gradients, src/trainer.py:582-583, then lives in the
 * caller's one flat tensor).  hpe_critic_set_params_dev also rebuilds the transposed copies hpe_critic_backward reads; one launch each,
 * no host round trip, no synchronisation, capturable: calls on `stream` see the new weights in stream order (calls on other streams
 * must be ordered by the caller).  HPE_ERR_STATE without a loaded critic: hpe_load_critic comes first, once. */
int hpe_critic_get_params(hpe_ctx* ctx, float* flat_dev, void* stream);
int hpe_critic_set_params_dev(hpe_ctx* ctx, const float* flat_dev, void* stream);

/* -- regressor training: the generator update's missing leg (src/trainer.py:383-505) -------------------------------------------
 * The RegressionNetwork (three Dense layers, src/models.py:60-74) and mean theta as ONE flat fp32 buffer of
 * hpe_regressor_param_floats() = 3,322,026 floats: dense_0/kernel [2133,1024], dense_0/bias, dense_1/kernel [1024,1024], dense_1/bias,
 * dense_2/kernel [1024,85], dense_2/bias, then the 85 floats of mean theta.  hpe_regressor_param_offset(idx, is_bias): the first float
 * of layer idx's kernel (is_bias 0) or bias; idx 3, is_bias 0: mean theta; -1 otherwise.  Host code: no device is needed. */
int hpe_regressor_param_floats(void);
int hpe_regressor_param_offset(int idx, int is_bias);
/* The live regressor <-> the flat layout, on the device.  hpe_regressor_set_params_dev rewrites every buffer hpe_finalize packed from
 * hpe_load_dense / hpe_load_mean_theta (the transposed kernels with their padding, biases, mean theta) and the [in][out] copies the
 * backward reads: afterwards hpe_tail / hpe_regress_stage give the bits of a ctx that loaded the same values.  Four launches (get: one),
 * no host round trip, no synchronisation, capturable; calls on `stream` see the new weights in stream order, calls on other streams
 * (a pipelined tail, too) must be ordered by the caller.  HPE_ERR_STATE before hpe_finalize or without a loaded regressor. */
int hpe_regressor_get_params(hpe_ctx* ctx, float* flat_dev, void* stream);
int hpe_regressor_set_params_dev(hpe_ctx* ctx, const float* flat_dev, void* stream);
/* The IEF loop of the generator step: for i = 0 .. num_stage - 1, x = [features | theta_{i-1}] (theta_{-1} = the tiled mean),
 * a1 = drop1 * relu(x W1 + b1), a2 = drop2 * relu(a1 W2 + b2), theta_i = theta_{i-1} + a2 W3 + b3; thetas_dev [num_stage][B][85].
 * drop_dev: float [2][B][1024] multipliers (>= 0; Keras dropout at rate 0.5: 0 or 2) applied at the LAST stage only, as the reference
 * passes training=True there only (src/trainer.py:395-398); NULL: no dropout, and then every theta row has the bits hpe_regress_stage /
 * hpe_tail compute (the same launches).  1 <= B <= max_batch.  The masks are an input: nothing here draws random numbers. */
int hpe_regressor_forward_train(hpe_ctx* ctx, const float* features_dev, int B, const float* drop_dev, float* thetas_dev, void* stream);
/* Gradient of  sum_i < grad_thetas[i], theta_i >  of that loop with respect to the flat parameters (grad_flat_dev
 * [hpe_regressor_param_floats()], overwritten) and, if grad_features_dev is not NULL, to the features ([B,2048], overwritten).  The
 * cotangent of stage i reaches every earlier stage through theta_{i-1}; every stage adds to the same six tensors and to mean theta.
 * grad_thetas_dev [num_stage][B][85]; NULL = all zero (a stage without a loss term is passed as zeros).  drop_dev as in the forward:
 * pass the same masks.  ReLU's gradient is taken as 0 at 0 (TensorFlow's).
 * Stateless: the forward is recomputed into a workspace of the ctx's own (sized by hpe_finalize for max_batch), so no forward call has
 * to precede it.  About 30 launches on `stream`; no allocation, no synchronisation, capturable; no atomics and a fixed summation order:
 * the same inputs give the same bits.  The result is a sum over rows, so it depends on B and on the order of the rows.
 * Concurrency: the two training calls share that one workspace, so they must not overlap each other or hpe_regressor_set_params_dev
 * on the same ctx; they read the weights only and share no buffer (no split-K slices either) with hpe_encoder, hpe_forward*, hpe_tail,
 * hpe_regress_stage, hpe_smpl* or the loss and critic calls, so they may run next to any of those on another stream.
 * HPE_ERR_INVALID for B outside [1, max_batch] or NULL features / grad_flat; HPE_ERR_STATE before hpe_finalize. */
int hpe_regressor_backward(hpe_ctx* ctx, const float* features_dev, int B, const float* drop_dev, const float* grad_thetas_dev,
                           float* grad_flat_dev, float* grad_features_dev, void* stream);

/* -- encoder training: fine-tuning ResNet-50 with the BatchNorm statistics held fixed ---------------------------------------------
 * (src/trainer.py:481 steps image_feature_extractor.trainable_variables with the regressor; here moving_mean / moving_variance stay as
 * loaded, Keras' frozen-BN mode.)  fp32 contexts only: every call that takes a ctx returns HPE_ERR_STATE on a bf16 context.
 * Per layer of the table (hpe_conv_layer_name), s = gamma / sqrt(var + eps):  y = act(s * (conv(x, W) + b - mean) + beta (+ residual)).
 * The trainable parameters as ONE flat fp32 buffer of hpe_encoder_param_floats() floats, layer after layer in table order: kernel HWIO,
 * bias, gamma, beta.  hpe_encoder_param_offset(idx, which): the first float of layer idx's kernel (which 0), bias (1), gamma (2) or
 * beta (3); -1 otherwise.  The statistics are not in it.  Host code: no device is needed. */
int hpe_encoder_param_floats(void);
int hpe_encoder_param_offset(int idx, int which);
/* hpe_encoder_train_reserve allocates, once and outside any capture, what the calls below need for batches up to B (1 <= B <= max_batch):
 * the activation stash (every layer's output and the pooled map, about 11 M floats per image), the cotangent buffers, the partial sums of
 * the weight gradient and the data-gradient packings of the weights (about 94 MB, kept beside the forward's packings); it also rebuilds
 * the flat parameters from the packed weights, and stores what hpe_encoder_set_params_dev needs (sqrt(var + eps) per channel in double, a
 * small layer table).  hpe_encoder_train_ws_floats(B): the floats it allocates.  An inference context that never
 * calls it does not grow.  A second call with a B not above the first is a no-op; a larger one is refused (HPE_ERR_STATE).
 * hpe_encoder_wg_slices(idx, B): the number of pixel slices the weight gradient of layer idx is cut into at batch B (host code). */
int hpe_encoder_train_reserve(hpe_ctx* ctx, int B);
long long hpe_encoder_train_ws_floats(int B);
int hpe_encoder_wg_slices(int idx, int B);
/* The encoder layer by layer (the launches of hpe_debug_conv, the max-pool and the average pool; no fused stem, dual or chained launch),
 * every output kept in the stash; images_dev [B,224,224,3], features_dev [B,2048]. */
int hpe_encoder_forward_train(hpe_ctx* ctx, const float* images_dev, int B, float* features_dev, void* stream);
/* Gradient of < grad_features, features > with respect to the flat parameters (grad_flat_dev [hpe_encoder_param_floats()], overwritten).
 * ReLU's gradient is 0 at 0 (TensorFlow's); the max-pool sends each cotangent to the first maximum of its zero-padded window in row-major
 * order.  Stateless: the training forward is run again into the stash first.  No allocation, no synchronisation, capturable on one
 * stream; no atomics and a fixed summation order: the same inputs give the same bits.  It shares the split-K slices and the padded-image
 * buffer of hpe_encoder / hpe_forward*, so it must not overlap them on another stream.
 * HPE_ERR_INVALID for NULL pointers or B outside [1, reserved B]; HPE_ERR_STATE before hpe_finalize or hpe_encoder_train_reserve. */
int hpe_encoder_backward(hpe_ctx* ctx, const float* images_dev, int B, const float* grad_features_dev, float* grad_flat_dev, void* stream);
/* The live encoder parameters in the flat layout (one device copy on `stream`).  Needs hpe_encoder_train_reserve. */
int hpe_encoder_get_params(hpe_ctx* ctx, float* flat_dev, void* stream);
/* Replace the encoder's kernels, biases, gammas and betas by flat_host (HOST memory): the host packing of hpe_finalize runs again for
 * every kernel family the plan uses, and for the data-gradient packings, and is copied into the buffers that already exist -- no pointer
 * changes, captured graphs stay valid.  SYNCHRONOUS (it waits for the device before and after) and NOT capturable.  Afterwards
 * hpe_encoder gives the bits of a fresh context that loaded the same values.  Needs hpe_encoder_train_reserve. */
int hpe_encoder_set_params(hpe_ctx* ctx, const float* flat_host);
/* The same replacement from DEVICE memory, in stream order: flat_dev [hpe_encoder_param_floats()] is read by a few gather kernels on
 * `stream` (one per packing form, every layer in one launch; seven launches and one copy) that rewrite, in the buffers that already
 * exist, every packing the context holds -- the GEMM weights Wt[n_pad][k_pad], their bf16 split, both Winograd forms, the fused-stem
 * weights, the folded BatchNorm scale / shift, the dual-source weights with their split and shift, the data-gradient packings and the
 * flat copy.  No host copy, no synchronisation, no allocation: capturable.  Moving mean and variance stay as loaded.  Afterwards
 * hpe_encoder, hpe_forward*, hpe_debug_conv, hpe_encoder_forward_train, hpe_encoder_backward and hpe_encoder_get_params give, bit for
 * bit, what a fresh context that loaded the same values gives (the folded values are computed in double in the host packers' operation
 * order; sqrt(var + eps) is taken once, on the host, by hpe_encoder_train_reserve).
 * Ordering: the caller orders the call after everything that still reads the weights.  Launches issued through the same `stream` are
 * ordered by the library: every encoder call makes `stream` wait for its batch-chunk streams before it returns (an event per chunk
 * stream, recorded behind its last launch), so nothing of an earlier call on `stream` can still run when these kernels start; the tail
 * of hpe_forward_pipelined reads no encoder weight.  Calls on other streams, and flat_dev itself until the launches have run, are the
 * caller's to order.  HPE_ERR_INVALID for a NULL ctx or pointer; HPE_ERR_STATE before hpe_finalize or hpe_encoder_train_reserve, on a
 * dead context and on a bf16 context. */
int hpe_encoder_set_params_dev(hpe_ctx* ctx, const float* flat_dev, void* stream);
/* Read-back of one packing of layer idx for tests: `which` names the buffer.  hpe_debug_encoder_packing_bytes: its size in bytes, 0 if
 * this context does not hold that form of that layer (a plan option off, a layer the form does not apply to, HPE_PACK_DXW / HPE_PACK_FLAT
 * before hpe_encoder_train_reserve, a bf16 or unfinalized context, an index out of range).  hpe_debug_encoder_packing copies that many
 * bytes to dst_dev on `stream` (device to device): HPE_ERR_INVALID for idx or which out of range or a NULL pointer, HPE_ERR_STATE where
 * the size is 0.  HPE_PACK_FLAT is layer idx's [kernel | bias | gamma | beta] slice of the flat copy. */
enum {
    HPE_PACK_W = 0,        /* Wt[n_pad][k_pad] fp32 */
    HPE_PACK_W_SPLIT,      /* bf16 [n_pad][3][k_pad] (f32_split) */
    HPE_PACK_WINO_U,       /* F(2x2,3x3) [cout/64][cin/8][16][2][64][4] */
    HPE_PACK_WINO4_U,      /* F(4x4,3x3) [cout/64][cin/4][36][64][4] */
    HPE_PACK_STEM_W,       /* conv1: bf16 [3][64][7][32], the three exact pieces of the fp32 weights */
    HPE_PACK_SCALE,        /* [cout] */
    HPE_PACK_SHIFT,        /* [cout] */
    HPE_PACK_W_DUAL,       /* *_branch2c of a conv_block: [n_pad][K1 + K2] fp32, scales folded in */
    HPE_PACK_W_DUAL_SPLIT, /* bf16 [n_pad][3][K1 + K2] */
    HPE_PACK_SHIFT_DUAL,   /* [cout] */
    HPE_PACK_DXW,          /* data-gradient operand Wt[cin padded to 128][taps * cout], taps flipped */
    HPE_PACK_FLAT,         /* the layer's slice of the flat parameters */
    HPE_PACK_COUNT
};
long long hpe_debug_encoder_packing_bytes(hpe_ctx* ctx, int idx, int which);
int hpe_debug_encoder_packing(hpe_ctx* ctx, int idx, int which, void* dst_dev, void* stream);
/* One layer's gate, weight gradient and data gradient: x_dev the layer's input (idx 0: the images), y_dev its output (after ReLU; the
 * gate is [y > 0]) or NULL for a layer without activation (the projection shortcuts in the network: dz = dy), dy_dev the cotangent of y.  grad_layer_dev receives [kernel | bias | gamma | beta] of that layer, dx_dev
 * [B,hin,hin,cin] the data gradient (NULL: not computed; must be NULL for idx 0). */
int hpe_debug_conv_backward(hpe_ctx* ctx, int idx, const float* x_dev, const float* y_dev, const float* dy_dev, int B, float* dx_dev,
                            float* grad_layer_dev, void* stream);
/* x_dev [B,H,H,C] (the max-pool's input), dy_dev [B,H/2,H/2,C] -> dx_dev [B,H,H,C]; dy_dev [B,C] -> dx_dev [B,HW,C] */
int hpe_debug_maxpool_backward(const float* x_dev, const float* dy_dev, int B, int H, int C, float* dx_dev, void* stream);
int hpe_debug_avgpool_backward(const float* dy_dev, int B, int HW, int C, float* dx_dev, void* stream);
/* Copies layer idx's output of the last training forward (hpe_encoder_forward_train / hpe_encoder_backward), B images of it, to out_dev;
 * idx -1: the max-pooled map [B,56,56,64]. */
int hpe_debug_encoder_stash(hpe_ctx* ctx, int idx, float* out_dev, void* stream);
/* The batch of the last training forward, i.e. the images hpe_debug_encoder_stash copies (0: none has run). */
int hpe_debug_encoder_stash_batch(hpe_ctx* ctx);

/* -- mixed-precision encoder training: bf16 walks on an fp32 context --
 * The context keeps its fp32 master weights, hpe_encoder_set_params(_dev) and every fp32 call as they are; the calls below run the
 * frozen-statistics training forward and backward with bf16 activations, bf16 cotangents and bf16 matrix products accumulated in fp32.
 * fp32 contexts only (a bf16 context: HPE_ERR_STATE).  Images, features, grad_features and the flat gradient stay fp32.  RNE = round to
 * nearest even to bf16; every sum is taken in fp32 in a fixed order:
 *   W16 = RNE(W);  pixels are RNE-rounded by the bf16 pad;  y = RNE(act(s * acc + shift (+ res))), s / shift the context's folded fp32
 *   BatchNorm, the residual added in fp32 before the one rounding;  the max-pool is exact;  features = (fp32 sum of 49 bf16 values) / 49;
 *   g = RNE(grad_features / 49);  dz = dy * [y > 0] exact;  dzs = RNE(dz * s);  dx = RNE(acc (+ block cotangent));  the stride-2 scatter is
 *   exact;  the max-pool backward sums its at most four cotangents in fp32 and rounds once.  G = A^T dz, dW = s * G, dshift, db, dbeta and
 *   dgamma = (<W16, G> + (b - mean) * dshift) / sqrt(var + eps) are fp32 and never rounded to bf16.
 * The bf16 weight operands are cast from the context's live fp32 weights by one launch at the start of EVERY mixed call: after
 * hpe_encoder_set_params(_dev)(q) the next mixed call computes with RNE(q), and the setters do not know of these buffers.
 * hpe_encoder_train_reserve_mixed: hpe_encoder_train_reserve(ctx, B) if that has not run, then, once and outside any capture: a bf16 stash,
 * bf16 cotangent and operand buffers, the padded bf16 input, the bf16 weight operands of all 53 layers (Wt[n_pad][k_pad], k_pad a multiple
 * of 64), the 52 bf16 data-gradient operands and the table of the cast launch.  The weight-gradient partials, the flat copy and the
 * statistics of the fp32 reserve are shared.  hpe_encoder_train_ws_floats_mixed(B): the floats of both reserves together (host code).
 * A second call with a B not above the first is a no-op; a larger one is refused (HPE_ERR_STATE). */
int hpe_encoder_train_reserve_mixed(hpe_ctx* ctx, int B);
long long hpe_encoder_train_ws_floats_mixed(int B);
/* The contract of hpe_encoder_forward_train / hpe_encoder_backward: the backward is stateless (it reruns the forward), grad_flat_dev is
 * overwritten, the same inputs give the same bits, no atomics, no allocation, capturable on one stream.  HPE_ERR_STATE before the mixed
 * reserve; HPE_ERR_INVALID for NULL pointers or B outside [1, batch of the mixed-precision reserve]. */
int hpe_encoder_forward_train_mixed(hpe_ctx* ctx, const float* images_dev, int B, float* features_dev, void* stream);
int hpe_encoder_backward_mixed(hpe_ctx* ctx, const float* images_dev, int B, const float* grad_features_dev, float* grad_flat_dev, void* stream);
/* hpe_debug_conv_backward in mixed precision: x_dev, y_dev (or NULL), dy_dev and dx_dev (or NULL) are bf16; for idx 0 x_dev is the fp32
 * image tensor and dx_dev must be NULL.  grad_layer_dev is fp32. */
int hpe_debug_conv_backward_mixed(hpe_ctx* ctx, int idx, const void* x_dev, const void* y_dev, const void* dy_dev, int B, void* dx_dev,
                                  float* grad_layer_dev, void* stream);
/* The pool backwards on bf16 maps (C a multiple of 8): x_dev, dy_dev, dx_dev bf16; the average pool's dy_dev [B,C] is fp32. */
int hpe_debug_maxpool_backward_mixed(const void* x_dev, const void* dy_dev, int B, int H, int C, void* dx_dev, void* stream);
int hpe_debug_avgpool_backward_mixed(const float* dy_dev, int B, int HW, int C, void* dx_dev, void* stream);
/* The mixed stash (bf16) of the last mixed forward, and that call's batch: a counter of its own, not the fp32 stash's. */
int hpe_debug_encoder_stash_mixed(hpe_ctx* ctx, int idx, void* out_dev, void* stream);
int hpe_debug_encoder_stash_batch_mixed(hpe_ctx* ctx);

/* -- encoder training with batch statistics: BatchNorm in training mode (src/trainer.py:386, image_feature_extractor(images, training=True)) --
 * fp32 contexts only.  Per layer, M = B * hout * hout rows:  z = conv(x, W) + b,  mu = mean_m z,  var = mean_m (z - mu)^2 (biased),
 * r = 1 / sqrt(var + eps),  xhat = (z - mu) * r,  y = act(gamma * xhat + beta (+ residual)).  Backward:  dz = dy * [y > 0] (a projection
 * shortcut: dz = dy),  dbeta = sum_m dz,  dgamma = sum_m dz * xhat,  dzraw = gamma * r * (dz - dbeta / M - xhat * dgamma / M),
 * dW = A^T dzraw,  dx = dzraw . W^T;  the bias gradient is written as exactly 0 (the bias cancels in z - mu).  The sums are accumulated in
 * double in a fixed order, no atomics: the same inputs give the same bits.  The frozen-statistics calls above are untouched by all of this.
 * The moving statistics as ONE fp32 tensor of hpe_encoder_stat_floats() = 2 * (channels of all layers) floats: moving_mean of every layer in
 * table order, then moving_variance of every layer in table order.  hpe_encoder_stat_offset(idx, which): the first float of layer idx's
 * mean (which 0) or variance (1); -1 otherwise.  Host code: no device is needed. */
int hpe_encoder_stat_floats(void);
int hpe_encoder_stat_offset(int idx, int which);
/* hpe_encoder_train_reserve_batchnorm: hpe_encoder_train_reserve(ctx, B) if that has not run, then, once and outside any capture, what the
 * batch-statistics calls need beyond it: a stash of every layer's raw output z (about 11 M floats per image), the batch statistics, the
 * installed moving statistics and the reduction partials.  hpe_encoder_train_ws_floats_batchnorm(B): the floats of both reserves together.
 * A context that only calls hpe_encoder_train_reserve does not grow.  A second call with a B not above the first is a no-op; a larger one
 * is refused (HPE_ERR_STATE).
 * Every call below returns HPE_ERR_STATE before this reserve. */
int hpe_encoder_train_reserve_batchnorm(hpe_ctx* ctx, int B);
long long hpe_encoder_train_ws_floats_batchnorm(int B);
/* hpe_encoder_forward_train / hpe_encoder_backward with batch statistics.  Each layer runs the convolution launch of the frozen forward
 * with a unit scale and the bias as shift, the two statistics launches and one elementwise launch; both calls keep y AND z of every layer
 * and the batch statistics of every layer (what hpe_encoder_update_stats reads).  The backward runs its own forward again and writes the
 * flat layout of hpe_encoder_backward (every bias slot 0).  No allocation, no synchronisation, capturable on one stream; the workspace
 * sharing of hpe_encoder_backward applies.  HPE_ERR_INVALID for NULL pointers or B outside [1, batch of the batch-norm reserve]. */
int hpe_encoder_forward_batchnorm(hpe_ctx* ctx, const float* images_dev, int B, float* features_dev, void* stream);
int hpe_encoder_backward_batchnorm(hpe_ctx* ctx, const float* images_dev, int B, const float* grad_features_dev, float* grad_flat_dev, void* stream);
/* The moving statistics as installed (as loaded, until hpe_encoder_set_stats_dev), one device copy on `stream`. */
int hpe_encoder_get_stats(hpe_ctx* ctx, float* stats_dev, void* stream);
/* stats_dev <- momentum * stats_dev + (1 - momentum) * batch, in place on the caller's tensor, from the batch statistics of the last
 * hpe_encoder_forward_batchnorm / hpe_encoder_backward_batchnorm (HPE_ERR_STATE if there has been none); unbiased != 0 multiplies each
 * batch variance by M / (M - 1), M = that call's B * hout * hout of the layer.  In double, one rounding.  One launch, capturable.
 * Keras' momentum is 0.99.  HPE_ERR_INVALID for a momentum outside [0, 1].  It installs nothing: hpe_encoder_set_stats_dev does. */
int hpe_encoder_update_stats(hpe_ctx* ctx, float* stats_dev, double momentum, int unbiased, void* stream);
/* Install stats_dev as the moving statistics, in stream order: the per-channel mean, sqrt(var + eps) (double, correctly rounded) and its
 * reciprocal are rewritten, then the two repack launches that fold them (BatchNorm scale / shift, the dual-source weights where the
 * context holds them) run again from the live flat parameters.  No host work, no synchronisation, capturable; the ordering rules of
 * hpe_encoder_set_params_dev apply.  After hpe_encoder_set_params_dev(q) and hpe_encoder_set_stats_dev(t), in either order, every packing
 * equals, byte for byte, that of a fresh context that loaded (q, t).  hpe_encoder_set_params (the host path) folds the installed statistics. */
int hpe_encoder_set_stats_dev(hpe_ctx* ctx, const float* stats_dev, void* stream);
/* One layer in batch-statistics mode for tests: z_out_dev [B,hout,hout,cout] the raw output, y_dev the activated one, stats_out_dev
 * [2 * cout] = mu | var of this call.  The backward takes z_dev and y_dev (NULL: no activation, dz = dy) as inputs, recomputes the batch
 * statistics from z_dev, and fills grad_layer_dev = [kernel | bias = 0 | gamma | beta] and dx_dev (NULL: not computed; NULL for idx 0).
 * Neither touches the statistics of the last whole-network call.  Device pointers are 16-byte aligned. */
int hpe_debug_conv_batchnorm(hpe_ctx* ctx, int idx, const float* x_dev, int B, const float* residual_dev, int relu, float* y_dev, float* z_out_dev,
                             float* stats_out_dev, void* stream);
int hpe_debug_conv_backward_batchnorm(hpe_ctx* ctx, int idx, const float* x_dev, const float* z_dev, const float* y_dev, const float* dy_dev, int B,
                                      float* dx_dev, float* grad_layer_dev, void* stream);
/* Layer idx's raw output z of the last batch-statistics forward (B images of it), and mu | var of all layers of that forward in the
 * statistics layout; HPE_ERR_STATE if none has run. */
int hpe_debug_encoder_stash_raw(hpe_ctx* ctx, int idx, float* out_dev, void* stream);
int hpe_debug_encoder_batch_stats(hpe_ctx* ctx, float* out_dev, void* stream);
/* For tests: the pixel slices the column sums of layer idx are cut into at batch B (host code; -1 for an idx or B out of range). */
int hpe_debug_encoder_bn_slices(int idx, int B);

/* -- data-parallel training: the batch statistics over the batch of ALL ranks --
 * Rank r holds B_r of the G images of a step.  A reduce hook joins the ranks: it adds `count` doubles at dev_buf (device memory) over
 * the ranks, in place, ordered on `stream`, and returns 0, or nonzero for a failure.  It is called from inside the library call, on
 * the calling thread, and may run any host code (an all-reduce of a process group, say); it must not synchronise the device unless
 * its transport needs that. */
typedef int (*hpe_reduce_fn)(void* user, double* dev_buf, long long count, void* stream);
/* hpe_encoder_set_reduce(ctx, fn, user, G): from now on hpe_encoder_forward_batchnorm and hpe_encoder_backward_batchnorm take every
 * layer's statistics over G * hout * hout rows.  Per layer the forward adds its local column sums (sum z | sum z^2, the order of the
 * one-rank reduction) into [2][cout] doubles, calls fn on them and finishes mu, var and r from the reduced sums with the formulas of the
 * one-rank path; the backward does the same with (sum dz | sum dz * xhat) and divides by the global M in dzraw: 2 * 53 hook calls per
 * backward (its own forward included).  grad_flat stays this rank's PARTIAL in every entry -- dgamma and dbeta are written from the
 * local sums, dW from the local rows, db is 0 -- so that ONE sum over the ranks of the whole flat tensor is the gradient of the
 * global batch.  hpe_encoder_update_stats then uses M = G * hout * hout for the unbiased factor of statistics such a call left.
 * With an identity hook and G = B every result has the bits of the path without a hook.  fn == NULL clears the hook (G is ignored):
 * every call is again, bit for bit, what it was.  The one-layer debug calls never call the hook.
 * A hook failure ends the walk: HPE_ERR_REDUCE, hpe_last_error() names the layer; the outputs are then undefined.  With a hook set, a
 * call on a stream that is being captured is refused (HPE_ERR_STATE): the hook is host code.  B > G is refused (HPE_ERR_INVALID).  No
 * allocation: the reduce buffers are part of the reserve (hpe_encoder_train_ws_floats_batchnorm counts them).
 * HPE_ERR_INVALID for a NULL ctx or, with fn, G outside [1, 65536]; HPE_ERR_STATE before hpe_encoder_train_reserve_batchnorm. */
int hpe_encoder_set_reduce(hpe_ctx* ctx, hpe_reduce_fn fn, void* user, int global_batch);
/* The two halves of one layer's reductions for tests, so that the arithmetic of a layer split over ranks can be checked on one device
 * (sums of the parts added on the host).  All of them leave the statistics of the last whole-network call alone.
 * hpe_debug_bn_sums: sums_out_dev [2][cout] doubles = (sum z | sum z^2) over the B * hout * hout rows of z_dev.
 * hpe_debug_bn_finish: mu, var, r from sums_dev over M rows (the caller's M: the rows of all parts), stats_out_dev [2 * cout] = mu |
 * var, and y_dev = act(BN(z_dev) (+ residual_dev)) of the B images given.
 * hpe_debug_bn_backward_sums: with mu and r from (sums_dev, M) as above, sums_out_dev [2][cout] doubles = (sum dz | sum dz * xhat)
 * over the rows given (y_dev NULL: no activation, dz = dy).
 * hpe_debug_bn_backward_finish: the layer's backward on the rows given, with the statistics of (sums_dev, M) and the reduced
 * bwd_sums_dev: grad_layer_dev = [kernel | bias = 0 | gamma | beta], each the PARTIAL of these rows, and dx_dev (NULL: not computed;
 * NULL for idx 0).  HPE_ERR_INVALID for a bad idx, a NULL pointer, B outside the batch-norm reserve or M < B * hout * hout. */
int hpe_debug_bn_sums(hpe_ctx* ctx, int idx, const float* z_dev, int B, double* sums_out_dev, void* stream);
int hpe_debug_bn_finish(hpe_ctx* ctx, int idx, const double* sums_dev, long long M, const float* z_dev, int B, const float* residual_dev, int relu,
                        float* y_dev, float* stats_out_dev, void* stream);
int hpe_debug_bn_backward_sums(hpe_ctx* ctx, int idx, const float* z_dev, const float* y_dev, const float* dy_dev, int B, const double* sums_dev,
                               long long M, double* sums_out_dev, void* stream);
int hpe_debug_bn_backward_finish(hpe_ctx* ctx, int idx, const float* x_dev, const float* z_dev, const float* y_dev, const float* dy_dev, int B,
                                 const double* sums_dev, const double* bwd_sums_dev, long long M, float* dx_dev, float* grad_layer_dev,
                                 void* stream);

/* -- mixed-precision encoder training with batch statistics: the bf16 walks with BatchNorm in training mode --
 * The calls of "encoder training with batch statistics" on the buffers of "mixed-precision encoder training": bf16 activations,
 * cotangents and matrix products accumulated in fp32; BatchNorm arithmetic in fp32, its reductions in double.  fp32 contexts only.  The
 * rounding points of the mixed section hold for W16, the pad, the pools, g and the scatter; per layer, M = B * hout * hout:
 *   z16 = RNE(acc + b): the layer's bf16 convolution launch with a unit scale and the bias of the flat copy as shift;
 *   mu, var (biased), r: the statistics OF z16 (double sums of the bf16 values and their squares), into the slots of the fp32 walk;
 *   y16 = RNE(act(gamma * ((z16 - mu) * r) + beta (+ res16))), fp32, the residual added before the one rounding;
 *   dz = dy16 * [y16 > 0] exact (a projection shortcut: dz = dy16);  xhat = (z16 - mu) * r in fp32;  dbeta = sum_m dz and
 *   dgamma = sum_m dz * xhat in double, written as fp32, never rounded to bf16;  db = 0 exactly;
 *   dzraw16 = RNE(gamma * r * (dz - dbeta / M - xhat * (dgamma / M)));  dW = A^T dzraw16 in fp32;  dx = RNE(acc (+ block cotangent)).
 * No product is fused into a sum in the elementwise passes, so a float32 restatement gives their bits.
 * hpe_encoder_train_reserve_batchnorm_mixed: hpe_encoder_train_reserve_mixed(ctx, B) and hpe_encoder_train_reserve_batchnorm(ctx, B) if
 * they have not run, then, once and outside any capture, a bf16 stash of every layer's raw output z16 (laid out as the fp32 one).  The
 * fp32 y and z stashes of the two shared reserves come with it.  hpe_encoder_train_ws_floats_batchnorm_mixed(B): the floats of all of
 * it together (host code; 0 for B < 1).  A second call with a B not above the first is a no-op; a larger one is refused (HPE_ERR_STATE).
 * hpe_encoder_forward_batchnorm_mixed / hpe_encoder_backward_batchnorm_mixed: the contract of the _mixed pair (stateless backward, the
 * same inputs give the same bits, no atomics, no allocation, capturable on one stream without a hook), and that of the _batchnorm pair
 * for the statistics and the hook: they fill the batch statistics that hpe_encoder_update_stats and hpe_debug_encoder_batch_stats read
 * (those of the last batch-statistics call of EITHER precision), and a reduce hook (hpe_encoder_set_reduce) is called at the same two
 * places per layer with the same sums.  HPE_ERR_STATE before this reserve, on a bf16 context, or on a captured stream with a hook set;
 * HPE_ERR_INVALID for NULL pointers, B outside [1, batch of this reserve] or above the hook's global batch. */
int hpe_encoder_train_reserve_batchnorm_mixed(hpe_ctx* ctx, int B);
long long hpe_encoder_train_ws_floats_batchnorm_mixed(int B);
int hpe_encoder_forward_batchnorm_mixed(hpe_ctx* ctx, const float* images_dev, int B, float* features_dev, void* stream);
int hpe_encoder_backward_batchnorm_mixed(hpe_ctx* ctx, const float* images_dev, int B, const float* grad_features_dev, float* grad_flat_dev,
                                         void* stream);
/* hpe_debug_conv_batchnorm / hpe_debug_conv_backward_batchnorm in mixed precision: x_dev, residual_dev, y_dev, z_out_dev, z_dev, dy_dev
 * and dx_dev are bf16, stats_out_dev and grad_layer_dev fp32; for idx 0 x_dev is the fp32 image tensor and dx_dev must be NULL.  Neither
 * touches the statistics of the last whole-network call nor calls the hook. */
int hpe_debug_conv_batchnorm_mixed(hpe_ctx* ctx, int idx, const void* x_dev, int B, const void* residual_dev, int relu, void* y_dev,
                                   void* z_out_dev, float* stats_out_dev, void* stream);
int hpe_debug_conv_backward_batchnorm_mixed(hpe_ctx* ctx, int idx, const void* x_dev, const void* z_dev, const void* y_dev, const void* dy_dev,
                                            int B, void* dx_dev, float* grad_layer_dev, void* stream);
/* Layer idx's raw output z16 (bf16) of the last mixed batch-statistics forward, B images of it; HPE_ERR_STATE if none has run.  (After
 * such a forward hpe_debug_encoder_stash_raw is refused: the fp32 z stash does not hold what the statistics were taken of.) */
int hpe_debug_encoder_stash_raw_mixed(hpe_ctx* ctx, int idx, void* out_dev, void* stream);

/* Both reprojection losses of all n_stage IEF stages in ONE call -- what Trainer.val_step evaluates per step
 * (src/trainer.py:274-296): the work that depends only on seg_gts (tf.where compaction, src/trainer.py:291;
 * the silhouette bitmap) is done once per call instead of once per stage.
 * kp2d_dev[i] [B,K,2] and verts2d_dev[i] [B,P,2] are host arrays of n_stage device pointers; seg_dev /
 * verts2d_dev may be NULL (keypoint loss only).  out_dev [n_stage][4] = {kp numerator, kp count, kp loss,
 * mesh loss sum}: a rank all-reduces the whole [n_stage][4] block once and re-divides column 0 by column 1. */
int hpe_val_losses(hpe_ctx* ctx, const float* seg_dev, const float* kp_gt_dev, const float* const* kp2d_dev,
                   const float* const* verts2d_dev, int n_stage, int B, int K, int H, int W, int P, float* out_dev, void* stream);

/* What a checkpoint is scored by (DESIGN.md "Checkpoint scores"), for all n_stage IEF stages of a batch in ONE launch, one workgroup per
 * image: the confusion counts of the projected mesh's silhouette against the mask, and the keypoint errors in pixels.
 * Silhouette part (verts2d_dev == NULL: none; then faces_dev, seg_dev and counts_dev are not read): verts2d_dev is a host array of
 * n_stage device pointers, each [B,P,2] in the pixel coordinates of hpe_reproject_vertices; faces_dev [F,3] vertex indices (a face with
 * an index outside [0, P) is dropped); seg_dev [B,H,W], foreground where > 0.  Mask pixel (row i, column j) is the point (x, y) = (j, i).
 * Vertices are snapped to X = rint(256 x), Y = rint(256 y); a face is dropped when a vertex is non-finite or outside +-16384 px or its
 * snapped area is 0; both windings are drawn; a pixel is covered when its point is inside some face by the renderer's rule (int64 edge
 * functions, top-left tie rule).  counts_dev [n_stage][B][4] = tp, fp, fn, tn with "positive" = covered.
 * Keypoint part (kp_gt_dev == NULL: none): kp_gt_dev [B,K,3] normalised x, y and visibility, kp2d_dev n_stage pointers, each [B,K,2];
 * kp_err_dev [n_stage][B][K] = hypot(0.5 W dx, 0.5 H dy) in pixels, -1 where the joint's visibility is not > 0; norm_dev [B][2] = the
 * ground truth's torso (joint 9 to joint 2) and head (joint 13 to joint 12) length in pixels, -1 where an end is not visible or K is
 * too small to hold it.
 * Stateless like hpe_orth_proj: no context, no workspace, no synchronisation, no allocation, no atomics on global memory, capturable; the
 * same inputs give the same bits.  HPE_ERR_INVALID with a message for both parts absent, a NULL pointer of a part that is present,
 * n_stage outside [1, 16], B, H, W < 1 (F, P, K < 1 where read), or H, W whose two bitmaps of H * ceil(W / 32) dwords do not fit the
 * 64 KiB of LDS of a workgroup. */
int hpe_eval_scores(const float* const* verts2d_dev, const int* faces_dev, int F, const float* seg_dev, const float* kp_gt_dev,
                    const float* const* kp2d_dev, int n_stage, int B, int P, int K, int H, int W, int* counts_dev, float* kp_err_dev,
                    float* norm_dev, void* stream);

/* The 3-D scores of a batch (DESIGN.md "3-D pose scores"; restated in float64 by tests/pose3d_ref.py), for all n_stage IEF stages in ONE
 * launch, one workgroup per (image, stage).  joints_dev: a host array of n_stage device pointers, each [B,K,3]; joints_gt_dev [B,K,3];
 * joint_weights_dev [B,K], a joint is scored where its weight is > 0 (NULL: all are).  verts_dev (n_stage pointers, each [B,P,3]) and
 * verts_gt_dev [B,P,3] are given together or both NULL (joints only).  Units are the caller's.
 * The fit of a predicted cloud X to the ground truth Y over the scored points: means mu1, mu2; K = sum (x - mu1) (y - mu2)^T;
 * var1 = sum |x - mu1|^2; R the proper rotation that maximises trace(R K) (never a reflection); scale = trace(R K) / var1;
 * t = mu2 - scale R mu1.  It is undefined for fewer than 3 scored points or var1 == 0.  var1 is taken as sum |x'|^2 - n |mean x'|^2 of
 * the points relative to the first scored one, and the test is "<= 0": exact for points that coincide (every x' is 0), while points
 * within rounding of each other, not equal, may fall on either side of it -- their fit means nothing either way.  The root of a skeleton is the mean of its joints
 * root_a and root_b (equal: a pelvis joint), defined when both are scored.
 * joint_err_dev [n_stage][B][2][K]: row 0 |(x - rootX) - (y - rootY)|, row 1 |scale R (x - mu1) - (y - mu2)| with the fit on the scored
 *   joints; -1 where the joint is not scored, NaN where the alignment is undefined.
 * summary_dev [n_stage][B][6]: the means of the two rows over the scored joints (MPJPE, PA-MPJPE), the means over all P vertices of the
 *   vertices translated by the JOINT roots (PVE) and aligned by the fit on the vertices themselves (PA-PVE), the number of scored
 *   joints, and the flags as a float: 1 a root joint is not scored (MPJPE and PVE are NaN), 2 the joint fit is undefined (PA-MPJPE is
 *   NaN), 4 the vertex fit is undefined (PA-PVE is NaN), 8 no vertices were given (PVE and PA-PVE are NaN).
 * xform_dev [n_stage][B][2][13]: scale, R row-major, t of the joint fit and of the vertex fit (NaN where undefined or absent).
 * Any output may be NULL, not all.  Every sum and the 3x3 solve are float64 in an order the launch shape fixes; the outputs are float32.
 * A NaN coordinate of a scored point makes that image's values NaN and nothing else.  Stateless like hpe_eval_scores: no context, no
 * workspace, no synchronisation, no allocation, no atomics, capturable; the same inputs give the same bits.  HPE_ERR_INVALID with a
 * message, before any HIP call, for NULL joints (or a NULL entry), n_stage outside [1, 16], B or K < 1, a root outside [0, K), vertices
 * on one side only, P < 1 with vertices, and all three outputs NULL. */
int hpe_pose3d_scores(const float* const* joints_dev, const float* joints_gt_dev, const float* joint_weights_dev, const float* const* verts_dev,
                      const float* verts_gt_dev, int n_stage, int B, int K, int P, int root_a, int root_b, float* joint_err_dev,
                      float* summary_dev, float* xform_dev, void* stream);
/* The host build of the 3x3 solver of the call above (csrc/procrustes3.h): K, R row-major; R is the proper rotation that maximises
 * trace(R K), *trace_RK that maximum.  A K that holds a NaN or an infinity gives NaN.  No device needed. */
int hpe_debug_procrustes3(const double K[9], double R[9], double* trace_RK);

/* The 3-D supervision terms of the generator step (DESIGN.md "3-D supervision"): the joint and SMPL-parameter losses on 3-D ground truth
 * and their gradient, two stateless calls in the style of the one above.  They are an extension of this interface with a header of their
 * own, hpe_loss3d.h, which this header includes: a consumer of hpe.h sees them, and the core list of entry points above stays the list
 * that the binding's core table pins. */
#include "hpe_loss3d.h"

/* -- the steps right before / after the path -------------------------- */
/* preprocess_image (preview.py:18-35) = resize_img + scale_and_crop (src/util/image.py:7-39) + [-1,1] normalisation,
 * fused: img_dev uint8 [H,W,C] (C = 3 or 4, RGB first) -> out224_dev float [224,224,3].
 * proc_param (host, out) = {start_pt.x, start_pt.y, end_pt.x, end_pt.y, img_size}; scale = 224 / max(H, W). */
int hpe_preprocess_u8(const unsigned char* img_dev, int H, int W, int C, float* out224_dev, int proc_param[5], void* stream);
/* The same for a batch of frames in ONE launch.  frames_dev: uint8 frames in one device buffer; frame i starts at byte
 * offsets[i] and is [sizes_hw[2i], sizes_hw[2i+1], C].  offsets == NULL: B frames of one size sizes_hw[0] x sizes_hw[1], back to
 * back (a camera / video stream) -- then no per-image table is needed and table_dev may be NULL.  Otherwise table_dev is a
 * caller-owned device scratch of >= 32 * B bytes; the per-image table is copied into it with a SYNCHRONOUS copy after
 * `stream` has drained (this variant blocks the host and cannot be captured; equal-sized frames never take it).  out_dev [B,224,224,3] float, proc_params (host, out) [B][5] as hpe_preprocess_u8. */
int hpe_preprocess_u8_batch(const unsigned char* frames_dev, const long long* offsets, const int* sizes_hw, int B, int C,
                            float* out_dev, int* proc_params, void* table_dev, void* stream);
/* get_original (src/util/renderer.py:260-283): vert_shifted_dev [B,P,3] = verts + [tx, ty, 500 / (0.5*img_size*s)];
 * cam_for_render (host, out) = {flength/scale, principal point x, y in the original image};
 * kp_original_host [B*K*2] = (joints2d_host + start_pt - img_size/2) / scale (both optional host arrays). */
int hpe_get_original(const float* verts_dev, const float* cam_dev, int B, int P, int K, const int start_pt[2], float scale,
                     int img_size, float* vert_shifted_dev, float cam_for_render[3], float* kp_original_host,
                     const float* joints2d_host, void* stream);

/* -- training-batch augmentation: DataLoader.image_preprocessing (src/data_loader.py:160-213) with jitter_center, jitter_scale,
 * pad_image_edge and random_flip (src/util/data_utils.py:144-238), the random draws as inputs.  What is computed is defined in
 * DESIGN.md "Training-batch augmentation": all float32, in the reference's operation order, casts truncate toward zero. */
typedef struct HpeAugmentFrame {
    long long frame_offset; /* byte offset of the uint8 [H,W,3] image in frames_dev */
    long long seg_offset;   /* byte offset of the uint8 [H,W] mask in segs_dev */
    int H, W;               /* source size */
    int newH, newW;         /* int(float(H) * scale), int(float(W) * scale) */
    int cx, cy;             /* jittered centre in the resized image: int(float(center + trans) * fx), ... * fy) */
    float fx, fy;           /* actual_factor: float(newW) / float(W), float(newH) / float(H) */
    int flip;               /* 0 / 1 */
    int inside;             /* 1: the 224 x 224 window lies inside the resized image padded by 112 + trans_max + 50 (where the reference's
                             * tf.slice succeeds); 0: it leaves it, and the kernel clamps to the edge as if the pad were wider */
    float rx, ry;           /* resize scale of tf.image.resize: float(W) / float(newW), float(H) / float(newH) */
} HpeAugmentFrame;

/* Pure host code, no device needed: fills table_out[B] from sizes_hw [B][2] (H, W), centers_xy [B][2], trans_xy [B][2], scales [B],
 * flips [B] (0 / 1) and the byte offsets of the packed frames and masks.  HPE_ERR_INVALID for a NULL pointer, B < 1, trans_max < 0, a
 * negative offset, H or W outside [1, 2^20], a scale that is not finite and positive, or a frame whose newH or newW is < 1 or > 2^20. */
int hpe_augment_plan(int B, const int* sizes_hw, const int* centers_xy, const int* trans_xy, const float* scales,
                     const unsigned char* flips, int trans_max, const long long* frame_offsets, const long long* seg_offsets,
                     HpeAugmentFrame* table_out);
/* ONE launch: images_out [B,224,224,3] in [-1,1], seg_out [B,224,224] in [0,1] and kp_out [B,19,3] from the packed uint8 frames and
 * masks, the table of hpe_augment_plan and kp_dev [B,19,3] (x, y, visibility in source pixels).  The kernel reads table_dev, the
 * caller's device copy of table_host (in flight on `stream` is enough); table_host is what this call checks.  No allocation, no
 * synchronisation, capturable, no atomics: the same inputs give the same bits.  HPE_ERR_INVALID for a NULL pointer, B outside
 * [1, 65535] and a table entry with H, W, newH or newW < 1 or a negative offset. */
int hpe_augment_batch(const unsigned char* frames_dev, const unsigned char* segs_dev, const HpeAugmentFrame* table_host,
                      const HpeAugmentFrame* table_dev, const float* kp_dev, int B, float* images_out, float* seg_out, float* kp_out,
                      void* stream);

/* -- the optimiser: tf.keras.optimizers.Adam = TensorFlow's fused ResourceApplyAdam (src/trainer.py:183-184) ------------------
 *     alpha = lr * sqrt(1 - beta2^t) / (1 - beta1^t)
 *     m += (g - m) * (1 - beta1);  v += (g * g - v) * (1 - beta2);  p -= (m * alpha) / (sqrt(v) + eps)
 * No ctx: every call takes a stream, launches, and returns; nothing reads the host, so a step is stream-ordered and capturable.
 * state_dev: 4 doubles {t, beta1^t, beta2^t, alpha} on the device; a fresh optimiser is {0, 1, 1, 0}.  HPE_ERR_INVALID for a NULL
 * pointer, a beta outside [0, 1), a lr that is not finite, t < 0 or n < 0. */
/* One single-thread launch: t += 1, both powers from t by square-and-multiply in double, alpha in double. */
int hpe_adam_advance(double* state_dev, double lr, double beta1, double beta2, void* stream);
/* One launch over n elements of p, m, v (updated in place) and g, in float32 in the order above, alpha rounded once to float.  Every
 * element gets the bits of the same lines in IEEE float32 whatever its position, n, or the alignment of the pointers (16-byte aligned
 * pointers take 16-byte loads and stores, anything else a scalar kernel).  n == 0 succeeds and launches nothing. */
int hpe_adam_apply(float* p, float* m, float* v, const float* g, long long n, const double* state_dev, float one_minus_beta1,
                   float one_minus_beta2, float eps, void* stream);
/* Resume: t and both powers as hpe_adam_advance would have left them after t steps; alpha is 0 until the next hpe_adam_advance. */
int hpe_adam_set_step(double* state_dev, long long t, double beta1, double beta2, void* stream);
/* The host build of the power helper of the two calls above: *out = beta^t (t >= 0), square-and-multiply in double.  No device needed. */
int hpe_debug_adam_power(double beta, long long t, double* out);

/* -- the guarded step: global-norm clipping and a skip on non-finite gradients, decided on the device ---------------------------
 * (the reference has neither: src/trainer.py:84.)  hpe_grad_stats per tensor, ONE hpe_adam_guard in the place of hpe_adam_advance, then
 * hpe_adam_apply_guarded per tensor.  Nothing reads the host, nothing allocates, no atomics: stream-ordered and capturable.
 * DESIGN.md "Guarded optimiser step" states the order of every sum; tests/grad_guard_ref.py restates it. */
/* One record of 3 doubles per segment of g[n]: {sum of squares, largest |g| over the finite elements, number of non-finite elements}.
 * The S + 1 ascending offsets (0 <= offsets[0], offsets[S] <= n; equal neighbours: an empty segment, record {0, 0, 0}) cut g into S
 * segments; offsets_host is what this call checks and sizes its grid from, offsets_dev the caller's device copy the kernels read.
 * Squares and sums are float64 ((double)g * (double)g is exact).  A segment is cut into chunks of hpe_grad_stats_chunk() elements from
 * its own start; a chunk is summed in one fixed binary tree, a segment's chunk partials are added in index order: a record's bits depend
 * on the segment's values alone -- not on the grid, the alignment of g, the segment's place in g or the other segments.  A non-finite
 * element's square (inf or NaN) is part of its segment's sum.  16-byte loads where a chunk allows them, scalar loads elsewhere.
 * Three launches (the chunk map, the chunks, the per-segment combine).  workspace_dev: at least hpe_grad_stats_workspace_bytes(n, S)
 * bytes, 8-byte aligned, the caller's (-1 from that query, with hpe_last_error() set, for n < 0 or S < 1).  HPE_ERR_INVALID, before any
 * launch and without a device, for a NULL pointer, n < 0, S < 1, descending offsets, an offset beyond n and a workspace too small. */
int hpe_grad_stats_chunk(void);
long long hpe_grad_stats_workspace_bytes(long long n, int S);
int hpe_grad_stats(const float* g, long long n, const long long* offsets_host, const long long* offsets_dev, int S, double* records_dev,
                   void* workspace_dev, long long workspace_bytes, void* stream);
/* One launch, one deciding thread, float64, nothing contracted.  records_dev / counts (HOST arrays of n_lists <= 16 device pointers and
 * record counts, >= 1 each): the records of the tensors of this step.  sumsq = their sums of squares added in list order, table order
 * within a list; norm = sqrt(sumsq).  skip_nonfinite != 0 and a non-finite count > 0: applied = 0, state_dev keeps its bits (t does not
 * move), skipped += 1.  Otherwise applied = 1, state_dev moves as by hpe_adam_advance, scale = (float)(clip_norm / fmax(norm,
 * clip_norm)) -- exactly 1.0f for norm <= clip_norm, for clip_norm = +inf (no clipping) and for a NaN norm -- and clipped += 1 when
 * scale < 1.  guard_dev: 8 doubles {norm, scale, applied, skipped, clipped, non-finite count, max |g|, sumsq}, zeros on a fresh
 * optimiser; skipped and clipped are running counts, the rest is of this step.  HPE_ERR_INVALID as hpe_adam_advance, and for n_lists
 * outside [1, 16], a NULL list, a count < 1 and a clip_norm that is negative or NaN; no device needed to refuse. */
int hpe_adam_guard(double* state_dev, double* guard_dev, const double* const* records_dev, const int* counts, int n_lists, double lr,
                   double beta1, double beta2, double clip_norm, int skip_nonfinite, void* stream);
/* hpe_adam_apply under a guard block: applied == 0 stores nothing (the launch still happens); otherwise g' = g * scale, one float32
 * multiply, then the element arithmetic of hpe_adam_apply on g' on the same paths.  scale == 1.0f gives the bits of hpe_adam_apply. */
int hpe_adam_apply_guarded(float* p, float* m, float* v, const float* g, long long n, const double* state_dev, const double* guard_dev,
                           float one_minus_beta1, float one_minus_beta2, float eps, void* stream);

/* -- JPEG decode: tf.image.decode_jpeg(buf, channels) of the training records (src/util/data_utils.py:129-141) ---------------
 * Baseline sequential DCT streams only (SOF0, 8-bit samples and quantisation tables, 1 or 3 components, luma sampling 1x1, 2x1 or
 * 2x2 with 1x1 chroma, one interleaved scan, DRI / RST, any DHT).  Everything else is refused with HPE_ERR_INVALID and a message that
 * names the image index and the clause.  Entropy decoding is host code (hpe_jpeg_info, hpe_jpeg_decode: no device needed);
 * dequantisation, inverse DCT, chroma upsampling, colour conversion and the store are two launches (hpe_jpeg_backend).  What is
 * computed is libjpeg's default decode (JDCT_ISLOW, fancy upsampling) in 32-bit integers, bit for bit: DESIGN.md "Training records and
 * JPEG decode". */
#define HPE_JPEG_MAX_SIDE 16384 /* larger frames are refused */
typedef struct HpeJpegInfo {
    int status;       /* HPE_OK, or HPE_ERR_INVALID: the stream is refused and every other field is 0 */
    int H, W, ncomp;  /* ncomp 1 (grey) or 3 (YCbCr) */
    int hs[3], vs[3]; /* sampling factors per component (a grey stream: 1, 1) */
    int blocks_w[3], blocks_h[3]; /* block grid per component plane, padded to whole MCUs */
    long long coefs;  /* int16 coefficients of all components: 64 * sum of blocks_w * blocks_h */
} HpeJpegInfo;

typedef struct HpeJpegImage {
    long long coef_offset[3];  /* index of component c's first int16 in the coefficient buffer: natural order, 64 per block, blocks
                                * row-major over [blocks_h, blocks_w] */
    long long plane_offset[3]; /* byte offset of component c's uint8 sample plane [8 * blocks_h, 8 * blocks_w] in the workspace */
    long long out_offset;      /* byte offset of the uint8 [H,W,channels] frame in the frame buffer, a multiple of 16 */
    int H, W;
    int ncomp;                 /* components stored: 1 (a grey stream, or channels == 1: Y alone) or 3 */
    int channels;              /* 1 or 3 */
    int hmax, vmax;            /* the stream's luma sampling: the chroma upsampling factors, and what pads every block grid to whole
                                * MCUs (so also set when Y alone is stored; a grey stream has 1, 1) */
    int blocks_w[3], blocks_h[3];
    int idct_group0;           /* first workgroup of this image in launch one (32 blocks per workgroup) */
    int store_group0;          /* first workgroup of this image in launch two (1024 output bytes per workgroup) */
    unsigned char quant[3][64]; /* quantisation table per component, natural order */
} HpeJpegImage;

/* Info pass over B streams: info_out[b] for every stream.  HPE_OK if all are accepted; HPE_ERR_INVALID if one is refused (its
 * info_out[b].status says which; hpe_last_error() names the first) or for a NULL pointer, B < 1 or a negative length. */
int hpe_jpeg_info(int B, const unsigned char* const* streams, const long long* lengths, HpeJpegInfo* info_out);
/* Decode pass over B streams: channels[b] in {1, 3} (1 on a colour stream stores the Y blocks only; 3 on a grey stream replicates Y in
 * the back end), threads in [1, 16] std::threads over the images (the bytes written do not depend on it).  Fills table_out[b] (offsets
 * of images packed in order: coefficients on 8-element, planes and frames on 16-byte boundaries), status_out[b], and totals_out[5] =
 * {int16 coefficients, workspace bytes, frame-buffer bytes, workgroups of launch one, workgroups of launch two}.  coef_out == NULL: layout
 * only (headers are parsed, table offsets and totals are filled, quant is not).  Otherwise the coefficients are written, never past
 * coef_capacity (int16 elements; HPE_ERR_INVALID before anything is written if the total exceeds it).  A refused stream gets
 * status_out[b] = HPE_ERR_INVALID and an all-zero table entry, and the call returns HPE_ERR_INVALID naming the first one. */
int hpe_jpeg_decode(int B, const unsigned char* const* streams, const long long* lengths, const int* channels, int threads,
                    short* coef_out, long long coef_capacity, HpeJpegImage* table_out, int* status_out, long long* totals_out);
/* Two launches on `stream`: coefficients -> uint8 sample planes in workspace_dev (dequantisation + 8x8 inverse DCT), planes -> packed
 * frames in frames_dev (upsampling + colour conversion).  The kernels read table_dev, the caller's device copy of table_host (in flight
 * on `stream` is enough); table_host is what this call checks, entry by entry, against coef_count (int16 elements), workspace_bytes and
 * frames_bytes before anything is launched.  Bytes of frames_dev outside the frames are not written.  No allocation, no
 * synchronisation, no atomics, capturable: the same inputs give the same bits. */
int hpe_jpeg_backend(const HpeJpegImage* table_host, const HpeJpegImage* table_dev, int B, const short* coef_dev, long long coef_count,
                     unsigned char* workspace_dev, long long workspace_bytes, unsigned char* frames_dev, long long frames_bytes,
                     void* stream);

/* -- JPEG encode: tf.image.encode_jpeg of the dataset writers (src/util/create_dataset.py:36-40), the mirror of the decoder --------
 * libjpeg's default baseline compressor bit for bit (jccolor.c, jcsample.c without smoothing, the edge rules of jcprepct.c and
 * jccoefct.c, jfdctint.c, the Annex K Huffman tables, no optimisation, no restart markers): DESIGN.md "Dataset writers and JPEG
 * encode".  Colour conversion, chroma downsampling, forward DCT and quantisation are one launch (hpe_jpeg_forward); the layout and the
 * entropy coder are host code (hpe_jpeg_encode_layout, hpe_jpeg_entropy_encode: no device needed). */
#define HPE_JPEG_ENC_HEADER_BYTES 640 /* covers every header and EOI (625 bytes for three components) */
#define HPE_JPEG_ENC_BLOCK_BYTES 416  /* no block's entropy-coded bytes are more: 63 AC terms of 16 + 10 bits, a DC of 11 + 11, all stuffed */
typedef struct HpeJpegEncImage {
    long long frame_offset;   /* byte offset of the packed uint8 [H,W,C] frame in the frame buffer */
    long long coef_offset[3]; /* as HpeJpegImage.coef_offset: natural order, 64 per block, blocks row-major over [blocks_h, blocks_w] */
    int H, W;                 /* 1 .. HPE_JPEG_MAX_SIDE */
    int C;                    /* 1 (grey: one component) or 3 (RGB: Y, Cb, Cr) */
    int hmax, vmax;           /* luma sampling 1x1, 2x1 or 2x2; chroma is 1x1; a grey frame has 1, 1 */
    int blocks_w[3], blocks_h[3]; /* block grid per component plane, padded to whole MCUs */
    int real_w[3], real_h[3]; /* the blocks that hold samples: ceil(ceil(W * h / hmax) / 8) by ceil(ceil(H * v / vmax) / 8); the
                               * others are dummy blocks (AC 0, DC of the previous block of the MCU) */
    int group0;               /* first workgroup of this image in the launch (32 blocks per workgroup) */
    unsigned char quant[2][64]; /* luminance and chrominance quantisation table, natural order, entries 1 .. 255 */
} HpeJpegEncImage;

/* shapes int [B][3] = H, W, C; frame_offsets [B] (bytes); hmax, vmax: the luma sampling of the colour frames (1,1 / 2,1 / 2,2; a grey
 * frame takes 1,1); quality in [1, 100] (libjpeg's scaling of the Annex K tables).  Fills table_out[b] (coefficients packed in order,
 * every plane on an 8-element boundary) and totals_out[3] = {int16 coefficients, workgroups, stream-buffer capacity =
 * sum of HPE_JPEG_ENC_HEADER_BYTES + HPE_JPEG_ENC_BLOCK_BYTES * blocks}.  HPE_ERR_INVALID names the image and the clause. */
int hpe_jpeg_encode_layout(int B, const int* shapes, const long long* frame_offsets, int hmax, int vmax, int quality,
                           HpeJpegEncImage* table_out, long long* totals_out);
/* One launch on `stream`: 8 threads per 8x8 block, every block of every component of every image, dummy blocks included.  The kernel
 * reads table_dev, the caller's device copy of table_host (in flight on `stream` is enough); table_host is what this call checks,
 * entry by entry, against frames_bytes and coef_count (int16 elements) before anything else: with a sound table a NULL device pointer
 * is refused next, so the check runs without a device.  Elements of coef_dev outside the images' planes are not written.  No
 * allocation, no synchronisation, no atomics, capturable: the same inputs give the same bits. */
int hpe_jpeg_forward(const HpeJpegEncImage* table_host, const HpeJpegEncImage* table_dev, int B, const unsigned char* frames_dev,
                     long long frames_bytes, short* coef_dev, long long coef_count, void* stream);
/* Host: coefficient planes -> whole streams (SOI, JFIF APP0 with `units` 0 none / 1 inch / 2 cm and the densities, DQT, SOF0, DHT,
 * SOS, data, EOI).  Image b's stream starts at offsets_out[b] = the sum of the images' bounds before it (see totals_out[2] above) and
 * is lengths_out[b] bytes long.  out_capacity below the batch's bound is refused before anything is written; every write is checked
 * against the image's own bound as well.  A coefficient the standard tables cannot code (|AC| > 1023, |DC difference| > 2047) is
 * refused naming the image.  threads in [1, 16] std::threads over the images; the bytes do not depend on it. */
int hpe_jpeg_entropy_encode(const HpeJpegEncImage* table, int B, const short* coef, long long coef_count, int units, int xdensity,
                            int ydensity, int threads, unsigned char* out, long long out_capacity, long long* offsets_out,
                            long long* lengths_out);

/* -- PNG decode: the PNG streams tf.image.decode_jpeg also takes (LSP masks, MPII frames) -------------------------------------
 * The chunk walk, the CRCs and inflate are host code (hpe_amd/png.py: zlib); what reaches this library is, per image, the inflated
 * scanlines -- H rows of one filter byte and rowbytes filtered bytes -- and a table entry.  Two launches (hpe_png_backend): the PNG
 * unfilter (None, Sub, Up, Average, Paeth), then unpack / palette / channel conversion and the store.  Lossless, so bit for bit:
 * DESIGN.md "PNG streams in the records". */
#define HPE_PNG_MAX_SIDE 16384 /* larger frames are refused */
#define HPE_PNG_STORE_BYTES_PER_GROUP 1024 /* launch two: 4 output bytes per thread, 256 threads */
typedef struct HpePngImage {
    long long raw_offset;  /* byte offset in the raw buffer of the H * (1 + rowbytes) inflated bytes, a multiple of 16 */
    long long pal_offset;  /* colour type 3: byte offset in the raw buffer of 256 entries of 4 bytes (R, G, B, 0), entries beyond PLTE
                            * zero, a multiple of 16; every other colour type: -1 */
    long long work_offset; /* byte offset in the workspace of the H * rowbytes unfiltered bytes, a multiple of 16; -1 for a direct image:
                            * 8-bit grey asked for 1 channel or 8-bit RGB asked for 3, whose unfiltered rows ARE the frame */
    long long out_offset;  /* byte offset of the uint8 [H,W,channels] frame in the frame buffer, a multiple of 16 */
    int H, W;
    int color_type;        /* 0 grey, 2 RGB, 3 palette, 4 grey + alpha, 6 RGBA */
    int depth;             /* 8; also 1, 2, 4 for colour types 0 and 3 */
    int channels;          /* 1 or 3 */
    int rowbytes;          /* ceil(W * samples * depth / 8) */
    int bpp;               /* max(1, samples * depth / 8): the filters' distance to the byte on the left */
    int store_group0;      /* first workgroup of this image in launch two (a direct image has none) */
} HpePngImage;

/* Two launches on `stream`: raw_dev -> unfiltered rows (one workgroup per image; into workspace_dev, or into frames_dev for a direct
 * image), rows -> packed frames in frames_dev.  The kernels read table_dev, the caller's device copy of table_host (in flight on
 * `stream` is enough); table_host is what this call checks, entry by entry, against raw_bytes, workspace_bytes and frames_bytes and
 * against what H, W, colour type and depth imply, before anything else: with a sound table a NULL device pointer is refused next, so
 * the check runs without a device.  Bytes of frames_dev outside the frames are not written.  No allocation, no synchronisation, no
 * atomics, capturable: the same inputs give the same bits. */
int hpe_png_backend(const HpePngImage* table_host, const HpePngImage* table_dev, int B, const unsigned char* raw_dev, long long raw_bytes,
                    unsigned char* workspace_dev, long long workspace_bytes, unsigned char* frames_dev, long long frames_bytes,
                    void* stream);

/* -- PNG encode: the mirror, for the panels of the training summaries -----------------------------------------------------------
 * Packed uint8 frames [H,W,C] with C in {1, 3, 4} -> PNG scanlines: per row one filter byte and W * C filtered bytes, the filter
 * chosen per row by libpng's minimum-sum rule (all five candidates from the raw neighbours, scored by the sum of v < 128 ? v :
 * 256 - v, lowest score, then lowest filter number).  Deflate and the chunks are host code (hpe_amd/png_encode.py).  DESIGN.md
 * "Training summaries". */
typedef struct HpePngFilterImage {
    long long frame_offset; /* byte offset of the uint8 [H,W,C] frame in the frame buffer */
    long long scan_offset;  /* byte offset in the scanline buffer of the H * (1 + W * C) bytes written */
    int H, W;               /* 1 .. HPE_PNG_MAX_SIDE */
    int C;                  /* 1 grey, 3 RGB, 4 RGBA: the filters' bpp */
    int row0;               /* first row of this image in the launch's grid over all rows: the sum of H of the images before */
} HpePngFilterImage;

/* One launch on `stream`, one wave per row.  The kernel reads table_dev, the caller's device copy of table_host (in flight on
 * `stream` is enough); table_host is what this call checks, entry by entry, against frames_bytes and scan_bytes before anything
 * else: with a sound table a NULL device pointer is refused next, so the check runs without a device.  Bytes of scan_dev outside
 * the scanlines are not written.  No allocation, no synchronisation, no atomics, capturable: the same inputs give the same bits. */
int hpe_png_filter(const HpePngFilterImage* table_host, const HpePngFilterImage* table_dev, int B, const unsigned char* frames_dev,
                   long long frames_bytes, unsigned char* scan_dev, long long scan_bytes, void* stream);

/* -- draw_results panels: the skeleton drawing of the reference's draw_skeleton (src/util/renderer.py:286-447) and the panel of
 * visualize_img / draw_results (src/trainer.py:622-679) composed on the device.  The raster rules are this project's own, in exact
 * integer arithmetic (DESIGN.md "Training summaries": PARITY UNPINNED against cv2):  disc d2 <= r*r;  ring of thickness 1
 * (2r-1)^2 <= 4*d2 < (2r+1)^2;  edge of thickness th: 4 * dist2 <= th*th with dist2 the squared distance to the segment, evaluated
 * without a division in 64-bit integers.  Joint pixels are rint of the float coordinate (half to even), clamped to +-32768 (a NaN
 * goes to -32768).  `skeleton` is the device copy of the drawing's tables (hpe_amd/draw.py holds them as data): int32 [19][8], per
 * joint its parent (-1: none), the joint's R, G, B, its edge's R, G, B, and 0. */
#define HPE_DRAW_JOINTS 19
#define HPE_DRAW_MAX_RADIUS 256
/* out uint8 [n, T*S, 3*S, 3]: row block t of image i is hstack[skeleton over the crop, rend_img[i*T+t], rend_seg[i*T+t]].
 * images fp32 [n,S,S,3] in [-1,1]; kp_gt fp32 [n,19,3] (x, y in [-1,1], visibility); kp_pred fp32 [n,T,19,2]; rend_img / rend_seg
 * uint8 [n*T,S,S,3].  The radius is max(4, int(0.01 * S)).  One launch on `stream`, no atomics. */
int hpe_draw_panels(const float* images, const float* kp_gt, const float* kp_pred, const unsigned char* rend_img,
                    const unsigned char* rend_seg, const int* skeleton, int n, int T, int S, unsigned char* out, void* stream);
/* draw_skeleton on n uint8 [H,W,3] images in place: joints fp32 [n,19,2] in PIXELS, vis uint8 [n,19] or NULL (all visible),
 * draw_edges 1: discs and edges of thickness max(1, radius - 2), 0: rings of radius - 1.  radius in [1, HPE_DRAW_MAX_RADIUS].  One
 * launch on `stream`. */
int hpe_draw_skeleton(unsigned char* images, const float* joints, const unsigned char* vis, const int* skeleton, int n, int H, int W,
                      int draw_edges, int radius, void* stream);

/* -- mesh renderer: the reference's SMPLRenderer (src/util/renderer.py:23-112) without OpenDR ---------------------------------
 * A renderer is its own handle (the reference builds SMPLRenderer without a predictor, preview.py:50).  What it computes is
 * defined in DESIGN.md "Renderer": pinhole projection snapped to 1/256 px, rasterisation with int64 edge functions and a
 * top-left tie rule (no MSAA), nearest depth wins (ties to the lower face index), Lambertian shading with the reference's three
 * point lights interpolated perspective-correctly, composited over an optional uint8 background.  No near-plane clipping: a face
 * with a vertex outside [near, far] is dropped.  A renderer is not re-entrant: its workspace serves one call at a time, so calls
 * on different streams must be ordered by the caller. */
typedef struct hpe_renderer hpe_renderer;

typedef struct HpeRenderParams {
    int struct_size; /* sizeof(HpeRenderParams); written by hpe_render_params_init, checked by every render call */
    int color_id;    /* albedo: even = light_blue (the reference's default), odd = light_pink (renderer.py:239-243) */
    int do_alpha;    /* 1: a fourth channel: 255 everywhere with a background, else 255 where a face covers the pixel and 0 elsewhere */
    int rot_axis;    /* 0 none; 1 x, 2 y, 3 z: the view rotation of SMPLRenderer.rotated (renderer.py:84-112) about the mesh mean */
    float rot_deg;   /* rotation angle in degrees */
    float near;      /* < 0: the reference's default max(min z - 25, 0.1) (renderer.py:65-66) */
    float far;       /* < 0: the reference's default max(max z + 25, 25) (renderer.py:67-68) */
} HpeRenderParams;

/* defaults: struct_size = sizeof(HpeRenderParams), color_id 0, do_alpha 0, no rotation, near = far = -1 */
void hpe_render_params_init(HpeRenderParams* p);
/* faces_host [Fn,3] int32, every index in [0, P); the vertex -> face adjacency is built here.  Workspace for max_batch images
 * (1..1024) per hpe_render call.  Synchronises. */
int hpe_renderer_create(int device, const int* faces_host, int Fn, int P, int max_batch, hpe_renderer** out);
int hpe_renderer_destroy(hpe_renderer* r);
/* verts_dev [B,P,3] float camera-space vertices (e.g. vert_shifted of hpe_get_original); cam_dev [B,3] (f, px, py) per image
 * (e.g. cam_for_render) or NULL = (500, W/2, H/2) (renderer.py:53-54); 1 <= B <= max_batch; 1 <= H, W <= 4096; bg_dev
 * [B,H,W,3] uint8 or NULL (white); p NULL = defaults.  out_dev [B,H,W,3] uint8, or [B,H,W,4] with do_alpha.  Vertex colours go
 * to channels 0, 1, 2 in that order, as the reference writes its RGB triples onto a BGR frame. */
int hpe_render(hpe_renderer* r, const float* verts_dev, const float* cam_dev, int B, int H, int W, const unsigned char* bg_dev,
               const HpeRenderParams* p, unsigned char* out_dev, void* stream);

/* -- test / measurement hooks -------------------------------------------------------------------- */
/* Renderer internals: face_dev [B,H,W] int32 winning face per pixel (-1 where uncovered) and z_dev [B,H,W] float its depth
 * z_pix (0 where uncovered); arguments as hpe_render. */
int hpe_debug_render_ids(hpe_renderer* r, const float* verts_dev, const float* cam_dev, int B, int H, int W, const HpeRenderParams* p,
                         int* face_dev, float* z_dev, void* stream);
/* the vertex records of hpe_render: rec_dev [B,P] of 8 x 4 bytes {int U, int V, int valid, int 0, float 1/z, float r, g, b}
 * with U = rint(256 u), V = rint(256 v) (projected pixel coordinates in 1/256 px); H and W only serve the default camera. */
int hpe_debug_render_vertices(hpe_renderer* r, const float* verts_dev, const float* cam_dev, int B, int H, int W, const HpeRenderParams* p,
                              void* rec_dev, void* stream);

/* Run loaded conv layer `idx` (+BN, optional residual, optional ReLU) on x_dev [B,Hin,Hin,Cin] ->
 * y_dev [B,Hout,Hout,Cout]; for idx 0 the input is the raw [B,224,224,3] image and y is the
 * post-ReLU conv1 output [B,112,112,64].  On a bf16 context (idx > 0 only) x / residual are rounded to bf16 on the way in, the
 * layer runs through the bf16 kernel the plan picks for this batch, and y is its bf16 output widened to float. */
int hpe_debug_conv(hpe_ctx* ctx, int idx, const float* x_dev, int B, const float* residual_dev, int relu, float* y_dev,
                   void* stream);
/* bf16 contexts: the chained launch of conv_chain_bf16.hip alone.  idx2c = res{2,3}{b..}_branch2c of a block that is followed by an
 * identity block: t2_dev [B,H,H,C], residual_dev [B,H,H,4C] (rounded to bf16 on the way in) -> t3_dev [B,H,H,4C] =
 * relu(bn(conv2c(t2)) + residual) and u1_dev [B,H,H,C] = relu(bn(conv2a_next(t3))), both widened to float.  idx2c = res2a_branch2c: the
 * conv_block form, residual_dev is the block INPUT [B,56,56,64] and t3 = relu(bn(conv2c(t2)) + bn(conv1(input))).  occupancy (host,
 * optional, 3 ints): resident workgroups per CU of the three instantiations (the design needs 2).  fp32 contexts: idx2c = res2b_branch2c
 * only (conv_chain_f32.hip), operands in fp32, occupancy[0] = that kernel's. */
int hpe_debug_chain(hpe_ctx* ctx, int idx2c, const float* t2_dev, const float* residual_dev, int B, float* t3_dev, float* u1_dev,
                    int* occupancy, void* stream);
/* The fused stem kernel alone (conv1_pad + conv1 + bn_conv1 + ReLU + pool1_pad + MaxPooling2D(3,2) of the Keras ResNet50,
 * src/models.py:39): images_dev [B,224,224,3] -> y_dev [B,56,56,64].  rows_per_strip: pooled rows per workgroup
 * (1, 2, 4, 7 or 8; 0 = the default for this batch).  fp32 contexts only. */
int hpe_debug_stem(hpe_ctx* ctx, const float* images_dev, int B, int rows_per_strip, float* y_dev, void* stream);
/* The fp32 implicit-GEMM kernel (conv_gemm.hip) with every launch argument in the caller's hands:
 *   y[m][n] = act((sum_k A[m][k] * wt[n][k]) * scale[n] + shift[n] (+ residual[m][n]))
 * mode picks how row m of A is gathered:
 *   HPE_GEMM_DENSE    x [M][lda];
 *   HPE_GEMM_STRIDED  x NHWC [B][Hi][Wi][Cin], row m = pixel (b, ho * stride, wo * stride) of the Ho x Wo output map, K = Cin;
 *   HPE_GEMM_CONV3    x NHWC [B][Hi][Wi][Cin], 3x3 / stride 1 / SAME (Ho = Hi, Wo = Wi), K = 9 * Cin, k = (kh * 3 + kw) * Cin + ci;
 *   HPE_GEMM_DUAL     k-slabs (of 32) [0, k1_slabs) from the dense x [M][lda], the rest from the strided x2 (Cin = K - 32 * k1_slabs).
 * tile: 0 = 128x128, 1 = 128x64, 2 = 64x64, 3 = 64x128 (4 waves; these may split K), 4 = 128x128, 5 = 128x64, 6 = 256x128 (8 waves).
 * wt: w_rows rows of pitch ldw, w_rows >= N rounded up to the tile width, zero padded.  scale / shift NULL: ones / zeros (N <= 1024).
 * y_slab8: y is written channel-slab major, y[(n / 8) * M + m][n % 8].  use_splitk: the launcher is handed the context's split-K
 * workspace (it then cuts K on small grids of the 4-wave tiles), else none.  split_k (host, optional) receives the number of K slices the
 * launcher chose (1 = not split).  Every argument goes through the launcher's host-side contract: a rejected one returns
 * HPE_ERR_INVALID with the name of the broken clause in hpe_last_error(), launches nothing and sets *split_k to 0.  All device
 * pointers 16-byte aligned; all pitches multiples of 4 floats. */
#define HPE_GEMM_DENSE 0
#define HPE_GEMM_STRIDED 1
#define HPE_GEMM_CONV3 2
#define HPE_GEMM_DUAL 4
typedef struct HpeDebugGemm {
    int struct_size; /* sizeof(HpeDebugGemm), written by the caller and checked by the call */
    int mode;
    int tile;
    int M, N, K;
    int lda, ldw, ldy, ldres, w_rows;
    int relu;
    int Hi, Wi, Cin, Ho, Wo, stride;
    int k1_slabs;
    int y_slab8;
    int use_splitk;
    int reserved; /* 0 */
    const float* x;
    const float* x2;
    const float* wt;
    const float* residual;
    const float* scale;
    const float* shift;
    float* y;
    int* split_k;
} HpeDebugGemm;
int hpe_debug_gemm_ex(hpe_ctx* ctx, const HpeDebugGemm* g, void* stream);
/* The host-side contract alone, of any of the four implicit-GEMM launchers: kernel 0 = fp32 (the one hpe_debug_gemm_ex launches),
 * 1 = fp32 on the bf16 matrix cores (split weights; tiles 0, 4, 6; w_piece = element offset between the three pieces of a weight row,
 * read for this kernel only), 2 = bf16 (tiles 0..6; K and Cin in slabs of 64, pitches multiples of 8 elements), 3 = bf16 256x256
 * (tile 7).  No context, no HIP call, nothing is launched: the pointers of g are taken as numbers (NULL or not, aligned or not) and
 * never dereferenced; scale, shift and the library's zero page count as present; use_splitk is ignored.  HPE_OK if the launch is
 * inside the contract, else HPE_ERR_INVALID with the name of the first broken clause in hpe_last_error(). */
int hpe_debug_gemm_check(const HpeDebugGemm* g, int kernel, int w_piece);
/* The launching twin of hpe_debug_gemm_check: the launch g on kernel 0..3 as numbered there (w_piece read for kernel 1 only).
 * Kernel 0 is hpe_debug_gemm_ex.  Kernel 1 (f32s): x, x2, residual, y in fp32 as for kernel 0, wt points at bf16 data -- the three
 * pieces of Wt[n][k] at wt + n * ldw + j * w_piece + k, j = 0..2, ldw and w_piece in bf16 elements.  Kernels 2 and 3: x, x2, wt,
 * residual and y all point at bf16 data, every pitch and offset is in bf16 elements, k-slabs are 64 wide (HPE_GEMM_DUAL: Cin = K -
 * 64 * k1_slabs), y_slab8 is ignored; scale and shift stay fp32.  scale / shift NULL (N <= 1024), the zero page and, with
 * use_splitk, the split-K workspace come from the context.  The contract is checked before the context is looked at: a broken clause
 * returns HPE_ERR_INVALID with its name in hpe_last_error() whatever ctx is, launches nothing and sets *split_k to 0.  *split_k
 * receives what the launcher chose: kernel 3 may cut K when handed the workspace, kernels 1 and 2 always report 1. */
int hpe_debug_gemm_launch(hpe_ctx* ctx, const HpeDebugGemm* g, int kernel, int w_piece, void* stream);
/* Which kernel conv layer idx takes, asked of the plan alone: cfg is resolved as hpe_create / hpe_finalize resolve it (fields >= 0, else the
 * environment, else the defaults of cfg->encoder_dtype), then the library's one routing function is asked.  No context, no GPU, no HIP
 * call.  B images; concurrent: the launch is a batch chunk running beside others (no split-K, the concurrent tile rules); residual: the
 * launch has a residual operand; workspace: it has a slice of the Winograd V workspace (false for a chunk that starts past image 0 with
 * fewer than 32 images).  out->kernel / mode / tile / in_slab8 are what hpe_debug_conv launches under that query (in_slab8: the kernel
 * reads channel-slab major input, hpe_debug_conv converts); out_slab8: idx is a branch2a whose block's 3x3 layer makes it write
 * channel-slab major in the network.  For a branch2c, join says how its block ends in the network: 0 = launches of their own (branch1 of
 * a conv_block first, then the layer as out->kernel says when asked with residual = 1), 1 = the dual-source GEMM, whose kernel and tile are
 * join_kernel / join_tile, 2 = chained with the next block's branch2a (hpe_debug_chain), whose output is channel-slab major if
 * next_slab8.  packs: bit (1 << HPE_PACK_*) for each of W_SPLIT, WINO_U, WINO4_U, STEM_W, W_DUAL, W_DUAL_SPLIT that hpe_finalize packs for
 * the layer.  HPE_ERR_INVALID on a wrong struct_size (of cfg or out), idx outside [0, HPE_NUM_CONV) or B < 1. */
enum {
    HPE_CONV_K_F32 = 0,      /* conv_gemm.hip */
    HPE_CONV_K_F32S,         /* conv_gemm_f32s.hip (f32_split) */
    HPE_CONV_K_BF16,         /* conv_gemm_bf16.hip */
    HPE_CONV_K_BF16_P8,      /* conv_gemm_bf16_p8.hip (bf16_p8) */
    HPE_CONV_K_HALO3,        /* conv3_halo_bf16.hip */
    HPE_CONV_K_WINO,         /* F(2x2,3x3) through the V workspace */
    HPE_CONV_K_WINO_FUSED,   /* F(2x2,3x3), input transform inside the GEMM */
    HPE_CONV_K_WINO4,        /* F(4x4,3x3) through the V workspace */
    HPE_CONV_K_WINO4_FUSED,  /* F(4x4,3x3), input transform inside the GEMM (wino4_fused) */
    HPE_CONV_K_COUNT
};
typedef struct HpeConvRoute {
    int struct_size; /* sizeof(HpeConvRoute), written by the caller and checked by the call */
    int kernel;      /* HPE_CONV_K_* */
    int mode;        /* HPE_GEMM_*; 3 = conv1 as the im2col stem GEMM */
    int tile;        /* as HpeDebugGemm.tile, 7 = 256x256 (bf16_p8); -1: the kernel has no tile table */
    int in_slab8, out_slab8;
    int join, join_kernel, join_tile, next_slab8; /* branch2c only; else 0, -1, -1, 0 */
    unsigned packs;
    int reserved; /* 0 */
} HpeConvRoute;
int hpe_debug_conv_route(const HpeConfig* cfg, int idx, int B, int concurrent, int residual, int workspace, HpeConvRoute* out);
/* The weight-resident streaming kernel (conv_stream_f32s.hip) stands beside the routes above: it takes the identity-block expand layers with
 * K <= 128 that are launches of their own (res2c_branch2c, res3{b,c,d}_branch2c; fp32 contexts with f32_split != 0, HPE_STREAM1X1) from
 * HPE_STREAM1X1_MIN_M rows on, and hpe_debug_conv_route then still names the GEMM the launch takes without it.  Asked of the plan alone, as
 * hpe_debug_conv_route: bit 0 = this launch runs on the streaming kernel, bit 1 = the layer is one of its layers (hpe_finalize keeps the
 * split weights it reads); -1 with hpe_last_error() set for a bad argument.  For res2a_branch2c the answer is about its block's dual-source
 * launch (value 2 of HPE_STREAM1X1).  The chained forms of that kernel (values 4 and 8 of HPE_STREAM1X1: a stage-2 join and the next
 * block's branch2a as one launch of conv_stream_chain_f32s.hip, hpe_debug_stream_chain below) are taken by the inference walk alone and
 * change neither this answer nor hpe_debug_conv_route's. */
int hpe_debug_conv_stream1x1(const HpeConfig* cfg, int idx, int B, int concurrent, int residual);
/* The dual-source launch of a conv_block alone (fp32 contexts): y [B,ho,ho,cout] = relu(bn2c(W2c . t2) + bn1(W1 . x at the shortcut's stride)),
 * t2_dev [B,ho,ho,cin of idx2c] the branch2b output, x_dev [B,hi,hi,cin of branch1] the block input, through the kernel the plan routes
 * that launch to at batch B.  HPE_ERR_INVALID unless idx2c is the branch2c of a conv_block joined as the dual-source GEMM. */
int hpe_debug_dual(hpe_ctx* ctx, int idx2c, const float* t2_dev, const float* x_dev, int B, float* y_dev, void* stream);
/* The chained streaming launch of conv_stream_chain_f32s.hip alone (fp32 contexts), whatever HPE_STREAM1X1 says.  idx2c = res2b_branch2c:
 * t3 [B,56,56,256] = relu(bn(conv2c(t2)) + x) with x_dev the residual [B,56,56,256]; idx2c = res2a_branch2c: t3 = relu(bn(conv2c(t2)) +
 * bn(conv1(x))) with x_dev the block input [B,56,56,64]; both: u1 = relu(bn(conv2a_next(t3))), [B,56,56,64] row-major, or channel-slab
 * major u1[(n / 8) * M + m][n % 8] when slab8 != 0.  rows: 0 = all M = B * 56 * 56 rows, else the launch is asked for the first `rows`
 * rows of the batch (slab8 then counts M = rows).  The launcher takes whole 32-row tiles only: HPE_ERR_INVALID, and nothing is launched,
 * for any other row count, for rows past the batch and for any idx2c but these two. */
int hpe_debug_stream_chain(hpe_ctx* ctx, int idx2c, const float* t2_dev, const float* x_dev, int B, float* t3_dev, float* u1_dev, int slab8,
                           int rows, void* stream);
/* The dense mode of hpe_debug_gemm_ex with scale = ones, shift = zeros, lda = ldw = K, ldy = ldres = N and no split-K
 * workspace: y[M,N] = act(x[M,K] . wt[n][k]^T (+ residual)); K % 32 == 0; N <= 1024; tile 0..6 as above.  Needs the regressor loaded. */
int hpe_debug_gemm(hpe_ctx* ctx, const float* x_dev, const float* wt_dev, int M, int N, int K, int w_rows, int tile,
                   const float* residual_dev, int relu, float* y_dev, void* stream);
/* ZeroPad(1)+MaxPool3x3/2: x [B,H,H,C] -> y [B,H/2,H/2,C];  global average pool x [B,HW,C] -> y [B,C] */
int hpe_debug_maxpool(const float* x_dev, int B, int H, int C, float* y_dev, void* stream);
int hpe_debug_avgpool(const float* x_dev, int B, int HW, int C, float* y_dev, void* stream);
/* generic regressor: out[n,k,c] = sum_v X[n,v,c] * reg[v,k]  (the 6890 -> K joint regressor kernel) */
int hpe_debug_joint_regress(hpe_ctx* ctx, const float* X_dev, int n, int use_kp_regressor, float* out_dev, void* stream);
/* Timing: level 1 brackets the phases of hpe_forward / hpe_encoder with HIP events recorded on `stream`;
 * level 2 additionally brackets every conv launch (adds ~100 event records per call).
 * hpe_get_timings synchronises on the last event and returns milliseconds of the LAST call:
 *   ms[0] encoder (pad + 53 convs + pools), ms[1] sum over the 53 conv launches (level 2, else 0),
 *   ms[2] regressor + SMPL stages, ms[3] reserved (0), ms[4] whole call. */
int hpe_enable_timing(hpe_ctx* ctx, int level);
/* Synchronises `stream` and reports the ctx's device error word: HPE_ERR_HIP if a kernel flagged an invalid result since
 * the last check (today only the opt-in HPE_WINO_STREAMK path can: a bounded inter-workgroup wait that timed out). */
int hpe_device_status(hpe_ctx* ctx, void* stream);
int hpe_get_timings(hpe_ctx* ctx, float ms[5]);
/* Encoder span (first launch to last completion on `stream`, HIP events) over ALL timed hpe_forward* / hpe_encoder calls since
 * hpe_enable_timing (the last 64 at most): ms[0] mean, ms[1] min, ms[2] max; *n_calls = calls averaged.  Synchronises. */
int hpe_get_span_stats(hpe_ctx* ctx, float ms[3], int* n_calls);
/* last timed hpe_val_losses call: ms[0] = whole call, ms[1] = sum over the stages of the pixel -> nearest-vertex search
 * (nn_a2b_mfma_kernel, the dominant kernel of the mesh loss) */
int hpe_get_loss_timings(hpe_ctx* ctx, float ms[2]);
/* Work counter of the pixel -> vertex search: while counter_dev (device, 2 x u64, caller-zeroed) is set, every hpe_val_losses /
 * hpe_mesh_loss call adds the v_mfma_f32_32x32x2_f32 instructions it issues (1024 (pixel, vertex) pairs each) to
 * counter_dev[0] (cell-grid search) and counter_dev[1] (full search).  NULL disables (the default). */
int hpe_debug_set_loss_counter(hpe_ctx* ctx, void* counter_dev);
/* per-conv-layer milliseconds of the last level-2 timed call: ms53[HPE_NUM_CONV] */
int hpe_get_conv_timings(hpe_ctx* ctx, float* ms53);

#ifdef __cplusplus
}
#endif
#endif /* HPE_H_ */
