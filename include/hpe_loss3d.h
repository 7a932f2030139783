/* hpe_loss3d.h -- the 3-D supervision extension of the C ABI of hpe.h (which includes this header; it may also be included on its own).
 * Same conventions: plain C, device pointers + sizes, int return codes (HPE_OK == 0), the message of a failure from hpe_last_error(). */
#ifndef HPE_LOSS3D_H_
#define HPE_LOSS3D_H_

#ifdef __cplusplus
extern "C" {
#endif

/* The 3-D supervision terms of the generator step (DESIGN.md "3-D supervision"; restated in float64 by tests/loss3d_ref.py): an L2 loss on
 * pelvis-aligned joints and an L2 loss on the 24 joint rotations and the 10 shape coefficients, for all n_stage IEF stages in ONE launch.
 * Predictions, host arrays of n_stage device pointers: joints_dev[s] [B,K,3] with 14 <= K <= HPE_MAX_KP (the first 14 joints are read),
 * Rs_dev[s] [B,24,3,3] as HpeOutputs.Rs (the root is included), betas_dev[s] 10 floats per row, betas_stride (>= 10) floats apart
 * (theta + 75 with stride 85 works in place).  Ground truth, shared by the stages: joints_gt_dev [B,14,3], Rs_gt_dev [B,24,3,3] (matrices,
 * hpe_smpl's Rs of the ground-truth theta: no Rodrigues happens here, so a prediction equal to its ground truth gives exactly 0),
 * shape_gt_dev [B,10], the row weights w_joints_dev [B] and w_smpl_dev [B], and flip_dev [B] uint8 (NULL: no row is flipped).
 * A row whose weight is 0 is NOT READ for that term: NaN or garbage in its labels or predictions reaches no output.
 * A flipped row is compared with its ground truth mirrored about the x axis (the labels are stored unflipped; flip is the augmentation's
 * draw): joints g'[k] = (-x, y, z) of g[SWAP14[k]], SWAP14 = 5 4 3 2 1 0 11 10 9 8 7 6 12 13; rotations R'[j] = M R[PERM24[j]] M with
 * M = diag(-1, 1, 1), which negates the entries (0,1), (0,2), (1,0), (2,0), PERM24 = 0 2 1 3 5 4 6 8 7 9 11 10 12 14 13 15 17 16 19 18
 * 21 20 23 22; the shape is unchanged.  A permutation and sign changes: exact.
 * With the pelvis the midpoint of joints 2 and 3 (the hips) of each skeleton and e_ik = (p_ik - pelvis(p_i)) - (g'_ik - pelvis(g'_i)):
 *   num_j = sum_i w_joints_i sum_{k<14} |e_ik|^2                 cnt_j = 42 * #{i : w_joints_i != 0}
 *   num_pose = sum_i w_smpl_i sum_{j<24} |Rs_ij - R'_ij|_F^2      num_shape = sum_i w_smpl_i |betas_i - shape_i|^2
 *   cnt_s = 226 * #{i : w_smpl_i != 0}
 *   L_joints = 0.5 num_j / cnt_j,  L_smpl = 0.5 (num_pose + num_shape) / cnt_s, each 0 where its count is 0 (SUM_BY_NONZERO_WEIGHTS).
 * parts_dev [n_stage][5] = num_j, num_pose, num_shape, cnt_j, cnt_s: numerators and counts apart, as hpe_kp_loss returns them, so that
 * ranks can all-reduce before dividing.  per_image_dev [n_stage][B][3] or NULL: the unweighted sums of squares of each row (joints,
 * rotations, shape), 0 for a term whose weight is 0.
 * Stateless like hpe_pose3d_scores: no context, no workspace, no allocation, no synchronisation, no atomics, capturable.  Every sum is
 * float64 in an order fixed by the launch shape alone, the outputs are float32: the same inputs give the same bits.  HPE_ERR_INVALID with
 * a message, before any HIP call, for a NULL pointer (flip_dev and per_image_dev excepted) or a NULL entry, n_stage outside [1, 16],
 * B < 1, K outside [14, HPE_MAX_KP], betas_stride < 10. */
int hpe_loss3d(const float* const* joints_dev, const float* const* Rs_dev, const float* const* betas_dev, int betas_stride,
               const float* joints_gt_dev, const float* Rs_gt_dev, const float* shape_gt_dev, const float* w_joints_dev, const float* w_smpl_dev,
               const unsigned char* flip_dev, int n_stage, int B, int K, float* parts_dev, float* per_image_dev, void* stream);
/* Gradient of hpe_loss3d's two losses with respect to the predictions of every stage.  scale_j_dev [n_stage] and scale_s_dev [n_stage]:
 * device floats the caller forms as grad_loss * 0.5 / count with the local or the global count (0 where the count is 0); nothing reads
 * the device.  Outputs, host arrays of n_stage device pointers, any of the three arrays may be NULL, not all:
 *   grad_joints_dev[s] [B,K,3] = 2 scale_j w_joints_i (e_ik - [k in {2, 3}] 0.5 sum_m e_im) for k < 14, zeros for 14 .. K-1; the hip
 *     term is the derivative of the pelvis alignment;
 *   grad_Rs_dev[s] [B,24,3,3] = 2 scale_s w_smpl_i (Rs - R');  grad_betas_dev[s] [B,10] dense = 2 scale_s w_smpl_i (betas - shape).
 * A row whose weight is 0 gets exact zeros and is not read.  One launch, one wave per (row, stage): a row's gradient depends neither on
 * B nor on the row's position.  Rules and error codes as hpe_loss3d; scale_j_dev is needed with grad_joints_dev, scale_s_dev with either
 * of the other two. */
int hpe_loss3d_backward(const float* const* joints_dev, const float* const* Rs_dev, const float* const* betas_dev, int betas_stride,
                        const float* joints_gt_dev, const float* Rs_gt_dev, const float* shape_gt_dev, const float* w_joints_dev,
                        const float* w_smpl_dev, const unsigned char* flip_dev, int n_stage, int B, int K, const float* scale_j_dev,
                        const float* scale_s_dev, float* const* grad_joints_dev, float* const* grad_Rs_dev, float* const* grad_betas_dev,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HPE_LOSS3D_H_ */
