// loss3d.hip -- the 3-D supervision terms of the generator step (DESIGN.md "3-D supervision"): an L2 loss on pelvis-aligned joints and an
// L2 loss on the 24 joint rotations and the 10 shape coefficients, both masked per row, with their gradient to the predictions.
//   hpe_loss3d           one launch, one workgroup of 16 waves per IEF stage.  Wave w takes rows w, w + 16, ...: 42 lanes hold the joint
//                        residuals, the 216 rotation entries go four to a lane, 10 lanes hold the shape.  A row's three sums of squares are
//                        added across the wave by shuffles; lane 0 keeps the wave's weighted sums over its rows, the waves' sums meet in LDS
//                        and five threads add them in wave order.
//   hpe_loss3d_backward  one launch, one wave per (row, stage); the hip term of the joint gradient needs the sum of a row's residuals per
//                        axis, which every lane gathers by shuffles in joint order.
// A flipped row reads its ground truth mirrored about the x axis: a permutation of joints and sign changes, so nothing is rounded.  A row
// whose weight is 0 is not read for that term.  Everything between the float32 loads and the float32 stores is double, in an order fixed
// by the launch shape alone: no atomics, the same inputs give the same bits.
#include <hip/hip_runtime.h>

#include <string>

#include "hpe_ctx.h"

namespace {

constexpr int kMaxStage = 16;
constexpr int kJoints = 14;        // the joints the loss reads
constexpr int kJointFloats = 42;
constexpr int kRotFloats = 216;    // 24 joints x 3 x 3
constexpr int kShape = 10;
constexpr int kFwdWaves = 16;
constexpr int kFwdThreads = 64 * kFwdWaves;
constexpr int kParts = 5;          // num_j, num_pose, num_shape, cnt_j, cnt_s

// the left/right swap of the 14 LSP joints (the first 14 of flip_image's swap_inds) and of the 24 SMPL joints
__constant__ unsigned char kSwap14[kJoints] = {5, 4, 3, 2, 1, 0, 11, 10, 9, 8, 7, 6, 12, 13};
__constant__ unsigned char kPerm24[24] = {0, 2, 1, 3, 5, 4, 6, 8, 7, 9, 11, 10, 12, 14, 13, 15, 17, 16, 19, 18, 21, 20, 23, 22};

struct Loss3dArgs {
    const float* joints[kMaxStage];
    const float* Rs[kMaxStage];
    const float* betas[kMaxStage];
    float* grad_joints[kMaxStage];
    float* grad_Rs[kMaxStage];
    float* grad_betas[kMaxStage];
    const float* joints_gt;
    const float* Rs_gt;
    const float* shape_gt;
    const float* w_joints;
    const float* w_smpl;
    const unsigned char* flip;
    const float* scale_j;
    const float* scale_s;
    float* parts;
    float* per_image;
    int n_stage, B, K, betas_stride, want_gj, want_gR, want_gb;
};

// component c = 3 k + a of the (mirrored, where flipped) ground-truth joints of one row
__device__ __forceinline__ double gt_joint(const float* G, int c, bool flipped) {
    const int k = c / 3, a = c - 3 * k;
    if (!flipped) return (double)G[c];
    const double g = (double)G[3 * kSwap14[k] + a];
    return a == 0 ? -g : g;
}

// entry c = 9 j + e of the (mirrored) ground-truth rotations of one row: M R[perm[j]] M negates (0,1), (0,2), (1,0), (2,0)
__device__ __forceinline__ double gt_rot(const float* R, int c, bool flipped) {
    if (!flipped) return (double)R[c];
    const int j = c / 9, e = c - 9 * j;
    const double r = (double)R[9 * kPerm24[j] + e];
    return (e == 1 || e == 2 || e == 3 || e == 6) ? -r : r;
}

// the pelvis-aligned residual of component c < 42 of one row: (p - pelvis(p)) - (g - pelvis(g)), the pelvis the midpoint of joints 2 and 3
__device__ __forceinline__ double joint_residual(const float* P, const float* G, int c, bool flipped) {
#pragma clang fp contract(off)
    const int a = c % 3;
    const double pbar = 0.5 * ((double)P[6 + a] + (double)P[9 + a]);
    const double gbar = 0.5 * (gt_joint(G, 6 + a, flipped) + gt_joint(G, 9 + a, flipped));
    return ((double)P[c] - pbar) - (gt_joint(G, c, flipped) - gbar);
}

__device__ __forceinline__ double wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;  // lane 0 holds the sum
}

__global__ __launch_bounds__(kFwdThreads) void loss3d_kernel(Loss3dArgs a) {
#pragma clang fp contract(off)
    __shared__ double part[kFwdWaves][kParts];
    const int st = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    double acc[kParts] = {0.0, 0.0, 0.0, 0.0, 0.0};  // lane 0's are the wave's
    for (int i = wave; i < a.B; i += kFwdWaves) {
        const float wj = a.w_joints[i], ws = a.w_smpl[i];
        const bool flipped = a.flip && a.flip[i] != 0;
        double sj = 0.0, sp = 0.0, ss = 0.0;
        if (wj != 0.f) {
            if (lane < kJointFloats) {
                const double e = joint_residual(a.joints[st] + (size_t)i * a.K * 3, a.joints_gt + (size_t)i * kJointFloats, lane, flipped);
                sj = e * e;
            }
            sj = wave_sum(sj);
        }
        if (ws != 0.f) {
            const float* R = a.Rs[st] + (size_t)i * kRotFloats;
            const float* G = a.Rs_gt + (size_t)i * kRotFloats;
            for (int c = lane; c < kRotFloats; c += 64) {
                const double d = (double)R[c] - gt_rot(G, c, flipped);
                sp += d * d;
            }
            if (lane < kShape) {
                const double d = (double)a.betas[st][(size_t)i * a.betas_stride + lane] - (double)a.shape_gt[(size_t)i * kShape + lane];
                ss = d * d;
            }
            sp = wave_sum(sp);
            ss = wave_sum(ss);
        }
        if (lane == 0) {
            if (wj != 0.f) acc[0] += (double)wj * sj, acc[3] += 1.0;
            if (ws != 0.f) acc[1] += (double)ws * sp, acc[2] += (double)ws * ss, acc[4] += 1.0;
            if (a.per_image) {
                float* o = a.per_image + ((size_t)st * a.B + i) * 3;
                o[0] = (float)sj, o[1] = (float)sp, o[2] = (float)ss;
            }
        }
    }
    if (lane == 0)
        for (int p = 0; p < kParts; ++p) part[wave][p] = acc[p];
    __syncthreads();
    if (t < kParts) {
        double s = part[0][t];
        for (int w = 1; w < kFwdWaves; ++w) s += part[w][t];
        if (t == 3) s *= 42.0;
        if (t == 4) s *= 226.0;
        a.parts[(size_t)st * kParts + t] = (float)s;
    }
}

__global__ __launch_bounds__(64) void loss3d_backward_kernel(Loss3dArgs a) {
#pragma clang fp contract(off)
    const int i = blockIdx.x, st = blockIdx.y, lane = threadIdx.x;
    const float wj = a.w_joints[i], ws = a.w_smpl[i];
    const bool flipped = a.flip && a.flip[i] != 0;
    if (a.want_gj) {
        float* o = a.grad_joints[st] + (size_t)i * a.K * 3;
        const int n = a.K * 3;  // at most 72: two passes of the wave
        if (wj != 0.f) {
            double e = 0.0;
            if (lane < kJointFloats) e = joint_residual(a.joints[st] + (size_t)i * a.K * 3, a.joints_gt + (size_t)i * kJointFloats, lane, flipped);
            double sum = 0.0;  // of this lane's axis over the 14 joints, in joint order
            const int ax = lane % 3;
            for (int m = 0; m < kJoints; ++m) sum += __shfl(e, 3 * m + ax);
            const double f = 2.0 * (double)a.scale_j[st] * (double)wj;
            if (lane < kJointFloats) {
                const int k = lane / 3;
                const double g = (k == 2 || k == 3) ? e - 0.5 * sum : e;
                o[lane] = (float)(f * g);
            }
            for (int c = lane; c < n; c += 64)
                if (c >= kJointFloats) o[c] = 0.f;
        } else {
            for (int c = lane; c < n; c += 64) o[c] = 0.f;
        }
    }
    if (a.want_gR) {
        float* o = a.grad_Rs[st] + (size_t)i * kRotFloats;
        if (ws != 0.f) {
            const float* R = a.Rs[st] + (size_t)i * kRotFloats;
            const float* G = a.Rs_gt + (size_t)i * kRotFloats;
            const double f = 2.0 * (double)a.scale_s[st] * (double)ws;
            for (int c = lane; c < kRotFloats; c += 64) o[c] = (float)(f * ((double)R[c] - gt_rot(G, c, flipped)));
        } else {
            for (int c = lane; c < kRotFloats; c += 64) o[c] = 0.f;
        }
    }
    if (a.want_gb && lane < kShape) {
        float* o = a.grad_betas[st] + (size_t)i * kShape;
        if (ws != 0.f) {
            const double f = 2.0 * (double)a.scale_s[st] * (double)ws;
            o[lane] = (float)(f * ((double)a.betas[st][(size_t)i * a.betas_stride + lane] - (double)a.shape_gt[(size_t)i * kShape + lane]));
        } else {
            o[lane] = 0.f;
        }
    }
}

// the checks both calls share; fills the inputs of `a`.  Returns HPE_OK or the code fail() set
int check_inputs(const char* who, const float* const* joints, const float* const* Rs, const float* const* betas, int betas_stride,
                 const float* joints_gt, const float* Rs_gt, const float* shape_gt, const float* w_joints, const float* w_smpl,
                 const unsigned char* flip, int n_stage, int B, int K, Loss3dArgs& a) {
    const std::string me = std::string(who) + ": ";
    if (!joints || !Rs || !betas) return fail(HPE_ERR_INVALID, me + "joints_dev, Rs_dev or betas_dev is NULL");
    if (!joints_gt || !Rs_gt || !shape_gt) return fail(HPE_ERR_INVALID, me + "joints_gt_dev, Rs_gt_dev or shape_gt_dev is NULL");
    if (!w_joints || !w_smpl) return fail(HPE_ERR_INVALID, me + "w_joints_dev or w_smpl_dev is NULL");
    if (n_stage < 1 || n_stage > kMaxStage) return fail(HPE_ERR_INVALID, me + "n_stage " + std::to_string(n_stage) + " outside [1, 16]");
    if (B < 1) return fail(HPE_ERR_INVALID, me + "batch " + std::to_string(B) + " < 1");
    if (K < kJoints || K > HPE_MAX_KP)
        return fail(HPE_ERR_INVALID, me + "K " + std::to_string(K) + " outside [14, " + std::to_string(HPE_MAX_KP) + "]");
    if (betas_stride < kShape) return fail(HPE_ERR_INVALID, me + "betas_stride " + std::to_string(betas_stride) + " < 10");
    for (int s = 0; s < n_stage; ++s) {
        if (!joints[s] || !Rs[s] || !betas[s])
            return fail(HPE_ERR_INVALID, me + "joints_dev[" + std::to_string(s) + "], Rs_dev[" + std::to_string(s) + "] or betas_dev[" + std::to_string(s) + "] is NULL");
        a.joints[s] = joints[s], a.Rs[s] = Rs[s], a.betas[s] = betas[s];
    }
    a.joints_gt = joints_gt, a.Rs_gt = Rs_gt, a.shape_gt = shape_gt, a.w_joints = w_joints, a.w_smpl = w_smpl, a.flip = flip;
    a.n_stage = n_stage, a.B = B, a.K = K, a.betas_stride = betas_stride;
    return HPE_OK;
}

}  // namespace

#pragma GCC visibility push(default)
extern "C" int hpe_loss3d(const float* const* joints, const float* const* Rs, const float* const* betas, int betas_stride, const float* joints_gt,
                          const float* Rs_gt, const float* shape_gt, const float* w_joints, const float* w_smpl, const unsigned char* flip,
                          int n_stage, int B, int K, float* parts, float* per_image, void* stream) {
    Loss3dArgs a = {};
    if (int rc = check_inputs("hpe_loss3d", joints, Rs, betas, betas_stride, joints_gt, Rs_gt, shape_gt, w_joints, w_smpl, flip, n_stage, B, K, a))
        return rc;
    if (!parts) return fail(HPE_ERR_INVALID, "hpe_loss3d: parts_dev is NULL");
    a.parts = parts, a.per_image = per_image;
    hipLaunchKernelGGL(loss3d_kernel, dim3(n_stage), dim3(kFwdThreads), 0, static_cast<hipStream_t>(stream), a);
    HIP_TRY(hipGetLastError());
    return HPE_OK;
}

extern "C" int hpe_loss3d_backward(const float* const* joints, const float* const* Rs, const float* const* betas, int betas_stride,
                                   const float* joints_gt, const float* Rs_gt, const float* shape_gt, const float* w_joints, const float* w_smpl,
                                   const unsigned char* flip, int n_stage, int B, int K, const float* scale_j, const float* scale_s,
                                   float* const* grad_joints, float* const* grad_Rs, float* const* grad_betas, void* stream) {
    Loss3dArgs a = {};
    if (int rc = check_inputs("hpe_loss3d_backward", joints, Rs, betas, betas_stride, joints_gt, Rs_gt, shape_gt, w_joints, w_smpl, flip, n_stage,
                              B, K, a))
        return rc;
    if (!grad_joints && !grad_Rs && !grad_betas) return fail(HPE_ERR_INVALID, "hpe_loss3d_backward: every output is NULL, nothing to write");
    if (grad_joints && !scale_j) return fail(HPE_ERR_INVALID, "hpe_loss3d_backward: grad_joints_dev needs scale_j_dev");
    if ((grad_Rs || grad_betas) && !scale_s) return fail(HPE_ERR_INVALID, "hpe_loss3d_backward: grad_Rs_dev and grad_betas_dev need scale_s_dev");
    for (int s = 0; s < n_stage; ++s) {
        if ((grad_joints && !grad_joints[s]) || (grad_Rs && !grad_Rs[s]) || (grad_betas && !grad_betas[s]))
            return fail(HPE_ERR_INVALID, "hpe_loss3d_backward: an output pointer of stage " + std::to_string(s) + " is NULL");
        a.grad_joints[s] = grad_joints ? grad_joints[s] : nullptr;
        a.grad_Rs[s] = grad_Rs ? grad_Rs[s] : nullptr;
        a.grad_betas[s] = grad_betas ? grad_betas[s] : nullptr;
    }
    a.scale_j = scale_j, a.scale_s = scale_s;
    a.want_gj = grad_joints != nullptr, a.want_gR = grad_Rs != nullptr, a.want_gb = grad_betas != nullptr;
    hipLaunchKernelGGL(loss3d_backward_kernel, dim3(B, n_stage), dim3(64), 0, static_cast<hipStream_t>(stream), a);
    HIP_TRY(hipGetLastError());
    return HPE_OK;
}
#pragma GCC visibility pop
