"""The 3-D supervision losses (include/hpe_loss3d.h: hpe_loss3d, hpe_loss3d_backward; DESIGN.md "3-D supervision") restated in torch, dtype-parametric:
float64 is the reference of tests/test_gpu_loss3d.py, and the same functions in float32 set its bar.  The flip is written on its own, as a
gather by the index lists below and a product with M = diag(-1, 1, 1); gradients come from torch.autograd.  Inputs are float32 values in
either dtype (numpy arrays or tensors); a row whose weight is 0 is left out by selecting the other rows, so its labels are never touched."""
import numpy as np
import torch

SWAP14 = [5, 4, 3, 2, 1, 0, 11, 10, 9, 8, 7, 6, 12, 13]
PERM24 = [0, 2, 1, 3, 5, 4, 6, 8, 7, 9, 11, 10, 12, 14, 13, 15, 17, 16, 19, 18, 21, 20, 23, 22]


def random_case(seed, B=4, K=19):
    """one stage's predictions and a ground truth as float32 numpy arrays, keyed by ``run``'s argument names; weights in [0.5, 1.5),
    rows 0 and 1 flipped and not"""
    g = np.random.RandomState(seed)
    f32 = lambda a: a.astype(np.float32)  # noqa: E731
    case = dict(joints=f32(g.randn(B, K, 3)), betas=f32(g.randn(B, 10)), Rs=f32(g.randn(B, 24, 3, 3)), joints_gt=f32(g.randn(B, 14, 3)),
                Rs_gt=f32(g.randn(B, 24, 3, 3)), shape_gt=f32(g.randn(B, 10)), w_joints=f32(g.rand(B) + 0.5), w_smpl=f32(g.rand(B) + 0.5),
                flip=g.rand(B) < 0.5)
    case["flip"][:2] = (True, False)[:B]
    return case


def _t(x, dtype):
    return None if x is None else torch.as_tensor(np.asarray(x)).to(dtype)


def mirror_gt(joints_gt, Rs_gt, flip):
    """the ground truth of the flipped rows mirrored about the x axis: g'[k] = M g[SWAP14[k]], R'[j] = M R[PERM24[j]] M"""
    M = torch.diag(torch.tensor([-1.0, 1.0, 1.0], dtype=joints_gt.dtype))
    f = torch.as_tensor(np.asarray(flip).astype(bool)) if flip is not None else torch.zeros(joints_gt.shape[0], dtype=torch.bool)
    gj = torch.where(f[:, None, None], joints_gt[:, SWAP14] @ M, joints_gt)
    gR = torch.where(f[:, None, None, None], M @ Rs_gt[:, PERM24] @ M, Rs_gt)
    return gj, gR


def per_row(joints, betas, Rs, joints_gt, Rs_gt, shape_gt, w_joints, w_smpl, flip):
    """-> the unweighted sums of squares [B,3] (joints, rotations, shape), 0 where the term's weight is 0 (the labels of such a row
    are replaced before any arithmetic: NaN there reaches nothing)"""
    sj_on, ss_on = (w_joints != 0), (w_smpl != 0)
    gj, gR = mirror_gt(torch.where(sj_on[:, None, None], joints_gt, torch.zeros_like(joints_gt)),
                       torch.where(ss_on[:, None, None, None], Rs_gt, torch.zeros_like(Rs_gt)), flip)
    gs = torch.where(ss_on[:, None], shape_gt, torch.zeros_like(shape_gt))
    p = joints[:, :14]
    e = (p - 0.5 * (p[:, 2:3] + p[:, 3:4])) - (gj - 0.5 * (gj[:, 2:3] + gj[:, 3:4]))
    zero = torch.zeros((), dtype=joints.dtype)
    sj = torch.where(sj_on, (e * e).sum((1, 2)), zero)
    sp = torch.where(ss_on, ((Rs - gR) ** 2).sum((1, 2, 3)), zero)
    ss = torch.where(ss_on, ((betas - gs) ** 2).sum(1), zero)
    return torch.stack([sj, sp, ss], 1)


def parts_of(per, w_joints, w_smpl):
    """-> [5] = num_j, num_pose, num_shape, cnt_j, cnt_s"""
    on_j, on_s = (w_joints != 0), (w_smpl != 0)
    wj, ws = torch.where(on_j, w_joints, torch.zeros_like(w_joints)), torch.where(on_s, w_smpl, torch.zeros_like(w_smpl))
    return torch.stack([(wj * per[:, 0]).sum(), (ws * per[:, 1]).sum(), (ws * per[:, 2]).sum(), 42.0 * on_j.sum().to(per.dtype),
                        226.0 * on_s.sum().to(per.dtype)])


def losses_of(parts, counts=None):
    """(L_joints, L_smpl) from one stage's parts; counts: the (cnt_j, cnt_s) to divide by (None: the parts' own); 0 where a count is 0"""
    cj, cs = (parts[3], parts[4]) if counts is None else (counts[0], counts[1])
    zero = torch.zeros((), dtype=parts.dtype)
    return (0.5 * parts[0] / cj if cj > 0 else zero * parts[0]), (0.5 * (parts[1] + parts[2]) / cs if cs > 0 else zero * parts[1])


def run(joints, betas, Rs, joints_gt, Rs_gt, shape_gt, w_joints, w_smpl, flip=None, scale_j=None, scale_s=None, dtype=torch.float64):
    """One stage: -> dict(parts [5], per_image [B,3], grad_joints [B,K,3], grad_Rs, grad_betas) as numpy float64.  The gradients are
    those of scale_j * num_j + scale_s * (num_pose + num_shape) by autograd, which is what hpe_loss3d_backward defines (scale = grad_loss
    * 0.5 / count; default 1): the hip term of the joint gradient comes out of the alignment by itself."""
    j, b, R = (_t(x, dtype).clone().requires_grad_(True) for x in (joints, betas, Rs))
    gj, gR, gs, wj, ws = (_t(x, dtype) for x in (joints_gt, Rs_gt, shape_gt, w_joints, w_smpl))
    per = per_row(j, b, R, gj, gR, gs, wj, ws, flip)
    parts = parts_of(per, wj, ws)
    sj = _t(1.0 if scale_j is None else scale_j, dtype)
    ss = _t(1.0 if scale_s is None else scale_s, dtype)
    (sj * parts[0] + ss * (parts[1] + parts[2])).backward()
    out = {"parts": parts, "per_image": per, "grad_joints": j.grad, "grad_Rs": R.grad, "grad_betas": b.grad}
    return {k: v.detach().to(torch.float64).numpy() for k, v in out.items()}


def bar(got, ref32, ref64, what=""):
    """the project's convention: max |got - ref64| <= 4 * max(max |ref32 - ref64|, 2^-22 * max |ref64|).  -> (error, allowed), printed"""
    got, ref32, ref64 = (np.asarray(a, np.float64) for a in (got, ref32, ref64))
    err = float(np.abs(got - ref64).max()) if got.size else 0.0
    own = float(np.abs(ref32 - ref64).max()) if got.size else 0.0
    floor = 2.0 ** -22 * (float(np.abs(ref64).max()) if got.size else 0.0)
    allowed = 4.0 * max(own, floor)
    print("loss3d %s: |out - ref64| %.3g, float32 reference %.3g, floor %.3g, ratio to the bar %.3g" % (what, err, own, floor, err / allowed if allowed > 0 else 0.0))
    return err, allowed
