"""torch.autograd glue of the HIP backward (include/hpe.h: hpe_smpl_backward, hpe_kp_loss_backward, hpe_mesh_loss_grad,
hpe_critic_backward, hpe_regressor_backward).  Used only when an input requires grad: ``HpeEngine.smpl`` / ``SMPL.__call__`` / ``kp_reprojection_loss`` /
``mesh_reprojection_loss`` / ``critic_scores`` keep their plain forward-only path otherwise.
Nothing numerical happens here -- forward and backward are one library call each."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from . import engine as _engine


class SmplFunction(torch.autograd.Function):
    """outputs = hpe_smpl(theta); every output is differentiable (cams and theta are pass-through copies of theta's columns)."""

    @staticmethod
    def forward(ctx, theta, engine, want):
        th = _engine._require_cuda_tensor(theta.detach(), "theta", (85,))
        B = th.shape[0]
        tensors, o = engine._alloc_outputs(B, want)
        _lib.check(engine.lib.hpe_smpl(engine._h, th.data_ptr(), B, C.byref(o), engine._stream()))
        ctx.engine, ctx.want = engine, want
        ctx.save_for_backward(th)
        return tuple(tensors[k] for k in want)

    @staticmethod
    def backward(ctx, *grad_outs):
        (th,) = ctx.saved_tensors
        grads = {k: g for k, g in zip(ctx.want, grad_outs) if g is not None}
        return ctx.engine.smpl_backward(th, grads), None, None


def smpl_with_grad(engine, theta, want):
    return dict(zip(want, SmplFunction.apply(theta, engine, want)))


class KpLossFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, kp_gt, kp_pred):
        ctx.save_for_backward(kp_gt.detach(), kp_pred.detach())
        return _engine.kp_loss_parts(kp_gt.detach(), kp_pred.detach())[2].clone()

    @staticmethod
    def backward(ctx, grad_loss):
        kp_gt, kp_pred = ctx.saved_tensors
        return None, _engine.kp_loss_backward(kp_gt, kp_pred, grad_loss.to(torch.float32))


class KpLossShareFunction(torch.autograd.Function):
    """One rank's share of kp_reprojection_loss over a batch spread across ranks: (this rank's sum of vis * |d|) / (2 * #visible of ALL
    ranks).  ``global_count``: that denominator as a one-element CUDA tensor, already summed over the ranks (``kp_visible_count`` and one
    all-reduce); the ranks' shares add up to the loss of the global batch, 0 where nothing is visible anywhere.  The backward is
    hpe_kp_loss_backward, which divides by the local count, scaled by local count / global count; nothing reads the device."""

    @staticmethod
    def forward(ctx, kp_gt, kp_pred, global_count):
        parts = _engine.kp_loss_parts(kp_gt.detach(), kp_pred.detach())
        g = global_count.detach().reshape(()).to(torch.float32)
        zero = torch.zeros_like(g)
        den = torch.clamp(g, min=1.0)
        ctx.save_for_backward(kp_gt.detach(), kp_pred.detach(), torch.where(g > 0, parts[1] / den, zero))
        return torch.where(g > 0, parts[0] / den, zero)

    @staticmethod
    def backward(ctx, grad_loss):
        kp_gt, kp_pred, ratio = ctx.saved_tensors
        return None, _engine.kp_loss_backward(kp_gt, kp_pred, grad_loss.to(torch.float32) * ratio), None


class Loss3DFunction(torch.autograd.Function):
    """(L_joints, L_smpl) = the 3-D supervision losses of one stage (DESIGN.md "3-D supervision"; hpe_loss3d), differentiable in joints
    [B,K,3], betas [B,10] and Rs [B,24,3,3] (hpe_loss3d_backward; stateless, so only the inputs are saved).  ``gt``: ``ops.Gt3D``.
    ``counts``: None for this batch's own (cnt_j, cnt_s), or those two as a [2] CUDA tensor already summed over the ranks
    (``loss3d_counts`` and one all-reduce): the losses are then this rank's SHARES, which add up to the losses of the global batch, 0
    where nothing is supervised anywhere.  ``parts``: this stage's row [5] of a ``loss3d_parts`` launch the caller made for several
    stages at once (None: launched here).  The backward scales by grad_loss * 0.5 / count on the device; nothing reads it."""

    @staticmethod
    def forward(ctx, joints, betas, Rs, gt, counts=None, parts=None):
        j, b, R = joints.detach(), betas.detach(), Rs.detach()
        if parts is None:
            parts = _engine.loss3d_parts(j, b, R, gt)[0]
        cnt = parts[3:5] if counts is None else counts.detach().reshape(2).to(torch.float32)
        den = torch.clamp(cnt, min=1.0)
        zero = torch.zeros_like(den)
        ctx.gt = gt
        ctx.save_for_backward(j, b, R, torch.where(cnt > 0, 0.5 / den, zero))
        loss = torch.where(cnt > 0, 0.5 * torch.stack([parts[0], parts[1] + parts[2]]) / den, zero)
        return loss[0], loss[1]

    @staticmethod
    def backward(ctx, grad_joints_loss, grad_smpl_loss):
        j, b, R, half = ctx.saved_tensors
        names = ("joints", "betas", "Rs")
        want = tuple(k for k, need in zip(names, ctx.needs_input_grad[:3]) if need)
        if not want:
            return (None,) * 6
        scale = [half[i : i + 1] * g.to(torch.float32) if g is not None else torch.zeros_like(half[i : i + 1])
                 for i, g in enumerate((grad_joints_loss, grad_smpl_loss))]
        g = _engine.loss3d_backward(j, b, R, ctx.gt, scale[0], scale[1], want=want)
        return tuple(g.get(k) for k in names) + (None, None, None)


class MeshLossFunction(torch.autograd.Function):
    """loss = mesh_reprojection_loss(seg, verts2d), differentiable in verts2d: the forward is ONE hpe_mesh_loss_grad call, which
    returns the loss and d loss / d verts2d from the same pair of searches; the backward scales the saved gradient."""

    @staticmethod
    def forward(ctx, engine, seg, verts2d):
        loss, grad = engine.mesh_loss_grad(seg.detach(), verts2d.detach())
        ctx.save_for_backward(grad)
        return loss.clone()

    @staticmethod
    def backward(ctx, grad_loss):
        (grad,) = ctx.saved_tensors
        return None, None, grad_loss.to(torch.float32) * grad


class CriticFunction(torch.autograd.Function):
    """scores = hpe_critic(joints, betas, Rs), differentiable in all three (hpe_critic_backward; stateless, so only the inputs are
    saved)."""

    @staticmethod
    def forward(ctx, engine, joints, betas, Rs):
        ctx.engine = engine
        ctx.save_for_backward(joints.detach(), betas.detach(), Rs.detach())
        return engine.critic(joints, betas, Rs)

    @staticmethod
    def backward(ctx, grad_scores):
        joints, betas, Rs = ctx.saved_tensors
        names = ("joints", "betas", "Rs")
        want = tuple(k for k, need in zip(names, ctx.needs_input_grad[1:]) if need)
        g = ctx.engine.critic_backward(joints, betas, Rs, grad_scores.to(torch.float32).contiguous(), want=want)
        return (None,) + tuple(g.get(k) for k in names)


class RegressorFunction(torch.autograd.Function):
    """thetas [S,B,85] = hpe_regressor_forward_train(features; the engine's live regressor), differentiable in ``params`` -- the flat
    tensor the optimiser owns, which must EQUAL what the engine holds: it carries ``.grad``, the arithmetic reads the engine's weights
    -- and in ``features`` (hpe_regressor_backward; stateless, so only the inputs are saved)."""

    @staticmethod
    def forward(ctx, engine, features, params, drop):
        ctx.engine = engine
        ctx.save_for_backward(features.detach(), drop.detach() if drop is not None else None)
        return engine.regressor_forward_train(features, drop)

    @staticmethod
    def backward(ctx, grad_thetas):
        features, drop = ctx.saved_tensors
        gflat, gfeat = ctx.engine.regressor_backward(features, grad_thetas.to(torch.float32).contiguous(), drop,
                                                     want_grad_features=ctx.needs_input_grad[1])
        return None, gfeat, gflat if ctx.needs_input_grad[2] else None, None


class EncoderFunction(torch.autograd.Function):
    """features [B,2048] = hpe_encoder_forward_train(images; the engine's live encoder, BatchNorm statistics fixed), differentiable in
    ``params`` -- the flat tensor the optimiser owns, which must EQUAL what the engine holds (``set_encoder_params_dev`` after every step):
    it carries ``.grad``, the arithmetic reads the engine's weights.  Images get no gradient.  hpe_encoder_backward is stateless, so only
    the images are saved.  ``bn``: "frozen" or "batch" (hpe_encoder_forward_batchnorm / hpe_encoder_backward_batchnorm).  ``precision``:
    "fp32" or "bf16" (hpe_encoder_forward_train_mixed / hpe_encoder_backward_mixed; frozen statistics only) or "mixed" (those two, or
    with bn="batch" hpe_encoder_forward_batchnorm_mixed / hpe_encoder_backward_batchnorm_mixed): features and ``.grad`` stay fp32."""

    @staticmethod
    def forward(ctx, engine, images, params, bn="frozen", precision="fp32"):
        ctx.engine, ctx.bn, ctx.precision = engine, bn, precision
        ctx.save_for_backward(images.detach())
        return engine.encoder_forward_train(images, bn=bn, precision=precision)

    @staticmethod
    def backward(ctx, grad_features):
        (images,) = ctx.saved_tensors
        g = (ctx.engine.encoder_backward(images, grad_features.to(torch.float32).contiguous(), bn=ctx.bn, precision=ctx.precision)
             if ctx.needs_input_grad[2] else None)
        return None, None, g, None, None
