"""Losses on the path's outputs (reference: src/ops.py:35-137; the critic term of the generator loss, src/trainer.py:300-313),
HIP-backed (BASELINE config 5)."""
from __future__ import annotations

from . import engine as _engine


def kp_reprojection_loss(kp_gt, kp_pred, scale=1.0, name="kp_reprojection_loss", return_parts=False):
    """kp_gt [N,K,3] (x, y, vis), kp_pred [N,K,2] -> sum(vis*|d|) / (2*#visible), 0 if none visible
    (tf.compat.v1.losses.absolute_difference, SUM_BY_NONZERO_WEIGHTS; src/ops.py:35-47).
    return_parts=True returns the tensor [numerator, count, loss] so ranks can all-reduce before dividing (forward only).
    A kp_pred that requires grad makes the loss differentiable with respect to it (hpe_kp_loss_backward)."""
    import torch

    if not return_parts and torch.is_grad_enabled() and isinstance(kp_pred, torch.Tensor) and kp_pred.requires_grad:
        from .autograd import KpLossFunction

        return KpLossFunction.apply(kp_gt, kp_pred)
    parts = _engine.kp_loss_parts(kp_gt, kp_pred)
    return parts if return_parts else parts[2]


def mesh_reprojection_loss(engine, seg_gts, silhouette_pred, name="mesh_reprojection_loss"):
    """seg_gts [N,H,W(,1)] (> 0 = silhouette), silhouette_pred [N,6890,2] pixels -> scalar
    sum_i bidirectional_dist_i / (3 + 6890)   (src/ops.py:117-137 with src/trainer.py:291 folded in:
    the reference first builds tf.where(seg > 0); here the compaction is a kernel of the same call).
    A silhouette_pred that requires grad makes the loss differentiable with respect to it (hpe_mesh_loss_grad; the silhouette is a
    constant)."""
    if seg_gts.dim() == 4:
        seg_gts = seg_gts[..., 0]
    import torch

    if torch.is_grad_enabled() and isinstance(silhouette_pred, torch.Tensor) and silhouette_pred.requires_grad:
        from .autograd import MeshLossFunction

        return MeshLossFunction.apply(engine, seg_gts.contiguous(), silhouette_pred)
    return engine.mesh_loss(seg_gts.contiguous(), silhouette_pred)


def critic_scores(engine, joints, shapes, Rs):
    """critic_network([get_kcs(joints), joints[:, :14], shapes, Rs[:, 1:]]) (src/trainer.py:300-308; CriticNetwork and get_kcs,
    src/models.py:97-202) as one hpe_critic call: joints [N,K,3], shapes [N,10] (a theta[:, 75:] view is read in place), Rs [N,24,3,3]
    -> scores [N,3].  An input that requires grad makes the scores differentiable in joints, shapes and Rs (hpe_critic_backward)."""
    import torch

    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (joints, shapes, Rs)):
        from .autograd import CriticFunction

        return CriticFunction.apply(engine, joints, shapes, Rs)
    return engine.critic(joints, shapes, Rs)


def generator_critic_loss(engine, joints, shapes, Rs, return_parts=False):
    """-reduce_sum(reduce_mean(critic scores, 0)) (src/trainer.py:309-313, before critic_loss_weight).  return_parts=True returns the
    tensor [4] = (the three column sums, N) so that ranks can all-reduce before dividing (forward only), as kp_reprojection_loss does."""
    scores = critic_scores(engine, joints, shapes, Rs)
    if return_parts:
        import torch

        return torch.cat([scores.detach().sum(0), scores.new_full((1,), float(scores.shape[0]))])
    return -scores.mean(0).sum()
