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


def encoder_features(engine, images, params, bn="frozen"):
    """features [B,2048] of the engine's encoder (layer by layer, BatchNorm statistics fixed), differentiable in ``params``, the flat
    tensor [resnet_spec.ENCODER_PARAM_FLOATS] that must equal ``engine.encoder_params()``; needs ``engine.reserve_encoder_train(B)``.
    bn="batch": BatchNorm with the statistics of this batch, the gradient through them (``reserve_encoder_train(B, batch_norm=True)``)"""
    from .autograd import EncoderFunction

    return EncoderFunction.apply(engine, images, params, bn)


def regressor_thetas(engine, features, params, drop=None):
    """The IEF loop of the generator step (src/trainer.py:389-401) on the engine's live regressor: features [B,2048] -> thetas
    [num_stage,B,85], with ``drop`` [2,B,1024] the dropout multipliers of the last stage (None: none).  ``params`` is the flat
    parameter tensor the optimiser owns (``engine.regressor_params()`` layout); it must equal what the engine holds -- it is the
    carrier of ``.grad``, not a second copy of the arithmetic.  The result has a ``grad_fn``: its backward is ONE
    hpe_regressor_backward call that fills ``params.grad`` and, if ``features`` requires grad, ``features.grad``."""
    from .autograd import RegressorFunction
    from .regressor_spec import PARAM_FLOATS

    if tuple(params.shape) != (PARAM_FLOATS,):
        raise ValueError("params must be the flat tensor [%d], got %s" % (PARAM_FLOATS, tuple(params.shape)))
    return RegressorFunction.apply(engine, features, params, drop)


_PENALTY_ORDER = ("kcs", "joints", "betas", "Rs")  # tf.gradients(out_interpolated, [kcs, joints, shapes, Rs]) (src/trainer.py:566-570)


def critic_gradient_penalty(grads):
    """compute_gradient_penalty (src/ops.py:153-172): grads = the four tensors [N, ...] of tf.gradients(out_interpolated, [kcs, joints,
    shapes, Rs]) -> sum over the four of (1 - || mean over the rows ||_2)^2.  The norm of the batch MEAN per input, as the reference
    has it, not the per-row norm of the WGAN-GP paper.  Plain torch on whatever device the tensors live on."""
    grads = list(grads)
    if len(grads) != 4:
        raise ValueError("the penalty takes the four gradients (kcs, joints, shapes, Rs), got %d tensors" % len(grads))
    return sum((1.0 - g.mean(0).norm()) ** 2 for g in grads)


def critic_wgan_loss(engine, real, fake, gp_weight=10.0, interp=None, generator=None, return_grad=True, per_row=False):
    """The critic's loss of Trainer.train_step and its gradient with respect to the critic's weights (src/trainer.py:511-583):

        loss = wgan + gp_weight * penalty
        wgan = reduce_sum(reduce_mean(critic(fake) - critic(real), 0))
        penalty = critic_gradient_penalty(d(sum scores) / d[kcs, joints, shapes, Rs]) at the rows fake + U(0,1) * (real - fake)

    ``real`` and ``fake`` are (joints [N,K,3], shapes [N,10], Rs [N,24,3,3]) triples with equal N; the first 14 joints are used.
    ``interp`` = (alpha [N,14,3], beta [N,10], gamma [N,24,3,3]) passes the uniform tensors; otherwise they are drawn with
    ``generator``.  per_row=True is the WGAN-GP paper's form instead: penalty = sum over the four inputs of the mean over the rows of
    (1 - ||g[n]||)^2.

    Scores come from hpe_critic, the penalised gradients from hpe_critic_backward (ones), the weight gradient from two
    hpe_critic_weight_grad calls: the real and fake rows concatenated with grad_scores -1/N and +1/N, and the interpolated rows with
    the tangent d(gp_weight * penalty) / d(those gradients).  Nothing reads the device.

    -> dict: loss, wgan, penalty (0-dim tensors), grad (flat [PARAM_FLOATS]; absent with return_grad=False), and the plain sums over
    the rows a data-parallel caller all-reduces before it divides and takes the norms: wgan_sums [3] (column sums of fake - real
    scores), grad_sums (the four sums over the rows of the penalised gradients, Rs without the root) and N."""
    import torch

    jr, br, Rr = real
    jf, bf, Rf = fake
    N = jf.shape[0]
    if jr.shape[0] != N or br.shape[0] != N or bf.shape[0] != N or Rr.shape[0] != N or Rf.shape[0] != N:
        raise ValueError("real and fake must have the same number of rows")
    jr, jf = jr.detach()[:, :14], jf.detach()[:, :14]
    br, bf, Rr, Rf = br.detach(), bf.detach(), Rr.detach(), Rf.detach()
    if interp is None:
        alpha, beta, gamma = (torch.rand(t.shape, generator=generator, device=t.device, dtype=t.dtype) for t in (jf, bf, Rf))
    else:
        alpha, beta, gamma = interp
    # the real and the fake rows as one batch: one forward, and one weight-gradient call
    j2, b2, R2 = torch.cat([jr, jf]), torch.cat([br, bf]), torch.cat([Rr, Rf])
    scores = engine.critic(j2, b2, R2)
    wgan_sums = scores[N:].sum(0) - scores[:N].sum(0)
    wgan = wgan_sums.sum() / N
    ji, bi, Ri = jf + alpha * (jr - jf), bf + beta * (br - bf), Rf + gamma * (Rr - Rf)
    g = engine.critic_backward(ji, bi, Ri, None, want=_PENALTY_ORDER)
    g["Rs"] = g["Rs"][:, 1:]  # the root is no input of the critic: its gradient is zero
    grad_sums = [g[k].sum(0) for k in _PENALTY_ORDER]
    if per_row:
        norms = [g[k].reshape(N, -1).norm(dim=1) for k in _PENALTY_ORDER]
        penalty = sum(((1.0 - n) ** 2).mean() for n in norms)
    else:
        norms = [(s / N).norm() for s in grad_sums]
        penalty = sum((1.0 - n) ** 2 for n in norms)
    out = dict(loss=wgan + gp_weight * penalty, wgan=wgan, penalty=penalty, wgan_sums=wgan_sums, grad_sums=grad_sums, N=N)
    if return_grad:
        gs = torch.full((2 * N, 3), 1.0 / N, dtype=torch.float32, device=scores.device)
        gs[:N] = -1.0 / N
        if per_row:  # d(gp_weight * mean_n (1 - ||g_n||)^2) / d g_n
            tangents = {k: ((-2.0 * gp_weight / N) * (1.0 - n) / n).reshape((N,) + (1,) * (g[k].dim() - 1)) * g[k] for k, n in zip(_PENALTY_ORDER, norms)}
        else:  # d(gp_weight * (1 - ||m||)^2) / d g_n with m the mean over the rows: the same vector for every row
            tangents = {k: ((-2.0 * gp_weight / N) * (1.0 - n) / n) * (s / N) for k, n, s in zip(_PENALTY_ORDER, norms, grad_sums)}
        out["grad"] = engine.critic_weight_grad(j2, b2, R2, grad_scores=gs) + engine.critic_weight_grad(ji, bi, Ri, tangents=tangents)
    return out
