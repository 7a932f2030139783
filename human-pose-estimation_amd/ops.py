"""Losses on the path's outputs (reference: src/ops.py:35-137; the critic term of the generator loss, src/trainer.py:300-313),
HIP-backed (BASELINE config 5)."""
from __future__ import annotations

import collections

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


def kp_visible_count(kp_gt):
    """2 * #visible of kp_gt [N,K,3] as a one-element CUDA tensor (hpe_kp_loss's own count): what a data-parallel caller all-reduces
    BEFORE the forward, so that every rank divides by the count of the global batch"""
    return _engine.kp_loss_parts(kp_gt, kp_gt[..., :2].contiguous())[1:2].clone()


def kp_loss_share(numerator, global_count):
    """one rank's share of the keypoint loss: its numerator sum(vis * |d|) over the denominator of ALL ranks, 0 where nothing is visible
    anywhere; the shares of the ranks add up to the loss of the global batch.  Plain torch, any device."""
    import torch

    g = global_count.reshape(()).to(numerator.dtype)
    return torch.where(g > 0, numerator / torch.clamp(g, min=1.0), torch.zeros_like(g))


def kp_reprojection_loss_share(kp_gt, kp_pred, global_count):
    """``kp_loss_share`` of this rank's rows through the library (hpe_kp_loss); differentiable in a kp_pred that requires grad"""
    import torch

    if torch.is_grad_enabled() and isinstance(kp_pred, torch.Tensor) and kp_pred.requires_grad:
        from .autograd import KpLossShareFunction

        return KpLossShareFunction.apply(kp_gt, kp_pred, global_count)
    return kp_loss_share(_engine.kp_loss_parts(kp_gt, kp_pred)[0], global_count)


class Gt3D(collections.namedtuple("Gt3D", "joints Rs shape w_joints w_smpl flip")):
    """The 3-D ground truth of a batch as the 3-D losses take it (DESIGN.md "3-D supervision"; built by ``augment.gt3d_real``), all CUDA
    tensors: joints float32 [B,14,3], Rs float32 [B,24,3,3] (``engine.smpl``'s rotations of the ground-truth theta), shape float32
    [B,10], the row weights w_joints [B] and w_smpl [B] (0: the row is not supervised by that term, and its labels are not read), and
    flip uint8 or bool [B] (None: no flips): the labels are UNFLIPPED, the kernel mirrors those of a flipped row."""
    __slots__ = ()

    def rows(self, lo, hi):
        """the ground truth of rows lo .. hi - 1"""
        return Gt3D(*[None if t is None else t[lo:hi] for t in self])


def loss3d_counts(gt):
    """(42 * #rows with w_joints != 0, 226 * #rows with w_smpl != 0) of ``gt`` as a [2] CUDA tensor (hpe_loss3d's own counts): what a
    data-parallel caller sums over the ranks BEFORE the forward, so that every rank divides by the counts of the global batch"""
    return _engine.loss3d_parts(gt.joints, gt.shape, gt.Rs, gt)[0, 3:5].clone()


def loss3d(joints, betas, Rs, gt, counts=None, parts=None):
    """-> (joints3d_loss, smpl_param_loss) of one stage from one hpe_loss3d launch (``Loss3DFunction``)"""
    from .autograd import Loss3DFunction

    return Loss3DFunction.apply(joints, betas, Rs, gt, counts, parts)


def joints3d_loss(joints, gt, counts=None):
    """0.5 * sum_i w_i sum_k |e_ik|^2 / (42 * #supervised rows): the L2 loss on the first 14 joints of joints [B,K,3] against
    ``gt.joints``, both relative to their pelvis (the midpoint of the hips, joints 2 and 3), over the rows with ``gt.w_joints`` != 0; 0
    where there is none.  counts: ``loss3d_counts`` summed over the ranks, for this rank's share.  Differentiable in joints
    (hpe_loss3d_backward, the derivative of the alignment included)."""
    return loss3d(joints, gt.shape, gt.Rs, gt, counts)[0]  # the SMPL term of the same launch compares gt with itself and is dropped


def smpl_param_loss(betas, Rs, gt, counts=None):
    """0.5 * sum_i w_i (|Rs_i - R_i|_F^2 + |betas_i - shape_i|^2) / (226 * #supervised rows): the L2 loss on the 24 rotation matrices
    Rs [B,24,3,3] and the shape betas [B,10] (a ``theta[:, 75:]`` view is read in place) over the rows with ``gt.w_smpl`` != 0; 0
    where there is none.  counts as ``joints3d_loss``.  Differentiable in betas and Rs."""
    return loss3d(gt.joints, betas, Rs, gt, counts)[1]


def critic_term_share(scores, global_rows):
    """one rank's share of -reduce_sum(reduce_mean(scores, 0)): its column sums over the rows of ALL ranks.  Plain torch."""
    return -(scores.sum(0) / global_rows).sum()


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


def generator_critic_loss(engine, joints, shapes, Rs, return_parts=False, global_rows=None):
    """-reduce_sum(reduce_mean(critic scores, 0)) (src/trainer.py:309-313, before critic_loss_weight).  return_parts=True returns the
    tensor [4] = (the three column sums, N) so that ranks can all-reduce before dividing (forward only), as kp_reprojection_loss does.
    global_rows: this rank's share of the term over a batch of that many rows spread across ranks (``critic_term_share``)."""
    scores = critic_scores(engine, joints, shapes, Rs)
    if global_rows is not None:
        return critic_term_share(scores, global_rows)
    if return_parts:
        import torch

        return torch.cat([scores.detach().sum(0), scores.new_full((1,), float(scores.shape[0]))])
    return -scores.mean(0).sum()


def encoder_features(engine, images, params, bn="frozen", precision="fp32"):
    """features [B,2048] of the engine's encoder (layer by layer, BatchNorm statistics fixed), differentiable in ``params``, the flat
    tensor [resnet_spec.ENCODER_PARAM_FLOATS] that must equal ``engine.encoder_params()``; needs ``engine.reserve_encoder_train(B)``.
    bn="batch": BatchNorm with the statistics of this batch, the gradient through them (``reserve_encoder_train(B, batch_norm=True)``).
    precision="bf16": the mixed-precision walks (``reserve_encoder_train(B, precision="bf16")``; frozen statistics only): bf16
    activations, cotangents and matrix products with fp32 accumulation; ``params``, the features and ``.grad`` stay fp32.
    precision="mixed": the same walks with bn="frozen"; with bn="batch" (``reserve_encoder_train(B, batch_norm=True,
    precision="mixed")``) the bf16 walks with batch statistics, BatchNorm arithmetic in fp32 and its reductions in float64"""
    from .autograd import EncoderFunction
    from .engine import HpeEngine

    HpeEngine._mixed(precision, bn)  # refuses bn="batch" with precision="bf16" (use "mixed") before anything runs
    return EncoderFunction.apply(engine, images, params, bn, precision)


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


def wgan_terms(wgan_sums, grad_sums, N, gp_weight=10.0):
    """The critic's loss from the plain sums over N rows (``critic_wgan_loss``; a data-parallel caller passes the sums and the N of ALL
    ranks): wgan = sum(wgan_sums) / N, penalty = sum over the four inputs of (1 - ||grad_sum / N||)^2, loss = wgan + gp_weight * penalty,
    and tangents = d(gp_weight * penalty) / d(the penalised gradient of any one row), the same vector for every row.  Plain torch.
    -> dict wgan, penalty, loss, norms, tangents (a list in the order of grad_sums)"""
    wgan = wgan_sums.sum() / N
    norms = [(s / N).norm() for s in grad_sums]
    penalty = sum((1.0 - n) ** 2 for n in norms)
    tangents = [((-2.0 * gp_weight / N) * (1.0 - n) / n) * (s / N) for n, s in zip(norms, grad_sums)]
    return dict(wgan=wgan, penalty=penalty, loss=wgan + gp_weight * penalty, norms=norms, tangents=tangents)


def pack_critic_sums(wgan_sums, grad_sums, N):
    """the sums of ``critic_wgan_loss`` and N as ONE flat block, for one all-reduce"""
    import torch

    return torch.cat([wgan_sums.reshape(-1)] + [s.reshape(-1) for s in grad_sums] + [wgan_sums.new_full((1,), float(N))])


def unpack_critic_sums(block, like):
    """the inverse: ``like`` = the local grad_sums (for the shapes) -> (wgan_sums, grad_sums, rows as a one-element tensor)"""
    out, pos = [], 3
    for s in like:
        out.append(block[pos:pos + s.numel()].reshape(s.shape))
        pos += s.numel()
    return block[:3], out, block[pos:pos + 1]


def critic_wgan_loss(engine, real, fake, gp_weight=10.0, interp=None, generator=None, return_grad=True, per_row=False, reduce=None,
                     global_rows=None):
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
    scores), grad_sums (the four sums over the rows of the penalised gradients, Rs without the root) and N.

    reduce (``Reducer.sum_block``) with global_rows: the data-parallel form, see ``_critic_wgan_reduced``."""
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
    if reduce is not None:
        return _critic_wgan_reduced(engine, (j2, b2, R2), (ji, bi, Ri), wgan_sums, grad_sums, N, gp_weight, return_grad, per_row, reduce, global_rows)
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


def _critic_wgan_reduced(engine, both, interpolated, wgan_sums, grad_sums, N, gp_weight, return_grad, per_row, reduce, global_rows):
    """``critic_wgan_loss`` on this rank's N rows of ``global_rows`` spread across ranks: the sums and N go through ``reduce`` (ONE packed
    all-reduce, in place) before the norms; loss, wgan and penalty are those of the global batch; grad_scores and the tangents divide
    by the global row count, so ``grad`` is this rank's partial and the sum over the ranks the gradient of the global batch.
    ``global_rows`` is the caller's host number (nothing reads the device); the reduced N comes back as ``rows`` for whoever checks."""
    import torch

    if per_row:
        raise ValueError("per_row is not available with reduce")
    if global_rows is None or int(global_rows) < N:
        raise ValueError("reduce needs global_rows, the rows of all ranks (at least this rank's %d)" % N)
    G = int(global_rows)
    wgan_sums, grad_sums, rows = unpack_critic_sums(reduce(pack_critic_sums(wgan_sums, grad_sums, N)), grad_sums)
    t = wgan_terms(wgan_sums, grad_sums, G, gp_weight)
    out = dict(loss=t["loss"], wgan=t["wgan"], penalty=t["penalty"], wgan_sums=wgan_sums, grad_sums=grad_sums, N=G, rows=rows)
    if return_grad:
        j2, b2, R2 = both
        gs = torch.full((2 * N, 3), 1.0 / G, dtype=torch.float32, device=j2.device)
        gs[:N] = -1.0 / G
        out["grad"] = engine.critic_weight_grad(j2, b2, R2, grad_scores=gs) + engine.critic_weight_grad(*interpolated, tangents=dict(zip(_PENALTY_ORDER, t["tangents"])))
    return out
