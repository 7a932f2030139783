"""fit_keypoints / fit_reprojection: refine theta rows against 2-D keypoints and / or a silhouette by descending the reprojection
losses (the SMPLify-style use of the SMPL backward), optionally with the critic as a prior.  Adam is torch.optim.Adam; the losses, the SMPL layer, the projection and their
gradients run in libhpe_hip.so."""
from __future__ import annotations

from .ops import generator_critic_loss, kp_reprojection_loss, mesh_reprojection_loss

KPR_LOSS_WEIGHT = 60.0  # the reference's kpr_loss_weight (src/config.py)
MR_LOSS_WEIGHT = 0.001  # its mr_loss_weight
CRITIC_LOSS_WEIGHT = 0.01  # its critic_loss_weight (src/config.py:69); fit_reprojection's default is 0: no prior
_GROUPS = {"cam": (0, 3), "pose": (3, 75), "betas": (75, 85)}


def fit_keypoints(engine_or_predictor, theta0, kp_gt, steps=100, lr=0.01, fit=("cam", "pose", "betas")):
    """theta0 [B,85] (B <= the engine's max_batch), kp_gt [B,K,3] (x, y, vis) -> (theta [B,85], losses [steps]).

    Runs ``steps`` Adam steps on 60 * kp_reprojection_loss(kp_gt, kp2d(theta)) over the groups named in ``fit``; the other
    columns of theta stay as given.  ``losses`` (a device tensor) holds the unweighted loss BEFORE each step; nothing in the loop
    reads the device, so the host only enqueues."""
    import torch

    engine = getattr(engine_or_predictor, "engine", engine_or_predictor)
    unknown = [g for g in fit if g not in _GROUPS]
    if unknown:
        raise ValueError("fit names %r are not among %s" % (unknown, sorted(_GROUPS)))
    dev = engine.tdev
    theta0 = torch.as_tensor(theta0, dtype=torch.float32).to(dev)
    kp_gt = torch.as_tensor(kp_gt, dtype=torch.float32).to(dev).contiguous()
    if theta0.dim() != 2 or theta0.shape[1] != 85 or kp_gt.shape[0] != theta0.shape[0]:
        raise ValueError("theta0 must be [B,85] and kp_gt [B,K,3]")
    parts = {g: theta0[:, lo:hi].detach().clone().requires_grad_(g in fit) for g, (lo, hi) in _GROUPS.items()}
    opt = torch.optim.Adam([parts[g] for g in _GROUPS if g in fit], lr=lr)
    losses = torch.zeros(int(steps), dtype=torch.float32, device=dev)
    for i in range(int(steps)):
        opt.zero_grad(set_to_none=True)
        theta = torch.cat([parts["cam"], parts["pose"], parts["betas"]], 1)
        loss = kp_reprojection_loss(kp_gt, engine.smpl(theta, want=("kp2d",))["kp2d"])
        losses[i].copy_(loss.detach())
        (KPR_LOSS_WEIGHT * loss).backward()
        opt.step()
    return torch.cat([parts["cam"], parts["pose"], parts["betas"]], 1).detach(), losses


def fit_reprojection(engine_or_predictor, theta0, kp_gt=None, seg_gts=None, steps=100, lr=0.01, fit=("cam", "pose", "betas"),
                     kpr_weight=KPR_LOSS_WEIGHT, mr_weight=MR_LOSS_WEIGHT, critic_weight=0.0):
    """theta0 [B,85] (B <= the engine's max_batch), kp_gt [B,K,3] (x, y, vis) and / or seg_gts [B,H,W(,1)] (> 0 = silhouette)
    -> (theta [B,85], losses [steps, 2]).

    Runs ``steps`` Adam steps on the reference's two reprojection terms (src/trainer.py:433-448),
    kpr_weight * kp_reprojection_loss(kp_gt, kp2d(theta)) + mr_weight * mesh_reprojection_loss(seg_gts, verts2d(theta)), over the
    groups named in ``fit``; a target that is None drops its term (at least one must be given).  ``losses`` (a device tensor) holds
    the unweighted (kp, mesh) losses BEFORE each step, 0 for a dropped term; nothing in the loop reads the device.

    critic_weight > 0 (the reference trains with CRITIC_LOSS_WEIGHT = 0.01) adds the learned prior over bone geometry, shape and joint
    rotations as a further term, critic_weight * generator_critic_loss(joints(theta), betas(theta), Rs(theta)) (src/trainer.py:300-313),
    which keeps the descent away from poses that reproject well and are anatomically impossible; it needs an engine with a loaded
    critic, and ``losses`` is then [steps, 3] = (kp, mesh, critic).  0 (the default) runs the loop exactly as without the argument."""
    import torch

    engine = getattr(engine_or_predictor, "engine", engine_or_predictor)
    if kp_gt is None and seg_gts is None:
        raise ValueError("fit_reprojection needs kp_gt, seg_gts or both")
    use_critic = float(critic_weight) > 0.0
    if float(critic_weight) < 0.0:
        raise ValueError("critic_weight must be >= 0")
    if use_critic and not engine.has_critic:
        raise RuntimeError("fit_reprojection(critic_weight > 0) needs an engine with a loaded critic (HpeEngine.load_critic)")
    unknown = [g for g in fit if g not in _GROUPS]
    if unknown:
        raise ValueError("fit names %r are not among %s" % (unknown, sorted(_GROUPS)))
    dev = engine.tdev
    theta0 = torch.as_tensor(theta0, dtype=torch.float32).to(dev)
    if theta0.dim() != 2 or theta0.shape[1] != 85:
        raise ValueError("theta0 must be [B,85]")
    if kp_gt is not None:
        kp_gt = torch.as_tensor(kp_gt, dtype=torch.float32).to(dev).contiguous()
        if kp_gt.dim() != 3 or kp_gt.shape[0] != theta0.shape[0] or kp_gt.shape[2] != 3:
            raise ValueError("kp_gt must be [B,K,3]")
    if seg_gts is not None:
        seg_gts = torch.as_tensor(seg_gts, dtype=torch.float32).to(dev)
        if seg_gts.dim() == 4:
            seg_gts = seg_gts[..., 0]
        seg_gts = seg_gts.contiguous()
        if seg_gts.dim() != 3 or seg_gts.shape[0] != theta0.shape[0]:
            raise ValueError("seg_gts must be [B,H,W] or [B,H,W,1]")
    parts = {g: theta0[:, lo:hi].detach().clone().requires_grad_(g in fit) for g, (lo, hi) in _GROUPS.items()}
    opt = torch.optim.Adam([parts[g] for g in _GROUPS if g in fit], lr=lr)
    losses = torch.zeros((int(steps), 3 if use_critic else 2), dtype=torch.float32, device=dev)
    want = ("kp2d", "verts2d") + (("joints", "Rs") if use_critic else ())
    for i in range(int(steps)):
        opt.zero_grad(set_to_none=True)
        theta = torch.cat([parts["cam"], parts["pose"], parts["betas"]], 1)
        out = engine.smpl(theta, want=want)
        total = None
        if kp_gt is not None:
            kp = kp_reprojection_loss(kp_gt, out["kp2d"])
            losses[i, 0].copy_(kp.detach())
            total = kpr_weight * kp
        if seg_gts is not None:
            mesh = mesh_reprojection_loss(engine, seg_gts, out["verts2d"])
            losses[i, 1].copy_(mesh.detach())
            total = mr_weight * mesh if total is None else total + mr_weight * mesh
        if use_critic:
            prior = generator_critic_loss(engine, out["joints"], theta[:, 75:], out["Rs"])
            losses[i, 2].copy_(prior.detach())
            total = total + critic_weight * prior
        total.backward()
        opt.step()
    return torch.cat([parts["cam"], parts["pose"], parts["betas"]], 1).detach(), losses
