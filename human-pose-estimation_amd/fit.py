"""fit_keypoints: refine theta rows against 2-D keypoints by descending the keypoint reprojection loss (the SMPLify-style use of
the SMPL backward).  Adam is torch.optim.Adam; the loss, the SMPL layer, the projection and their gradients run in libhpe_hip.so."""
from __future__ import annotations

from .ops import kp_reprojection_loss

KPR_LOSS_WEIGHT = 60.0  # the reference's kpr_loss_weight (src/config.py)
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
