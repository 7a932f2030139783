"""Torch restatement of the SMPL layer + orthographic projection (the mathematics of oracle/hmr_oracle.py's SMPL.__call__,
batch_orth_proj_idrot and reproject_vertices), differentiable by autograd and dtype-parametric.  Test helper: the gradient
reference of tests/test_gpu_smpl_backward.py, always evaluated in float64 on the CPU there."""
import numpy as np
import torch


class SmplTorch(object):
    def __init__(self, model, dtype=torch.float64, joint_type="cocoplus", img_size=224):
        def t(x):
            return torch.as_tensor(np.asarray(x, np.float32).astype(np.float64)).to(dtype)  # the float32-rounded constants

        self.dtype = dtype
        self.v_template = t(model["v_template"])  # [V,3]
        self.shapedirs = t(model["shapedirs"])  # [V,3,10]
        self.posedirs = t(model["posedirs"])  # [V,3,207]
        self.J_regressor = t(model["J_regressor"])  # [24,V]
        self.weights = t(model["weights"])  # [V,24]
        kp = np.asarray(model["cocoplus_regressor"])
        self.kp_regressor = t(kp[:14] if joint_type == "lsp" else kp)  # [K,V]
        self.parents = [int(p) for p in np.asarray(model["kintree_table"])[0].astype(np.int64)]
        self.img_size = float(img_size)

    def rodrigues(self, th):
        """th [N,3] -> [N,3,3]: angle = ||th + 1e-8||, axis = th / angle (the epsilon is in the norm only)"""
        angle = torch.sqrt(((th + 1e-8) ** 2).sum(1, keepdim=True))
        r = th / angle
        c, s = torch.cos(angle)[:, :, None], torch.sin(angle)[:, :, None]
        z = torch.zeros_like(r[:, 0])
        skew = torch.stack([z, -r[:, 2], r[:, 1], r[:, 2], z, -r[:, 0], -r[:, 1], r[:, 0], z], 1).reshape(-1, 3, 3)
        eye = torch.eye(3, dtype=th.dtype)[None]
        return c * eye + (1 - c) * (r[:, :, None] * r[:, None, :]) + s * skew

    def __call__(self, theta):
        """theta [B,85] = [s, tx, ty | 72 axis-angle | 10 betas] -> dict of every output of hpe_smpl"""
        B = theta.shape[0]
        cam, pose, beta = theta[:, :3], theta[:, 3:75], theta[:, 75:]
        v_shaped = self.v_template[None] + torch.einsum("vck,bk->bvc", self.shapedirs, beta)
        J = torch.einsum("jv,bvc->bjc", self.J_regressor, v_shaped)
        Rs = self.rodrigues(pose.reshape(-1, 3)).reshape(B, 24, 3, 3)
        pose_feature = (Rs[:, 1:] - torch.eye(3, dtype=theta.dtype)).reshape(B, 207)
        v_posed = v_shaped + torch.einsum("vck,bk->bvc", self.posedirs, pose_feature)
        # global rigid transforms down the kinematic tree
        GR, Gt = [Rs[:, 0]], [J[:, 0]]
        for j in range(1, 24):
            p = self.parents[j]
            GR.append(GR[p] @ Rs[:, j])
            Gt.append((GR[p] @ (J[:, j] - J[:, p])[:, :, None])[:, :, 0] + Gt[p])
        GR, Gt = torch.stack(GR, 1), torch.stack(Gt, 1)  # [B,24,3,3], [B,24,3]
        At = Gt - (GR @ J[:, :, :, None])[..., 0]  # A = G - [0 | G_R J]
        TR = torch.einsum("vj,bjrc->bvrc", self.weights, GR)
        Tt = torch.einsum("vj,bjr->bvr", self.weights, At)
        verts = (TR @ v_posed[..., None])[..., 0] + Tt
        joints = torch.einsum("kv,bvc->bkc", self.kp_regressor, verts)
        s, t = cam[:, None, 0:1], cam[:, None, 1:3]
        kp2d = s * (joints[:, :, :2] + t)
        verts2d = (s * (verts[:, :, :2] + t) + 1.0) * 0.5 * self.img_size
        return dict(verts=verts, joints=joints, J_transformed=Gt, kp2d=kp2d, verts2d=verts2d, Rs=Rs, cams=cam * 1.0, theta=theta * 1.0)


def make_theta(B, seed, special=True):
    """theta rows as drawn for the gradient checks: s = 0.9 + 0.1 N, t = 0.1 N, pose 0.3 N with the root + pi, betas N; with
    ``special`` image 0 is the exact mean-pose shape (23 non-root joints exactly zero), image 1 (if any) has its pose scaled by
    1e-4, image 2 (if any) has a joint rotation of angle near pi."""
    g = np.random.RandomState(seed)
    th = np.zeros((B, 85), np.float64)
    th[:, 0] = 0.9 + 0.1 * g.randn(B)
    th[:, 1:3] = 0.1 * g.randn(B, 2)
    th[:, 3:75] = 0.3 * g.randn(B, 72)
    th[:, 3] += np.pi
    th[:, 75:] = g.randn(B, 10)
    if special:
        th[0, 6:75] = 0.0
        if B > 1:
            th[1, 3:75] *= 1e-4
        if B > 2:
            ax = g.randn(3)
            th[2, 3 + 3 * 5 : 6 + 3 * 5] = ax / np.linalg.norm(ax) * (np.pi - 1e-3)
    return th.astype(np.float32)
