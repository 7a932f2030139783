"""Restatement of the generator step's IEF loop (src/trainer.py:389-401) over the RegressionNetwork (src/models.py:60-74) in torch, with
the dropout multipliers as explicit inputs: the yardstick of the regressor-training tests, as critic_train_ref.py is for the critic.

    x_i = [f | theta_{i-1}],  theta_{-1} = tile(mean)
    a1 = drop1_i * relu(x_i W1 + b1),  a2 = drop2_i * relu(a1 W2 + b2),  theta_i = theta_{i-1} + a2 W3 + b3

drop [2,B,1024] acts at the last stage only (training=True is passed there only).  float64 on the CPU is the reference; the same code in
float32 (CPU or GPU) is the fp32 restatement that headroom and timing are measured against.  ``kernel_arithmetic`` restates in numpy
float64 what the HIP backward computes: gates from a > 0, the hoisted sum of dz1, weight gradients as products over the stacked rows."""
import numpy as np
import torch

from hpe_amd import regressor_spec, synthetic
from oracle import hmr_oracle as O

S = regressor_spec.NUM_STAGE
KEYS = [k for k, _ in regressor_spec.REGRESSOR_TENSORS]
KINK = 1e-5  # 3x the worst fp32-vs-fp64 pre-activation difference measured on these inputs (3.2e-6)


def fixture_params():
    """(Keras-layout dict of the bounded regressor, mean theta [85] with s = 0.9 and root pi)"""
    return synthetic.make_regressor_params(variant="bounded"), O.load_mean_param(synthetic.make_mean_params()).reshape(85).astype(np.float32)


def flat_of(params, mean):
    return regressor_spec.params_to_flat(params, mean)


def make_features(B, seed):
    g = np.random.Generator(np.random.Philox(int(seed)))
    return np.abs(g.normal(0, 1, (B, 2048))).astype(np.float32)


def make_drop(B, seed):
    """[2,B,1024] multipliers, 0 or 2 with equal probability (Keras Dropout(0.5))"""
    g = np.random.Generator(np.random.Philox(int(seed) + 17))
    return (2.0 * (g.random((2, B, 1024)) >= 0.5)).astype(np.float32)


def tensors(flat, dtype=torch.float64, device="cpu", requires_grad=True):
    """flat numpy vector -> {key: leaf tensor}"""
    p = regressor_spec.flat_to_params(np.asarray(flat))
    return {k: torch.as_tensor(v, device=device).to(dtype).requires_grad_(requires_grad) for k, v in p.items()}


def ief(P, feat, drop=None, stages=S):
    """-> (thetas [S,B,85], pre: the 2 S pre-activations [B,1024] in stage order)"""
    B = feat.shape[0]
    th = P["mean_theta"].reshape(1, 85).expand(B, 85)
    out, pre = [], []
    for i in range(stages):
        z1 = torch.cat([feat, th], 1) @ P["dense_0/kernel"] + P["dense_0/bias"]
        a1 = torch.relu(z1)
        if drop is not None and i == stages - 1:
            a1 = a1 * drop[0]
        z2 = a1 @ P["dense_1/kernel"] + P["dense_1/bias"]
        a2 = torch.relu(z2)
        if drop is not None and i == stages - 1:
            a2 = a2 * drop[1]
        th = th + a2 @ P["dense_2/kernel"] + P["dense_2/bias"]
        out.append(th)
        pre += [z1, z2]
    return torch.stack(out), pre


def as_t(x, dtype, device="cpu"):
    return None if x is None else torch.as_tensor(np.asarray(x), device=device).to(dtype)


def forward(flat, feat, drop=None, dtype=torch.float64):
    with torch.no_grad():
        th, _ = ief(tensors(flat, dtype, requires_grad=False), as_t(feat, dtype), as_t(drop, dtype))
    return th.numpy()


def autograd_grads(flat, feat, drop, grad_thetas, dtype=torch.float64):
    """-> (flat gradient [PARAM_FLOATS], grad_features [B,2048]) of sum(grad_thetas * thetas), as numpy arrays of ``dtype``"""
    P = tensors(flat, dtype)
    f = as_t(feat, dtype).requires_grad_(True)
    th, _ = ief(P, f, as_t(drop, dtype))
    (th * as_t(grad_thetas, dtype)).sum().backward()
    g = np.concatenate([(P[k].grad if P[k].grad is not None else torch.zeros_like(P[k])).reshape(-1).numpy() for k in KEYS])
    return g, f.grad.numpy()


def kink_distance(flat, feat, drops=(None,)):
    """per row, the smallest |pre-activation| over the 2 S x 1024 units, in float64, over every dropout setting in ``drops``"""
    d = None
    for drop in drops:
        with torch.no_grad():
            _, pre = ief(tensors(flat, requires_grad=False), as_t(feat, torch.float64), as_t(drop, torch.float64))
        m = torch.cat([z.abs() for z in pre], 1).min(1).values.numpy()
        d = m if d is None else np.minimum(d, m)
    return d


def kernel_arithmetic(flat, feat, drop, grad_thetas):
    """What hpe_regressor_backward computes, in numpy float64: -> (flat gradient, grad_features)"""
    p = {k: v.astype(np.float64) for k, v in regressor_spec.flat_to_params(np.asarray(flat)).items()}
    W1, b1, W2, b2, W3, b3, mean = (p[k] for k in KEYS)
    f = np.asarray(feat, np.float64)
    B = f.shape[0]
    ext = np.asarray(grad_thetas, np.float64)
    ones = np.ones((2, B, 1024))
    th = [np.tile(mean[None], (B, 1))]
    A1, A2 = [], []
    P1 = f @ W1[:2048]  # hoisted
    for i in range(S):
        d = np.asarray(drop, np.float64) if (drop is not None and i == S - 1) else ones
        a1 = d[0] * np.maximum(P1 + th[i] @ W1[2048:] + b1, 0.0)
        a2 = d[1] * np.maximum(a1 @ W2 + b2, 0.0)
        th.append(th[i] + a2 @ W3 + b3)
        A1.append(a1)
        A2.append(a2)
    G = [np.zeros((B, 85))] + [ext[i].copy() for i in range(S)]  # G[i + 1]: cotangent of theta_i
    DZ1, DZ2 = [None] * S, [None] * S
    sum1 = None
    for i in range(S - 1, -1, -1):
        d = np.asarray(drop, np.float64) if (drop is not None and i == S - 1) else ones
        DZ2[i] = (G[i + 1] @ W3.T) * d[1] * (A2[i] > 0)
        DZ1[i] = (DZ2[i] @ W2.T) * d[0] * (A1[i] > 0)
        sum1 = DZ1[i] if sum1 is None else sum1 + DZ1[i]
        G[i] = (G[i + 1] + G[i]) + DZ1[i] @ W1[2048:].T
    st = np.concatenate
    TH, D1, D2, D3 = st(th[:S]), st(DZ1), st(DZ2), st(G[1:])
    dW1 = np.concatenate([f.T @ sum1, TH.T @ D1])
    g = np.concatenate([dW1.reshape(-1), D1.sum(0), (st(A1).T @ D2).reshape(-1), D2.sum(0), (st(A2).T @ D3).reshape(-1), D3.sum(0), G[0].sum(0)])
    return g, sum1 @ W1[:2048].T


def per_tensor_errors(got_flat, want_flat, got_f=None, want_f=None):
    """-> [(name, worst absolute error / largest reference magnitude)] over the seven parameter tensors (and grad_features)"""
    out = []
    for key, off, shape in regressor_spec.flat_layout():
        n = int(np.prod(shape))
        a, b = np.asarray(got_flat[off : off + n], np.float64), np.asarray(want_flat[off : off + n], np.float64)
        assert np.isfinite(a).all(), key
        out.append((key, float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))))
    if want_f is not None:
        a, b = np.asarray(got_f, np.float64), np.asarray(want_f, np.float64)
        out.append(("grad_features", float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))))
    return out


# ---- the fixture of tests/test_gpu_regressor_train.py (checked on the CPU by tests/test_regressor_train_cpu.py)
POOL_ROWS, POOL_SEED, DROP_SEED = 512, 4100, 4200
BATCHES = (1, 3, 4, 5, 64, 65)
_POOL = {}


def pool():
    """-> dict(flat, feat [n,2048], drop [2,n,1024], generated, kept): POOL_ROWS generated feature rows minus those with a float64
    pre-activation within KINK of 0, with or without the fixture's dropout masks (the masks are drawn per generated row and filtered
    with it).  Computed once, never modified."""
    if not _POOL:
        params, mean = fixture_params()
        flat = flat_of(params, mean)
        feat, drop = make_features(POOL_ROWS, POOL_SEED), make_drop(POOL_ROWS, DROP_SEED)
        keep = kink_distance(flat, feat, drops=(None, drop)) > KINK
        _POOL.update(flat=flat, feat=np.ascontiguousarray(feat[keep]), drop=np.ascontiguousarray(drop[:, keep]), generated=POOL_ROWS,
                     kept=int(keep.sum()), params=params, mean=mean)
    return _POOL


def case(B, with_drop, last_only, seed=None):
    """inputs of one backward case on the first B pool rows: (feat, drop or None, grad_thetas [S,B,85])"""
    P = pool()
    g = np.random.Generator(np.random.Philox(int(5000 + B if seed is None else seed)))
    gt = g.normal(0, 1, (S, B, 85)).astype(np.float32)
    if last_only:
        gt[: S - 1] = 0.0
    return P["feat"][:B], (np.ascontiguousarray(P["drop"][:, :B]) if with_drop else None), gt


# ---- the generator step as a torch loop (tests/test_gpu_regressor_train.py::test_training)
def kp_loss(kp_gt, kp_pred):
    """kp_reprojection_loss (src/ops.py:35-47): sum(vis * |d|) / (2 * #visible)"""
    vis = kp_gt[:, :, 2:3]
    return (vis * (kp_gt[:, :, :2] - kp_pred).abs()).sum() / (2.0 * (vis > 0).sum())


def generator_loop(flat, feat, kp_gt, drop, smpl_model, critic_params, steps, lr, dtype, kpr_w=60.0, critic_w=0.01):
    """``steps`` Adam steps (Keras' epsilon) on kpr_w * kp loss + critic_w * critic term of the LAST stage, the same ``drop`` every step
    -> (losses [steps, 2] = (weighted kp loss, weighted critic term) before each step, the trained flat vector)"""
    from critic_ref import CriticTorch
    from smpl_torch_ref import SmplTorch

    P = tensors(flat, dtype)
    opt = torch.optim.Adam([P[k] for k in KEYS], lr=lr, betas=(0.9, 0.999), eps=1e-7)
    smpl, critic = SmplTorch(smpl_model, dtype), CriticTorch(critic_params, dtype)
    f, d, gt = as_t(feat, dtype), as_t(drop, dtype), as_t(kp_gt, dtype)
    out = []
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        th, _ = ief(P, f, d)
        o = smpl(th[-1])
        kp = kpr_w * kp_loss(gt, o["kp2d"])
        gc = critic_w * -critic(o["joints"], th[-1][:, 75:], o["Rs"]).mean(0).sum()
        out.append([float(kp.detach()), float(gc.detach())])
        (kp + gc).backward()
        opt.step()
    return np.asarray(out, np.float64), np.concatenate([P[k].detach().reshape(-1).numpy() for k in KEYS])
