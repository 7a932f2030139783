"""Float64 torch restatement of the critic update of the reference's Trainer.train_step (src/trainer.py:511-583) with the gradient
penalty of src/ops.py:153-172, on top of ``critic_ref.CriticTorch``: the yardstick of the critic-training tests.

    loss = sum_c mean_n(fake[n,c] - real[n,c]) + gp_weight * penalty
    penalty = sum over the four inputs i of (1 - || mean_n g_i[n] ||_2)^2
    g = d(sum_{n,c} scores[n,c]) / d[kcs, joints, shapes, Rs] at the rows fake + U(0,1) * (real - fake), kcs = get_kcs(those joints)

and the functional the library's hpe_critic_weight_grad differentiates,

    F = sum_n [ sum_c gs[n,c] * scores[n,c] + sum_i < t_i[n], g_i[n] > ]

both with torch autograd (create_graph=True: the weight gradient of the penalty is a double backward)."""
import numpy as np
import torch

import critic_ref as R
from hpe_amd import critic_spec

ORDER = ("kcs", "joints", "betas", "Rs")


def net_with_weight_grad(params, dtype=torch.float64, device="cpu"):
    net = R.CriticTorch(params, dtype, device)
    # clones: torch.as_tensor shares memory with a numpy array of the same dtype, and an optimiser stepping these leaves in place would
    # otherwise rewrite the caller's float32 ``params``
    net.P = {k: v.detach().clone().requires_grad_(True) for k, v in net.P.items()}
    return net


def flat_of(net, tensors):
    """{key: tensor or None} in the net's keys -> flat numpy vector in critic_spec's layout (None = zeros)"""
    out = np.zeros(critic_spec.PARAM_FLOATS, np.float64)
    for key, off, shape in critic_spec.flat_layout():
        if tensors[key] is not None:
            out[off : off + int(np.prod(shape))] = tensors[key].detach().cpu().numpy().reshape(-1)
    return out


def weight_grad(net, value):
    keys = list(net.P)
    g = torch.autograd.grad(value, [net.P[k] for k in keys], allow_unused=True)
    return flat_of(net, dict(zip(keys, g)))


def input_gradients(net, joints, betas, Rs, create_graph=True):
    """tf.gradients(out, [kcs, joints, shapes, Rs]): kcs is the graph tensor get_kcs(joints), so its gradient is the partial one and the
    joints' the total one; Rs comes back without the root -> dict of [N,13,13], [N,14,3], [N,10], [N,23,3,3]"""
    j = joints[:, :14].detach().clone().requires_grad_(True)
    b = betas.detach().clone().requires_grad_(True)
    r = Rs.detach().clone().requires_grad_(True)
    k = net.kcs(j)
    out = net(j, b, r, kcs=k)
    gk, gj, gb, gr = torch.autograd.grad(out.sum(), [k, j, b, r], create_graph=create_graph)
    return dict(kcs=gk, joints=gj, betas=gb, Rs=gr[:, 1:])


def functional(net, joints, betas, Rs, grad_scores=None, tangents=None):
    """F above; tangents {name: [shape] (shared by all rows) or [N, shape]} for some of ORDER; all in the net's dtype"""
    F = 0.0
    if grad_scores is not None:
        F = F + (net(joints[:, :14], betas, Rs) * grad_scores).sum()
    if tangents:
        g = input_gradients(net, joints, betas, Rs)
        for k, t in tangents.items():
            F = F + (g[k] * t).sum()  # a shared tangent broadcasts over the rows
    return F


def functional_weight_grad(params, joints, betas, Rs, grad_scores=None, tangents=None):
    """numpy in, flat float64 numpy out"""
    net = net_with_weight_grad(params)
    t64 = lambda a: None if a is None else torch.as_tensor(np.asarray(a, np.float64))  # noqa: E731
    tg = {k: t64(v) for k, v in (tangents or {}).items()}
    return weight_grad(net, functional(net, t64(joints), t64(betas), t64(Rs), t64(grad_scores), tg))


def penalty_literal(grads):
    """compute_gradient_penalty as the reference writes it"""
    p1 = torch.square(1.0 - torch.linalg.vector_norm(torch.mean(grads[0], 0)))
    p2 = torch.square(1.0 - torch.linalg.vector_norm(torch.mean(grads[1], 0)))
    p3 = torch.square(1.0 - torch.linalg.vector_norm(torch.mean(grads[2], 0)))
    p4 = torch.square(1.0 - torch.linalg.vector_norm(torch.mean(grads[3], 0)))
    return p1 + p2 + p3 + p4


def wgan_loss(net, real, fake, interp, gp_weight=10.0, per_row=False):
    """-> dict(loss, wgan, penalty, g (the penalised gradients), rows (the interpolated inputs)) as graph tensors of the net's dtype"""
    jr, br, Rr = real
    jf, bf, Rf = fake
    jr, jf = jr[:, :14], jf[:, :14]
    alpha, beta, gamma = interp
    wgan = (net(jf, bf, Rf) - net(jr, br, Rr)).mean(0).sum()
    ji, bi, Ri = jf + alpha * (jr - jf), bf + beta * (br - bf), Rf + gamma * (Rr - Rf)
    g = input_gradients(net, ji, bi, Ri)
    if per_row:
        N = ji.shape[0]
        penalty = sum(torch.square(1.0 - g[k].reshape(N, -1).norm(dim=1)).mean() for k in ORDER)
    else:
        penalty = penalty_literal([g[k] for k in ORDER])
    return dict(loss=wgan + gp_weight * penalty, wgan=wgan, penalty=penalty, g=g, rows=(ji, bi, Ri))


def adam_loop(params, real, fake, interps, lr, dtype, device="cpu", betas=(0.9, 0.999), eps=1e-7, gp_weight=10.0):
    """The critic update as a plain torch loop (autograd double backward + torch.optim.Adam on the 18 tensors), one step per entry of
    ``interps`` -> (losses [steps, 3] = (loss, wgan, penalty) BEFORE each step as float64 numpy, the net after the last step)"""
    net = net_with_weight_grad(params, dtype, device)
    cast = lambda t: tuple(torch.as_tensor(np.asarray(a), dtype=dtype, device=device) for a in t)  # noqa: E731
    real, fake = cast(real), cast(fake)
    opt = torch.optim.Adam(list(net.P.values()), lr=lr, betas=betas, eps=eps)
    losses = []
    for interp in interps:
        opt.zero_grad(set_to_none=True)
        r = wgan_loss(net, real, fake, cast(interp), gp_weight)
        r["loss"].backward()
        opt.step()
        losses.append([float(r[k].detach()) for k in ("loss", "wgan", "penalty")])
    return np.asarray(losses, np.float64), net
