"""CPU-side checks of critic training: the gradient penalty against the reference's four-term formula, the flat parameter layout
against critic_spec / critic_ref.LAYERS / the library's offsets, and -- in float64 -- the identity the GPU path relies on: the weight
gradient of the literal loss (WGAN term + 10 * penalty, torch double backward) equals dF/dW of the functional F that
hpe_critic_weight_grad differentiates, with grad_scores -1/N, +1/N on the real and fake rows and, on the interpolated rows, the tangents
v_i = 10 * (-2 (1 - ||m_i||) / ||m_i||) * m_i / N shared by all rows."""
import numpy as np
import torch

import hpe_amd
from hpe_amd import critic_spec, synthetic

import critic_ref as R
import critic_train_ref as T
from smpl_torch_ref import SmplTorch


def rel(got, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / np.abs(ref).max())


def make_rows(N, seed):
    """float64 torch (joints [N,14,3], betas [N,10], Rs [N,24,3,3]) of synthetic thetas through the float64 SMPL restatement"""
    th = torch.from_numpy(synthetic.make_thetas(N, seed=seed)).to(torch.float64)
    o = SmplTorch(synthetic.make_smpl_model(), torch.float64)(th)
    return o["joints"][:, :14].detach(), th[:, 75:].clone(), o["Rs"].detach()


def test_gradient_penalty_matches_literal_formula():
    g = torch.Generator().manual_seed(3)
    grads = [torch.randn((17,) + s, generator=g, dtype=torch.float64) * 0.3 for s in ((13, 13), (14, 3), (10,), (24, 3, 3))]
    want = sum((1.0 - np.linalg.norm(x.numpy().mean(0).reshape(-1))) ** 2 for x in grads)
    got = hpe_amd.critic_gradient_penalty(grads)
    assert abs(float(got) - want) <= 1e-14 * abs(want)
    assert abs(float(T.penalty_literal(grads)) - want) <= 1e-14 * abs(want)
    x = [t.clone().requires_grad_(True) for t in grads]  # differentiable: plain torch
    hpe_amd.critic_gradient_penalty(x).backward()
    assert all(t.grad is not None and torch.isfinite(t.grad).all() for t in x)
    f32 = hpe_amd.critic_gradient_penalty([t.float() for t in grads])
    assert f32.dtype == torch.float32 and abs(float(f32) - want) <= 1e-5 * abs(want)


def test_flat_layout():
    layout = critic_spec.flat_layout()
    assert len(layout) == 18
    off = 0
    for i, (name, fi, fo, _act) in enumerate(R.LAYERS):
        (kk, ko, ks), (bk, bo, bs) = layout[2 * i], layout[2 * i + 1]
        assert (kk, ko, ks) == ("critic/%s/kernel" % name, off, (fi, fo))
        assert (bk, bo, bs) == ("critic/%s/bias" % name, off + fi * fo, (fo,))
        off += fi * fo + fo
    assert off == critic_spec.PARAM_FLOATS == 114273
    # the library's table (host code: runs without a GPU)
    from hpe_amd import _lib, build as hbuild

    hbuild.build()
    lib = _lib.load()
    assert lib.hpe_critic_param_floats() == critic_spec.PARAM_FLOATS
    for i in range(9):
        assert lib.hpe_critic_layer_name(i).decode() == R.LAYERS[i][0]
        assert lib.hpe_critic_param_offset(i, 0) == layout[2 * i][1] and lib.hpe_critic_param_offset(i, 1) == layout[2 * i + 1][1]
    assert lib.hpe_critic_param_offset(9, 0) == -1 and lib.hpe_critic_param_offset(-1, 1) == -1
    assert lib.hpe_critic_weight_grad_ws_floats(0) == 0 and lib.hpe_critic_weight_grad_ws_floats(1) >= 1043 + 618 + 3
    # dict <-> flat, both ways
    p = synthetic.make_critic_params(seed=6)
    flat = critic_spec.params_to_flat(p)
    assert flat.dtype == np.float32 and flat.shape == (critic_spec.PARAM_FLOATS,)
    k = p["critic/rotation_dense_1/kernel"]
    o = lib.hpe_critic_param_offset(6, 0)
    assert flat[o + 5 * 300 + 7] == k[5, 7]  # kernels are [in, out], row-major
    back = critic_spec.flat_to_params(torch.from_numpy(flat))
    assert sorted(back) == sorted(p)
    for key in p:
        assert back[key].dtype == np.float32 and np.array_equal(back[key], p[key]), key
    assert np.array_equal(critic_spec.params_to_flat(back), flat)


def test_penalty_weight_gradient_is_a_tangent_term():
    N = 96
    params = synthetic.make_critic_params(seed=6)
    real, fake = make_rows(N, seed=11), make_rows(N, seed=12)
    g = torch.Generator().manual_seed(13)
    interp = tuple(torch.rand(t.shape, generator=g, dtype=torch.float64) for t in fake)
    # the literal loss and its weight gradient by double backward
    net = T.net_with_weight_grad(params)
    lit = T.wgan_loss(net, real, fake, interp)
    want = T.weight_grad(net, lit["loss"])
    # the decomposition: first-order term on real and fake rows, tangent term on the interpolated rows
    pre = R.critic_np(params, *(t.detach().numpy() for t in lit["rows"]))["pre"]
    print("interpolated rows: smallest distance to a kink %.3g" % R.kink_distance(pre).min())
    tangents = {}
    for k in T.ORDER:
        m = lit["g"][k].detach().mean(0)
        n = m.norm()
        tangents[k] = 10.0 * (-2.0 * (1.0 - n) / n) * m / N
    ones = torch.full((N, 3), 1.0 / N, dtype=torch.float64)
    net2 = T.net_with_weight_grad(params)
    F = (T.functional(net2, *real, grad_scores=-ones) + T.functional(net2, *fake, grad_scores=ones)
         + T.functional(net2, *(t.detach() for t in lit["rows"]), tangents=tangents))
    got = T.weight_grad(net2, F)
    worst = 0.0
    for key, off, shape in critic_spec.flat_layout():
        n = int(np.prod(shape))
        a, b = got[off : off + n], want[off : off + n]
        assert np.abs(b).max() > 0 or key.endswith("_3/bias") or key.endswith("combined_dense/bias"), key
        e = float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))
        worst = max(worst, e)
        assert e <= 1e-12, (key, e)
    print("weight gradient of the literal loss vs dF/dW: worst %.3g" % worst)
    # equal real and fake counts: the WGAN term gives the three output biases exactly 0, and the tangent term gives every bias exactly 0
    only_t = T.weight_grad(net2, T.functional(net2, *(t.detach() for t in lit["rows"]), tangents=tangents))
    for key, off, shape in critic_spec.flat_layout():
        if key.endswith("/bias"):
            assert not only_t[off : off + shape[0]].any(), key
