"""GPU tests of the critic (run with -m gpu on an MI355X): hpe_critic / hpe_critic_backward against the float64 restatement of
get_kcs + CriticNetwork (tests/critic_ref.py) and its autograd, bit-level repeatability and row independence, the autograd wiring
through hpe_smpl_backward, Predictor.val_step, fit_reprojection and graph capture.

Inputs are hpe_smpl outputs for ``synthetic.make_thetas`` rows plus adversarial rows (all-zero joints; identity rotations; betas that
drive every ReLU of the shapes branch negative).  Bar, the project's fp32 parity bar: per tensor, worst absolute error / largest
reference magnitude <= 1e-4.

The gradient of a (leaky) ReLU network jumps where a pre-activation crosses 0, so a row whose float64 pre-activation lies within
2e-6 of 0 in any of the six layers with a kink has no gradient that fp32 could match: fp32 accumulation of <= 300 terms of this size
moves a pre-activation by up to ~1e-6 and may put it on the other side.  Such rows (decided by the float64 reference alone; about
1e-5 of the pre-activations) are left out of the comparison with THE reference gradient, at least 99 % of the rows must remain, and
each row left out must still match, to the same bar and in all four gradients at once, one of the one-sided reference gradients: the
float64 gradient with its near-kink units put on one side or the other (every combination, at most 3 such units in a row).

Measured on an MI355X (worst over N in {1, 3, 64, 257, 768} and K in {14, 19}): scores 9.0e-7, kcs 1.4e-7, grad_joints 4.0e-7,
grad_betas 1.1e-7, grad_Rs 8.0e-7, grad_kcs 4.2e-7; at most 4 of 768 rows within 2e-6 of a kink."""
import numpy as np
import pytest
import torch

import hpe_amd
from hpe_amd import synthetic

import critic_ref as R
from smpl_torch_ref import SmplTorch

pytestmark = pytest.mark.gpu
TOL = 1e-4
KINK = 2e-6
MAX_BATCH = 128


def critic_params():
    """synthetic weights; shapes_dense_2's biases are made negative so that betas CAN switch the whole shapes branch off"""
    p = synthetic.make_critic_params(seed=6)
    p["critic/shapes_dense_2/bias"] = -np.abs(p["critic/shapes_dense_2/bias"]) - np.float32(0.01)
    return p


@pytest.fixture(scope="module")
def params():
    return critic_params()


@pytest.fixture(scope="module")
def model():
    return synthetic.make_smpl_model()


@pytest.fixture(scope="module")
def engine(model, params):
    e = hpe_amd.HpeEngine(device=0, max_batch=MAX_BATCH)
    e.load_smpl(model)
    assert not e.has_critic
    with pytest.raises(hpe_amd.HpeError, match="no critic loaded"):
        z = torch.zeros((1, 14, 3), device="cuda")
        e.critic(z, torch.zeros((1, 10), device="cuda"), torch.zeros((1, 24, 3, 3), device="cuda"))
    e.load_critic(synthetic.make_critic_params(seed=1))  # before finalize ...
    e.finalize()
    e.load_critic(params)  # ... and after: loading again replaces the weights
    assert e.has_critic
    yield e
    e.close()
    assert not e.has_critic


def dead_betas(params):
    """betas with shapes_dense_1's pre-activations all equal to -1"""
    W1 = params["critic/shapes_dense_1/kernel"].astype(np.float64)
    b1 = params["critic/shapes_dense_1/bias"].astype(np.float64)
    return np.linalg.solve(W1.T, -1.0 - b1).astype(np.float32)


def make_inputs(engine, params, N, K, seed):
    """-> (joints [N,K,3], betas [N,10], Rs [N,24,3,3]) CUDA tensors, adversarial rows included when N >= 3"""
    theta = torch.from_numpy(synthetic.make_thetas(N, seed=seed)).cuda()
    joints, Rs = [], []
    for lo in range(0, N, MAX_BATCH):
        o = engine.smpl(theta[lo : lo + MAX_BATCH], want=("joints", "Rs"))
        joints.append(o["joints"])
        Rs.append(o["Rs"])
    joints, Rs = torch.cat(joints)[:, :K].contiguous(), torch.cat(Rs).contiguous()
    betas = theta[:, 75:].contiguous()
    if N >= 3:
        joints[1] = 0.0
        Rs[2] = torch.eye(3, device="cuda")
        betas[2] = torch.from_numpy(dead_betas(params)).cuda()
    if N >= 4:
        Rs[3] = torch.eye(3, device="cuda")
        joints[3] = 0.0
    return joints, betas, Rs


def rel(got, ref):
    """worst absolute error / largest reference magnitude"""
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / np.abs(ref).max())


def ref_gradients(params, joints, betas, Rs, gs, side=None):
    """float64 autograd of the restatement -> dict(joints (total), betas, Rs, kcs (partial, KCS as an independent input))"""
    net = R.CriticTorch(params, torch.float64)
    j, b, r = (torch.from_numpy(np.asarray(a, np.float64)).requires_grad_(True) for a in (joints, betas, Rs))
    gs = torch.from_numpy(np.asarray(gs, np.float64))
    gj, gb, gr = torch.autograd.grad((net(j, b, r, side=side) * gs).sum(), [j, b, r])
    k = net.kcs(j).detach().requires_grad_(True)
    (gk,) = torch.autograd.grad((net(j, b, r, kcs=k, side=side) * gs).sum(), [k])
    return dict(joints=gj.numpy(), betas=gb.numpy(), Rs=gr.numpy(), kcs=gk.numpy())


def one_sided_error(params, pre, i, jn, bn, rn, gs_row, got_row, scale):
    """row i lies within KINK of a kink: the smallest, over the 2^n placements of its n near-kink units on either side, of the worst
    (over the four gradients) absolute error / ``scale[name]`` (the largest magnitude of the whole reference tensor)"""
    import itertools

    near = [(name, int(c)) for name, _i, _o, act in R.LAYERS if act is not None for c in np.nonzero(np.abs(pre[name][i]) <= KINK)[0]]
    assert 1 <= len(near) <= 3, near
    best = np.inf
    for combo in itertools.product((False, True), repeat=len(near)):
        side = {name: (pre[name][i : i + 1] > 0).copy() for name, _c in near}
        for (name, c), v in zip(near, combo):
            side[name][0, c] = v
        want = ref_gradients(params, jn[i : i + 1], bn[i : i + 1], rn[i : i + 1], gs_row, side=side)
        best = min(best, max(float(np.abs(got_row[k].astype(np.float64) - want[k][0]).max() / scale[k]) for k in want))
    return best


@pytest.mark.parametrize("K", [14, 19])
@pytest.mark.parametrize("N", [1, 3, 64, 257, 768])
def test_forward_and_gradient_accuracy(engine, params, N, K):
    joints, betas, Rs = make_inputs(engine, params, N, K, seed=100 + N + K)
    jn, bn, rn = joints.cpu().numpy(), betas.cpu().numpy(), Rs.cpu().numpy()
    ref = R.critic_np(params, jn, bn, rn)
    if N >= 64:  # both slopes of every leaky layer and both sides of every ReLU are exercised, as the reference sees them
        for name, _i, _o, act in R.LAYERS:
            if act is not None:
                assert (ref["pre"][name] > 0).any() and (ref["pre"][name] < 0).any(), name
    if N >= 3:  # row 2: every ReLU of the shapes branch is off
        assert (ref["pre"]["shapes_dense_1"][2] < 0).all() and (ref["pre"]["shapes_dense_2"][2] < 0).all()
    scores, kcs = engine.critic(joints, betas, Rs, want_kcs=True)
    assert torch.equal(scores, engine.critic(joints, betas, Rs))
    e_s, e_k = rel(scores.cpu().numpy(), ref["scores"]), rel(kcs.cpu().numpy(), ref["kcs"])
    report = ["N=%d K=%d forward: scores %.3g kcs %.3g" % (N, K, e_s, e_k)]
    keep = R.kink_distance(ref["pre"]) > KINK
    report.append("rows away from a kink: %d of %d" % (int(keep.sum()), N))
    assert keep.mean() >= 0.99 or N < 100 and keep.sum() >= N - 1, report
    g = torch.Generator().manual_seed(7 * N + K)
    worst = max(e_s, e_k)
    for gs in (torch.randn((N, 3), generator=g), None):
        want = ref_gradients(params, jn, bn, rn, np.ones((N, 3)) if gs is None else gs.numpy())
        got = engine.critic_backward(joints, betas, Rs, None if gs is None else gs.cuda(), want=("joints", "betas", "Rs", "kcs"))
        for name in ("joints", "betas", "Rs", "kcs"):
            a = got[name].cpu().numpy()
            assert np.isfinite(a).all()
            e = rel(a[keep], want[name][keep])
            report.append("grad_%-6s (%s grad_scores) %.3g" % (name, "ones " if gs is None else "random", e))
            worst = max(worst, e)
        for i in np.nonzero(~keep)[0]:  # rows at a kink: one of the one-sided reference gradients, same bar
            e = one_sided_error(params, ref["pre"], int(i), jn, bn, rn, np.ones((1, 3)) if gs is None else gs.numpy()[i : i + 1],
                                {k: got[k][i].cpu().numpy() for k in got}, {k: np.abs(want[k]).max() for k in want})
            report.append("row %d at a kink: one-sided gradients %.3g" % (i, e))
            worst = max(worst, e)
        assert float(got["joints"][:, 14:].abs().max() if K > 14 else 0.0) == 0.0
        assert float(got["Rs"][:, 0].abs().max()) == 0.0
        if N >= 3:
            assert float(got["betas"][2].abs().max()) == 0.0  # the dead shapes branch passes nothing back
        # NULL outputs are skipped: every single output alone gives the same bits
        for name in ("joints", "betas", "Rs", "kcs"):
            one = engine.critic_backward(joints, betas, Rs, None if gs is None else gs.cuda(), want=(name,))
            assert list(one) == [name] and torch.equal(one[name].view(torch.int32), got[name].view(torch.int32)), name
    msg = "\n".join(report)
    print(msg)
    assert worst <= TOL, msg


def test_errors(engine):
    z = lambda *s: torch.zeros(s, device="cuda")  # noqa: E731
    with pytest.raises(ValueError):
        engine.critic(z(2, 13, 3), z(2, 10), z(2, 24, 3, 3))
    with pytest.raises(ValueError):
        engine.critic(z(2, 14, 3), z(3, 10), z(2, 24, 3, 3))
    with pytest.raises(ValueError):
        engine.critic_backward(z(2, 14, 3), z(2, 10), z(2, 24, 3, 3), want=())
    lib, h = engine.lib, engine._h
    j, b, r, s = z(2, 14, 3), z(2, 10), z(2, 24, 3, 3), z(2, 3)
    assert lib.hpe_critic(h, j.data_ptr(), 13, b.data_ptr(), 10, r.data_ptr(), 2, s.data_ptr(), None, None) == 1
    assert lib.hpe_critic(h, j.data_ptr(), 25, b.data_ptr(), 10, r.data_ptr(), 2, s.data_ptr(), None, None) == 1
    assert lib.hpe_critic(h, j.data_ptr(), 14, b.data_ptr(), 9, r.data_ptr(), 2, s.data_ptr(), None, None) == 1
    assert lib.hpe_critic(h, j.data_ptr(), 14, b.data_ptr(), 10, r.data_ptr(), 0, s.data_ptr(), None, None) == 1
    assert lib.hpe_critic(h, j.data_ptr(), 14, b.data_ptr(), 10, r.data_ptr(), 2, None, None, None) == 1
    assert lib.hpe_critic_backward(h, j.data_ptr(), 14, b.data_ptr(), 10, r.data_ptr(), 2, None, None, None, None, None, None) == 1
    assert b"every output is NULL" in lib.hpe_last_error()


def test_load_twice_replaces(engine, params):
    """load_critic(Q) then load_critic(P) on one context leaves what load_critic(P) alone leaves, bit for bit: the scores, the input
    gradients (the only readers of the transposed kernels) and critic_params().  N = 5 is two row tiles, the second partial."""
    N, K = 5, 14
    joints, betas, Rs = make_inputs(engine, params, N, K, seed=95)
    names = ("joints", "betas", "Rs", "kcs")
    twice, once = hpe_amd.HpeEngine(device=0, max_batch=8), hpe_amd.HpeEngine(device=0, max_batch=8)
    try:
        twice.load_critic(synthetic.make_critic_params(seed=2))
        s_q = twice.critic(joints, betas, Rs).clone()
        twice.load_critic(params)
        once.load_critic(params)
        s2, s1 = twice.critic(joints, betas, Rs), once.critic(joints, betas, Rs)
        assert not torch.equal(s_q, s2)  # Q is another critic
        assert torch.equal(s2.view(torch.int32), s1.view(torch.int32))
        g2, g1 = twice.critic_backward(joints, betas, Rs, want=names), once.critic_backward(joints, betas, Rs, want=names)
        for k in names:
            assert torch.equal(g2[k].view(torch.int32), g1[k].view(torch.int32)), k
        assert torch.equal(twice.critic_params().view(torch.int32), once.critic_params().view(torch.int32))
    finally:
        twice.close()
        once.close()


def test_bitwise_repeatable(engine, params):
    N = 300
    joints, betas, Rs = make_inputs(engine, params, N, 19, seed=31)
    gs = torch.randn((N, 3), generator=torch.Generator().manual_seed(32)).cuda()
    s0 = engine.critic(joints, betas, Rs).clone()
    g0 = {k: v.clone() for k, v in engine.critic_backward(joints, betas, Rs, gs, want=("joints", "betas", "Rs", "kcs")).items()}
    other = make_inputs(engine, params, 77, 14, seed=33)
    engine.critic(*other)
    engine.critic_backward(*other)
    assert torch.equal(s0.view(torch.int32), engine.critic(joints, betas, Rs).view(torch.int32))
    g1 = engine.critic_backward(joints, betas, Rs, gs, want=("joints", "betas", "Rs", "kcs"))
    for k in g0:
        assert torch.equal(g0[k].view(torch.int32), g1[k].view(torch.int32)), k


def test_row_independence(engine, params):
    """row i of an N = 768 call equals, bit for bit, the N = 1 call on that row: scores, kcs and the four gradients, every row"""
    N, K = 768, 19
    joints, betas, Rs = make_inputs(engine, params, N, K, seed=41)
    gs = torch.randn((N, 3), generator=torch.Generator().manual_seed(42)).cuda()
    names = ("joints", "betas", "Rs", "kcs")
    scores, kcs = engine.critic(joints, betas, Rs, want_kcs=True)
    grads = engine.critic_backward(joints, betas, Rs, gs, want=names)
    s1, k1 = torch.empty_like(scores), torch.empty_like(kcs)
    g1 = {k: torch.empty_like(v) for k, v in grads.items()}
    for i in range(N):
        a, b = engine.critic(joints[i : i + 1], betas[i : i + 1], Rs[i : i + 1], want_kcs=True)
        s1[i], k1[i] = a[0], b[0]
        g = engine.critic_backward(joints[i : i + 1], betas[i : i + 1], Rs[i : i + 1], gs[i : i + 1], want=names)
        for k in names:
            g1[k][i] = g[k][0]
    assert torch.equal(scores.view(torch.int32), s1.view(torch.int32)) and torch.equal(kcs.view(torch.int32), k1.view(torch.int32))
    for k in names:
        assert torch.equal(grads[k].view(torch.int32), g1[k].view(torch.int32)), k
    # ... and a row's result does not depend on its slot in a tile: the same rows shifted by one
    s2 = engine.critic(joints[1:], betas[1:], Rs[1:])
    assert torch.equal(s2.view(torch.int32), scores[1:].contiguous().view(torch.int32))


def test_strided_betas(engine, params):
    """betas read in place from a theta tensor (row stride 85) equal dense betas bit for bit, and no copy is made"""
    N = 130
    joints, betas, Rs = make_inputs(engine, params, N, 19, seed=51)
    theta = torch.randn((N, 85), device="cuda")
    theta[:, 75:] = betas
    view = theta[:, 75:]
    assert not view.is_contiguous()
    j, b, r, n, k, stride = engine._critic_inputs(joints, view, Rs)
    assert stride == 85 and b.data_ptr() == view.data_ptr()
    assert torch.equal(engine.critic(joints, view, Rs).view(torch.int32), engine.critic(joints, betas, Rs).view(torch.int32))
    ga, gb = engine.critic_backward(joints, view, Rs), engine.critic_backward(joints, betas, Rs)
    for name in ga:
        assert ga[name].is_contiguous() and torch.equal(ga[name].view(torch.int32), gb[name].view(torch.int32)), name


def test_autograd_wiring(engine, model, params):
    """generator_critic_loss(...).backward() on a theta that requires grad, through hpe_critic_backward and hpe_smpl_backward, against
    float64 autograd of restatement o SmplTorch; the camera columns get exactly 0 (the critic never sees the camera)."""
    N = 24
    th = synthetic.make_thetas(N, seed=61)
    theta = torch.from_numpy(th).cuda().requires_grad_(True)
    out = engine.smpl(theta, want=("joints", "Rs"))
    loss = hpe_amd.generator_critic_loss(engine, out["joints"], theta[:, 75:], out["Rs"])
    assert loss.grad_fn is not None
    loss.backward()
    x = torch.from_numpy(th).to(torch.float64).requires_grad_(True)
    o = SmplTorch(model, torch.float64)(x)
    sc = R.CriticTorch(params, torch.float64)(o["joints"], x[:, 75:], o["Rs"])
    ref_loss = -sc.mean(0).sum()
    ref_loss.backward()
    pre = R.critic_np(params, o["joints"].detach().numpy(), th[:, 75:], o["Rs"].detach().numpy())["pre"]
    keep = R.kink_distance(pre) > KINK
    assert keep.sum() >= N - 1
    got, want = theta.grad.cpu().numpy(), x.grad.numpy()
    e_l, e_g = abs(float(loss.detach()) - float(ref_loss.detach())) / abs(float(ref_loss.detach())), rel(got[keep], want[keep])
    print("autograd wiring: loss rel %.3g, theta.grad %.3g" % (e_l, e_g))
    assert e_l <= TOL and e_g <= TOL
    assert float(theta.grad[:, :3].abs().max()) == 0.0
    # without requires_grad: the plain call, same bits, no graph
    with torch.no_grad():
        plain = hpe_amd.critic_scores(engine, out["joints"], theta[:, 75:], out["Rs"])
    sc2 = hpe_amd.critic_scores(engine, out["joints"].detach(), theta.detach()[:, 75:], out["Rs"].detach())
    assert plain.grad_fn is None and sc2.grad_fn is None and torch.equal(plain, sc2)
    parts = hpe_amd.generator_critic_loss(engine, out["joints"].detach(), theta.detach()[:, 75:], out["Rs"].detach(), return_parts=True)
    assert tuple(parts.shape) == (4,) and float(parts[3]) == N and torch.equal(parts[:3], sc2.sum(0))


class _Cfg(object):
    img_size, num_stage, batch_size, data_format = 224, 3, 3, "NHWC"
    checkpoint_dir = smpl_model_path = None


def test_val_step(model, params):
    kw = dict(smpl_model=model, mean_params=synthetic.make_mean_params(), encoder_params=synthetic.make_encoder_params(),
              regressor_params=synthetic.make_regressor_params())
    p = hpe_amd.Predictor(_Cfg(), critic_params=params, **kw)
    img = synthetic.make_images(3, seed=71)
    seg, kp_gt = synthetic.make_lsp_targets(3, seed=72)
    base = p.val_step(img, seg, kp_gt)
    assert "generator_critic_losses" not in base and "critic_parts" not in base
    calls = []

    def reduce_fn(t):
        calls.append(tuple(t.shape))
        return t

    r = p.val_step(img, seg, kp_gt, critic_loss_weight=0.01, reduce_fn=reduce_fn)
    assert calls == [(3, 8)]  # one block, so one collective per step
    assert sorted(set(r) - set(base)) == ["critic_parts", "generator_critic_losses"]
    for k, v in base.items():  # every other key is bit-equal
        for a, b in zip(v if isinstance(v, list) else [v], r[k] if isinstance(v, list) else [r[k]]):
            assert torch.equal(a, b), k
    stages = p.engine.forward(torch.from_numpy(img).cuda(), all_stages=True, want=("joints", "theta", "Rs"))
    assert tuple(r["critic_parts"].shape) == (3, 4) and len(r["generator_critic_losses"]) == 3
    for i, st in enumerate(stages):
        sc = R.critic_np(params, st["joints"].cpu().numpy(), st["theta"][:, 75:].cpu().numpy(), st["Rs"].cpu().numpy())["scores"]
        want = 0.01 * -sc.mean(0).sum()
        got = float(r["generator_critic_losses"][i])
        print("val_step stage %d: critic loss %.6g, restatement %.6g" % (i, got, want))
        assert abs(got - want) <= TOL * abs(want)
        assert float(r["critic_parts"][i, 3]) == 3.0
    # the project's own reduce function (what ShardedPredictor.val_step passes) leaves the critic's columns as sums, in and out of a
    # process group of one rank, and a step still issues no second collective
    from hpe_amd import distributed as D

    for fn in (D.reduce_losses, D.reduce_sum):
        rr = p.val_step(img, seg, kp_gt, critic_loss_weight=0.01, reduce_fn=fn)
        assert torch.equal(rr["critic_parts"], r["critic_parts"]), fn.__name__
        for a, b in zip(rr["generator_critic_losses"], r["generator_critic_losses"]):
            assert torch.equal(a, b), fn.__name__
    rs = D.ShardedPredictor(p).val_step(img, seg, kp_gt, critic_loss_weight=0.01)
    for i, st in enumerate(stages):
        sc = R.critic_np(params, st["joints"].cpu().numpy(), st["theta"][:, 75:].cpu().numpy(), st["Rs"].cpu().numpy())["scores"]
        want = 0.01 * -sc.mean(0).sum()
        assert abs(float(rs["generator_critic_losses"][i]) - want) <= TOL * abs(want), (i, float(rs["generator_critic_losses"][i]), want)
        assert torch.allclose(rs["kpr_losses"][i], base["kpr_losses"][i], rtol=1e-6, atol=0.0)  # column 2 is re-divided by reduce_losses
        assert torch.equal(rs["mr_losses"][i], base["mr_losses"][i])
    assert tuple(rs["loss_parts"].shape) == (3, 4) and torch.equal(rs["loss_parts"][:, [0, 1, 3]], base["loss_parts"][:, [0, 1, 3]])
    q = hpe_amd.Predictor(_Cfg(), **kw)
    assert not q.engine.has_critic
    with pytest.raises(RuntimeError, match="critic"):
        q.val_step(img, seg, kp_gt, critic_loss_weight=0.01)


def test_fit_reprojection(engine, params, monkeypatch):
    B, steps = 4, 5
    th = synthetic.make_thetas(B, seed=81)
    theta0 = torch.from_numpy(th).cuda()
    with torch.no_grad():
        kp = engine.smpl(torch.from_numpy(synthetic.make_thetas(B, seed=82)).cuda(), want=("kp2d",))["kp2d"]
    kp_gt = torch.cat([kp, torch.ones((B, kp.shape[1], 1), device="cuda")], 2)
    seg, _ = synthetic.make_lsp_targets(B, seed=83)
    seg = torch.from_numpy(seg).cuda()
    t0, l0 = hpe_amd.fit_reprojection(engine, theta0, kp_gt, seg, steps=steps)
    t0b, l0b = hpe_amd.fit_reprojection(engine, theta0, kp_gt, seg, steps=steps, critic_weight=0.0)
    assert tuple(l0.shape) == (steps, 2) and torch.equal(t0, t0b) and torch.equal(l0, l0b)
    # the loop with the prior reads nothing from the device: every host read of a CUDA tensor goes through one of these
    def guarded(orig):
        def call(self, *a, **k):
            if self.is_cuda:
                raise AssertionError("the fit loop read the device")
            return orig(self, *a, **k)  # the optimiser's own step counters live on the host

        return call

    for name in ("item", "cpu", "tolist", "numpy", "__bool__", "__float__", "__int__"):
        monkeypatch.setattr(torch.Tensor, name, guarded(getattr(torch.Tensor, name)))
    t1, l1 = hpe_amd.fit_reprojection(engine, theta0, kp_gt, seg, steps=steps, critic_weight=0.01)
    monkeypatch.undo()
    assert tuple(l1.shape) == (steps, 3) and tuple(t1.shape) == (B, 85) and torch.isfinite(l1).all() and torch.isfinite(t1).all()
    assert torch.equal(l1[0, :2], l0[0, :2])  # the first step's reprojection terms see the same theta
    out = engine.smpl(theta0, want=("joints", "Rs"))
    first = hpe_amd.generator_critic_loss(engine, out["joints"], theta0[:, 75:], out["Rs"])
    assert torch.equal(first, l1[0, 2])
    assert not torch.equal(t1, t0)  # the prior moves the solution
    with pytest.raises(ValueError):
        hpe_amd.fit_reprojection(engine, theta0, kp_gt, seg, steps=1, critic_weight=-1.0)


def test_graph_capture(engine, params):
    """forward + backward captured into one graph and replayed give the bits of the eager calls"""
    N = 96
    joints, betas, Rs = make_inputs(engine, params, N, 19, seed=91)
    gs = torch.randn((N, 3), generator=torch.Generator().manual_seed(92)).cuda()
    names = ("joints", "betas", "Rs", "kcs")
    s_e = engine.critic(joints, betas, Rs).clone()
    g_e = {k: v.clone() for k, v in engine.critic_backward(joints, betas, Rs, gs, want=names).items()}
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s_g = engine.critic(joints, betas, Rs)
        g_g = engine.critic_backward(joints, betas, Rs, gs, want=names)
    s_g.zero_()
    for v in g_g.values():
        v.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(s_g.view(torch.int32), s_e.view(torch.int32))
    for k in names:
        assert torch.equal(g_g[k].view(torch.int32), g_e[k].view(torch.int32)), k
