"""GPU tests of critic training (run with -m gpu on an MI355X): hpe_critic_weight_grad against float64 autograd of the functional F
(tests/critic_train_ref.py), bit-level repeatability, the device-side get / set of the weights, critic_wgan_loss against the float64
restatement of the reference's critic loss and its double backward, CriticTrainer against the float64 torch Adam loop, graph capture,
error codes.

Engine and inputs as in tests/test_gpu_critic.py.  Bar, the project's fp32 parity bar: for each of the 18 parameter tensors, worst
absolute error / largest reference magnitude <= 1e-4; where the reference tensor is exactly zero (every bias under a tangent-only
call, a branch no tangent reaches) the library's must be exactly zero.

A gradient summed over the rows jumps where one row's pre-activation crosses 0, so the rows are CHOSEN: rows whose float64
pre-activation lies within 2e-6 of 0 in a layer with a kink (decided by the reference alone, tests/test_gpu_critic.py's KINK) are
taken out of the generated rows before the reference and the library run; at least 99 % of the generated rows must remain.

Training: the per-step losses of 10 CriticTrainer steps must stay within 4x the deviation that the fp32 torch restatement of the same
loop shows from the float64 loop on the same data (the rule fit_keypoints is held to).  The figures measured on an MI355X are in DESIGN.md
"Critic training"."""
import numpy as np
import pytest
import torch

import hpe_amd
from hpe_amd import critic_spec, synthetic

import critic_ref as R
import critic_train_ref as T
from test_gpu_critic import critic_params, make_inputs

pytestmark = pytest.mark.gpu
TOL = 1e-4
KINK = 2e-6
MAX_BATCH = 128
POOL = 2400
CRITIC_LR = 0.0005  # the reference's critic_lr default (src/config.py:65)


@pytest.fixture(scope="module")
def params():
    return critic_params()


@pytest.fixture(scope="module")
def engine(params):
    e = hpe_amd.HpeEngine(device=0, max_batch=MAX_BATCH)
    e.load_smpl(synthetic.make_smpl_model())
    e.load_critic(params)
    e.finalize()
    yield e
    e.close()


def critic_only_engine(p):
    """a second engine that only holds a critic (valid without finalize): the tests that change weights use their own"""
    e = hpe_amd.HpeEngine(device=0, max_batch=8)
    e.load_critic(p)
    return e


def keep_mask(params, joints, betas, Rs):
    pre = R.critic_np(params, joints.cpu().numpy(), betas.cpu().numpy(), Rs.cpu().numpy())["pre"]
    return torch.from_numpy(R.kink_distance(pre) > KINK)


@pytest.fixture(scope="module")
def pool(engine, params):
    """POOL generated rows (K = 19, adversarial rows included) minus the rows at a kink -> (joints, betas, Rs) CUDA tensors"""
    joints, betas, Rs = make_inputs(engine, params, POOL, 19, seed=700)
    keep = keep_mask(params, joints, betas, Rs)
    print("rows away from a kink: %d of %d generated" % (int(keep.sum()), POOL))
    assert keep.float().mean() >= 0.99
    k = keep.cuda()
    return joints[k].contiguous(), betas[k].contiguous(), Rs[k].contiguous()


def rows(pool, N, K, start=0):
    j, b, r = pool
    assert start + N <= j.shape[0]
    return j[start : start + N, :K].contiguous(), b[start : start + N].contiguous(), r[start : start + N].contiguous()


TANGENT_SHAPES = {"kcs": (13, 13), "joints": (14, 3), "betas": (10,), "Rs": (23, 3, 3)}


def variants(N, seed):
    """[(label, grad_scores or None, tangents or None)]: random grad_scores only; tangents only, shared and per row; both; each alone"""
    g = torch.Generator().manual_seed(seed)
    gs = torch.randn((N, 3), generator=g)
    shared = {k: torch.randn(s, generator=g) for k, s in TANGENT_SHAPES.items()}
    per_row = {k: torch.randn((N,) + s, generator=g) for k, s in TANGENT_SHAPES.items()}
    out = [("grad_scores", gs, None), ("tangents shared", None, shared), ("tangents per row", None, per_row), ("both", gs, shared),
           ("both per row", gs, per_row)]
    out += [("tangent %s alone" % k, None, {k: shared[k]}) for k in TANGENT_SHAPES]
    return out


def on_gpu(t):
    return None if t is None else ({k: v.cuda() for k, v in t.items()} if isinstance(t, dict) else t.cuda())


def per_tensor_errors(got, want):
    """-> [(key, error)], error = worst absolute error / largest reference magnitude; asserts exact zeros where the reference is zero"""
    got = np.asarray(got, np.float64)
    out = []
    for key, off, shape in critic_spec.flat_layout():
        n = int(np.prod(shape))
        a, b = got[off : off + n], want[off : off + n]
        assert np.isfinite(a).all(), key
        if not b.any():
            assert not a.any(), "%s: the reference is exactly zero, the library is not" % key
            out.append((key, 0.0))
        else:
            out.append((key, float(np.abs(a - b).max() / np.abs(b).max())))
    return out


@pytest.mark.parametrize("K", [14, 19])
@pytest.mark.parametrize("N", [1, 3, 64, 257, 768, 2304])
def test_weight_gradient_accuracy(engine, params, pool, N, K):
    joints, betas, Rs = rows(pool, N, K, start=0 if N >= 4 else N)  # the adversarial rows 1-3 are in every N >= 4; N = 1 is row 1 (all-zero joints)
    jn, bn, rn = joints.cpu().numpy(), betas.cpu().numpy(), Rs.cpu().numpy()
    report, worst = [], 0.0
    for label, gs, tg in variants(N, seed=1000 + 3 * N + K):
        want = T.functional_weight_grad(params, jn, bn, rn, None if gs is None else gs.numpy(),
                                        None if tg is None else {k: v.numpy() for k, v in tg.items()})
        got = engine.critic_weight_grad(joints, betas, Rs, grad_scores=on_gpu(gs), tangents=on_gpu(tg))
        assert tuple(got.shape) == (critic_spec.PARAM_FLOATS,)
        errs = per_tensor_errors(got.cpu().numpy(), want)
        if gs is None:  # the tangent term gives exactly zero to every bias
            for key, off, shape in critic_spec.flat_layout():
                if key.endswith("/bias"):
                    assert not want[off : off + shape[0]].any() and float(got[off : off + shape[0]].abs().max()) == 0.0, key
        key, e = max(errs, key=lambda t: t[1])
        report.append("N=%d K=%d %-22s worst %.3g (%s)" % (N, K, label, e, key))
        worst = max(worst, e)
    msg = "\n".join(report)
    print(msg)
    assert worst <= TOL, msg


def test_bitwise_repeatable(engine, pool):
    N = 768
    joints, betas, Rs = rows(pool, N, 19, start=5)
    other = rows(pool, 77, 14, start=900)
    for label, gs, tg in variants(N, seed=2000):
        a = engine.critic_weight_grad(joints, betas, Rs, grad_scores=on_gpu(gs), tangents=on_gpu(tg)).clone()
        engine.critic_weight_grad(*other, grad_scores=torch.ones((77, 3), device="cuda"))
        b = engine.critic_weight_grad(joints, betas, Rs, grad_scores=on_gpu(gs), tangents=on_gpu(tg))
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), label


def test_set_critic_params(engine, params, pool):
    """after set_critic_params the forward and the input gradient give the bits of an engine that load_critic-ed the same values, and
    critic_params returns them bit for bit"""
    N = 130
    joints, betas, Rs = rows(pool, N, 19, start=11)
    gs = torch.randn((N, 3), generator=torch.Generator().manual_seed(5)).cuda()
    names = ("joints", "betas", "Rs", "kcs")
    a, b = critic_only_engine(synthetic.make_critic_params(seed=1)), critic_only_engine(params)
    try:
        flat = torch.from_numpy(critic_spec.params_to_flat(params)).cuda()
        assert torch.equal(b.critic_params().view(torch.int32), flat.view(torch.int32))
        assert not torch.equal(a.critic_params(), flat)
        assert not torch.equal(a.critic(joints, betas, Rs), b.critic(joints, betas, Rs))
        a.set_critic_params(flat)
        assert torch.equal(a.critic_params().view(torch.int32), flat.view(torch.int32))
        assert torch.equal(a.critic(joints, betas, Rs).view(torch.int32), b.critic(joints, betas, Rs).view(torch.int32))
        ga, gb = a.critic_backward(joints, betas, Rs, gs, want=names), b.critic_backward(joints, betas, Rs, gs, want=names)
        for k in names:
            assert torch.equal(ga[k].view(torch.int32), gb[k].view(torch.int32)), k
        wa, wb = a.critic_weight_grad(joints, betas, Rs, grad_scores=gs), b.critic_weight_grad(joints, betas, Rs, grad_scores=gs)
        assert torch.equal(wa.view(torch.int32), wb.view(torch.int32))
        back = critic_spec.flat_to_params(a.critic_params())
        for key in params:
            assert np.array_equal(back[key], params[key]), key
        with pytest.raises(ValueError):
            a.set_critic_params(flat[:-1])
    finally:
        a.close()
        b.close()


def wgan_case(params, pool, N, seed):
    """real, fake and uniform tensors for N rows, with the triples whose real, fake or interpolated row lies at a kink taken out (at
    least 99 % of the generated triples remain) -> (real, fake, interp) as CUDA fp32 triples"""
    G = N + max(8, N // 16)
    real, fake = rows(pool, G, 14, start=0), rows(pool, G, 14, start=1100)
    g = torch.Generator().manual_seed(seed)
    interp = tuple(torch.rand(t.shape, generator=g).cuda() for t in fake)
    inter = tuple(f + u * (r - f) for r, f, u in zip(real, fake, interp))
    keep = keep_mask(params, *inter)
    print("interpolated rows away from a kink: %d of %d generated" % (int(keep.sum()), G))
    assert keep.float().mean() >= 0.99
    idx = torch.nonzero(keep.cuda())[:N, 0]
    assert idx.numel() == N
    pick = lambda t: tuple(x[idx].contiguous() for x in t)  # noqa: E731
    return pick(real), pick(fake), pick(interp)


def to64(t):
    return tuple(x.cpu().to(torch.float64) for x in t)


@pytest.mark.parametrize("per_row", [False, True])
def test_wgan_loss(engine, params, pool, per_row):
    N = 256
    real, fake, interp = wgan_case(params, pool, N, seed=31)
    net = T.net_with_weight_grad(params)
    ref = T.wgan_loss(net, to64(real), to64(fake), to64(interp), per_row=per_row)
    want = T.weight_grad(net, ref["loss"])
    got = hpe_amd.critic_wgan_loss(engine, real, fake, interp=interp, per_row=per_row)
    report = []
    for k in ("wgan", "penalty", "loss"):
        want_k = float(ref[k].detach())
        e = abs(float(got[k]) - want_k) / abs(want_k)
        report.append("%s %.9g, float64 %.9g: %.3g" % (k, float(got[k]), want_k, e))
        assert e <= TOL, report
    errs = per_tensor_errors(got["grad"].cpu().numpy(), want)
    key, e = max(errs, key=lambda t: t[1])
    report.append("weight gradient (%s penalty) vs float64 double backward: worst %.3g (%s)" % ("per-row" if per_row else "batch-mean", e, key))
    print("\n".join(report))
    assert e <= TOL, report
    # the parts are plain sums over the rows
    assert got["N"] == N and tuple(got["wgan_sums"].shape) == (3,)
    assert abs(float(got["wgan_sums"].sum()) / N - float(ref["wgan"])) <= TOL * abs(float(ref["wgan"]))
    for k, s in zip(T.ORDER, got["grad_sums"]):
        m = ref["g"][k].detach().sum(0).numpy()
        assert np.abs(s.cpu().numpy() - m).max() <= TOL * np.abs(m).max(), k
    if not per_row:
        means = [s / N for s in got["grad_sums"]]
        pen = sum((1.0 - m.norm()) ** 2 for m in means)
        assert abs(float(pen) - float(got["penalty"])) <= 1e-6 * abs(float(got["penalty"]))
        # without the gradient: same loss, no 'grad'; and the draws come from the generator when no interp is given
        plain = hpe_amd.critic_wgan_loss(engine, real, fake, interp=interp, return_grad=False)
        assert "grad" not in plain and torch.equal(plain["loss"], got["loss"])
        g1 = hpe_amd.critic_wgan_loss(engine, real, fake, generator=torch.Generator(device="cuda").manual_seed(1))
        g2 = hpe_amd.critic_wgan_loss(engine, real, fake, generator=torch.Generator(device="cuda").manual_seed(1))
        assert torch.equal(g1["grad"].view(torch.int32), g2["grad"].view(torch.int32)) and torch.equal(g1["wgan"], got["wgan"])
        assert not torch.equal(g1["penalty"], got["penalty"])


def test_training(params, pool):
    """10 Adam steps of CriticTrainer on fixed real and fake batches against the float64 torch loop; the bound is 4x the deviation of the
    fp32 torch restatement of the same loop from the float64 loop"""
    N, steps = 256, 10
    real, fake, _ = wgan_case(params, pool, N, seed=41)
    g = torch.Generator().manual_seed(42)
    interps = [tuple(torch.rand(t.shape, generator=g) for t in fake) for _ in range(steps)]
    cpu = lambda t: tuple(x.cpu() for x in t)  # noqa: E731
    l64, net64 = T.adam_loop(params, cpu(real), cpu(fake), interps, CRITIC_LR, torch.float64)
    l32, _net32 = T.adam_loop(params, cpu(real), cpu(fake), interps, CRITIC_LR, torch.float32)
    e = critic_only_engine(params)
    try:
        favour = lambda eng: float((eng.critic(*real).mean(0) - eng.critic(*fake).mean(0)).sum())  # noqa: E731
        before = favour(e)
        tr = hpe_amd.CriticTrainer(e, lr=CRITIC_LR)
        assert torch.equal(tr.params, e.critic_params())
        got = []
        for i in range(steps):
            r = tr.step(real, fake, interp=tuple(x.cuda() for x in interps[i]))
            assert sorted(r) == ["critic_network_loss", "critic_penalty", "critic_wgan"]
            got.append([float(r["critic_network_loss"]), float(r["critic_wgan"]), float(r["critic_penalty"])])
        got = np.asarray(got, np.float64)
        after = favour(e)
        assert torch.equal(tr.params.view(torch.int32), e.critic_params().view(torch.int32))
        trained = critic_spec.flat_to_params(tr.params)
    finally:
        e.close()
    report = []
    for c, name in ((0, "critic_network_loss"), (2, "critic_penalty")):
        scale = np.abs(l64[:, c]).max()
        d_lib, d_t32 = np.abs(got[:, c] - l64[:, c]).max() / scale, np.abs(l32[:, c] - l64[:, c]).max() / scale
        report.append("%s over %d steps: library vs float64 %.3g, fp32 torch vs float64 %.3g (bound 4x = %.3g)" % (name, steps, d_lib, d_t32, 4 * d_t32))
    report.append("float64 loss per step: " + " ".join("%.6g" % v for v in l64[:, 0]))
    report.append("library loss per step: " + " ".join("%.6g" % v for v in got[:, 0]))
    r64, f64 = to64(real), to64(fake)
    with torch.no_grad():
        ref0 = T.net_with_weight_grad(params)
        before64 = float((ref0(*r64).mean(0) - ref0(*f64).mean(0)).sum())
        after64 = float((net64(*r64).mean(0) - net64(*f64).mean(0)).sum())
    report.append("mean(real) - mean(fake): library %.6g -> %.6g, float64 %.6g -> %.6g" % (before, after, before64, after64))
    msg = "\n".join(report)
    print(msg)
    for c in (0, 2):
        scale = np.abs(l64[:, c]).max()
        assert np.abs(got[:, c] - l64[:, c]).max() / scale <= 4 * np.abs(l32[:, c] - l64[:, c]).max() / scale, msg
    assert after64 > before64 and after > before, msg
    # the trained critic goes back through load_critic
    e2 = critic_only_engine(trained)
    try:
        assert torch.equal(e2.critic_params().cpu(), torch.from_numpy(critic_spec.params_to_flat(trained)))
    finally:
        e2.close()


def test_step_from_thetas(engine, params, pool):
    """the one-call helper: fake rows from hpe_smpl of every stage's theta, concatenated; real rows of one stage serve every stage"""
    B, stages = 16, 3
    thetas = [torch.from_numpy(synthetic.make_thetas(B, seed=50 + i)).cuda() for i in range(stages)]
    real = rows(pool, B, 14, start=300)
    saved = engine.critic_params().clone()
    try:
        g = torch.Generator().manual_seed(9)
        interp = (torch.rand((B * stages, 14, 3), generator=g).cuda(), torch.rand((B * stages, 10), generator=g).cuda(),
                  torch.rand((B * stages, 24, 3, 3), generator=g).cuda())
        outs = [engine.smpl(t, want=("joints", "Rs")) for t in thetas]
        fake = (torch.cat([o["joints"] for o in outs]), torch.cat(thetas)[:, 75:], torch.cat([o["Rs"] for o in outs]))
        real3 = tuple(torch.cat([t] * stages) for t in real)
        want = hpe_amd.critic_wgan_loss(engine, real3, fake, interp=interp)
        tr = hpe_amd.CriticTrainer(engine, lr=CRITIC_LR)
        r = tr.step_from_thetas(real, thetas, interp=interp)
        assert torch.equal(r["critic_network_loss"], want["loss"]) and torch.equal(r["critic_penalty"], want["penalty"])
        assert not torch.equal(engine.critic_params(), saved)
    finally:
        engine.set_critic_params(saved)
    assert torch.equal(engine.critic_params().view(torch.int32), saved.view(torch.int32))


def test_graph_capture(params, pool):
    """hpe_critic_weight_grad + hpe_critic_set_params_dev captured once (one stream: no parallel branches) and replayed"""
    N = 200
    joints, betas, Rs = rows(pool, N, 19, start=21)
    g = torch.Generator().manual_seed(93)
    gs = torch.randn((N, 3), generator=g).cuda()
    tg = {k: torch.randn(s, generator=g).cuda() for k, s in TANGENT_SHAPES.items()}
    e = critic_only_engine(params)
    try:
        e.critic_reserve(N)
        new = torch.from_numpy(critic_spec.params_to_flat(synthetic.make_critic_params(seed=2))).cuda()
        eager = e.critic_weight_grad(joints, betas, Rs, grad_scores=gs, tangents=tg).clone()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = e.critic_weight_grad(joints, betas, Rs, grad_scores=gs, tangents=tg)
            e.set_critic_params(new)
        captured.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured.view(torch.int32), eager.view(torch.int32))
        assert torch.equal(e.critic_params().view(torch.int32), new.view(torch.int32))
    finally:
        e.close()


def test_errors(engine, pool):
    z = lambda *s: torch.zeros(s, device="cuda")  # noqa: E731
    j, b, r, s, out = z(2, 14, 3), z(2, 10), z(2, 24, 3, 3), z(2, 3), z(critic_spec.PARAM_FLOATS)
    lib, h = engine.lib, engine._h
    call = lambda hh, K, N, gs, o: lib.hpe_critic_weight_grad(hh, j.data_ptr(), K, b.data_ptr(), 10, r.data_ptr(), N, gs, None, None, None,  # noqa: E731
                                                              None, 0, o, None)
    assert call(h, 14, 2, None, out.data_ptr()) == 1  # HPE_ERR_INVALID: grad_scores and every tangent NULL
    assert b"every tangent" in lib.hpe_last_error()
    assert call(h, 13, 2, s.data_ptr(), out.data_ptr()) == 1
    assert call(h, 14, 0, s.data_ptr(), out.data_ptr()) == 1
    assert call(h, 14, 2, s.data_ptr(), None) == 1
    assert lib.hpe_critic_get_params(h, None, None) == 1 and lib.hpe_critic_set_params_dev(h, None, None) == 1
    assert lib.hpe_critic_reserve(h, 0) == 1
    assert call(h, 14, 2, s.data_ptr(), out.data_ptr()) == 0
    bare = hpe_amd.HpeEngine(device=0, max_batch=8)  # no critic loaded: HPE_ERR_STATE
    try:
        assert call(bare._h, 14, 2, s.data_ptr(), out.data_ptr()) == 3
        assert lib.hpe_critic_get_params(bare._h, out.data_ptr(), None) == 3
        assert lib.hpe_critic_set_params_dev(bare._h, out.data_ptr(), None) == 3
        with pytest.raises(RuntimeError, match="critic"):
            hpe_amd.CriticTrainer(bare)
    finally:
        bare.close()
    with pytest.raises(ValueError):
        engine.critic_weight_grad(j, b, r)
    with pytest.raises(ValueError):
        engine.critic_weight_grad(j, b, r, tangents={"Rs": z(24, 3, 3)})
    with pytest.raises(ValueError):
        engine.critic_weight_grad(j, b, r, tangents={"kcs": z(13, 13), "betas": z(2, 10)})
    torch.cuda.synchronize()
