"""GPU tests of regressor training (run with -m gpu on an MI355X): hpe_regressor_forward_train against the inference path bit for bit and
against the float64 restatement, hpe_regressor_backward against float64 autograd of the IEF loop (tests/regressor_train_ref.py) at every
batch size where a launch changes form, repeatability, the device-side get / set of the parameters, the autograd wrapper, graph capture,
GeneratorTrainer against the float64 torch loop, error codes.

Batch sizes 1, 3, 4, 5, 64, 65: dense_gemv up to 4 rows and the 64 x 64 GEMM from 5, its tile edge at 64 / 65, and S * B = 3, 9, 12, 15,
192, 195 rows for the k-tail of the weight-gradient GEMM (steps of 2 rows, blocks of 16).

Bars.  Forward with masks: rel per image <= 5e-6, the bar tests/test_gpu_head.py holds the regressor's theta to.  Backward: for each of
the seven parameter tensors and grad_features, worst absolute error / largest reference magnitude <= 1e-4, the project's fp32 parity
bar.  The fp32 torch restatement sits under a quarter of both on these rows (tests/test_regressor_train_cpu.py).

A gradient summed over rows jumps where a pre-activation crosses 0, so the rows are CHOSEN by the float64 reference alone
(regressor_train_ref.pool: no pre-activation within 1e-5 of 0).

Training: the per-step losses of 10 GeneratorTrainer steps must stay within 4x the deviation that the fp32 torch restatement of the same
loop shows from the float64 loop (the rule fit_keypoints and CriticTrainer are held to).

No figures are recorded here yet: this file had not run on an MI355X when it was written (DESIGN.md "Regressor training")."""
import numpy as np
import pytest
import torch

import hpe_amd
from hpe_amd import regressor_spec, synthetic

import regressor_train_ref as T
from smpl_torch_ref import SmplTorch, make_theta

pytestmark = pytest.mark.gpu
TOL = 1e-4
REG_BAR = 5e-6
MAX_BATCH = 128
S = T.S
SENTINEL = 12345.678
N = regressor_spec.PARAM_FLOATS


def gpu(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()


def bits(t):
    return t.contiguous().view(torch.int32)


def make_engine(params, mean, max_batch, critic=None):
    e = hpe_amd.HpeEngine(device=0, max_batch=max_batch)
    e.load_smpl(synthetic.make_smpl_model())
    e.load_regressor({k: v for k, v in params.items() if k != "mean_theta"})
    e.load_mean_theta(mean)
    if critic is not None:
        e.load_critic(critic)
    e.finalize()
    return e


@pytest.fixture(scope="module")
def pool():
    return T.pool()


@pytest.fixture(scope="module")
def engine(pool):
    e = make_engine(pool["params"], pool["mean"], MAX_BATCH)
    yield e
    e.close()


_REF = {}  # (B, with_drop, last_only) -> float64 autograd result: computed once, never modified


def reference(pool, B, with_drop, last_only):
    key = (B, with_drop, last_only)
    if key not in _REF:
        feat, drop, gt = T.case(B, with_drop, last_only)
        _REF[key] = T.autograd_grads(pool["flat"], feat, drop, gt)
    return _REF[key]


@pytest.mark.parametrize("B", T.BATCHES)
def test_forward_train(engine, pool, B):
    feat, drop, _ = T.case(B, True, False)
    f = gpu(feat)
    got = engine.regressor_forward_train(f)
    assert tuple(got.shape) == (S, B, 85)
    th = None
    for i in range(S):  # the inference path, one stage at a time
        th = engine.regress_stage(f, th)
        assert torch.equal(bits(got[i]), bits(th)), "stage %d differs from regress_stage" % i
    assert torch.equal(bits(got[S - 1]), bits(engine.tail(f, want=("theta",))[0]["theta"]))
    masked = engine.regressor_forward_train(f, gpu(drop)).cpu().numpy()
    assert np.array_equal(masked[: S - 1], got[: S - 1].cpu().numpy())  # dropout at the last stage only
    want = T.forward(pool["flat"], feat, drop)
    r = float((np.abs(masked - want).reshape(-1, 85).max(1) / np.abs(want).reshape(-1, 85).max(1)).max())
    plain = T.forward(pool["flat"], feat, None)
    r0 = float((np.abs(got.cpu().numpy() - plain).reshape(-1, 85).max(1) / np.abs(plain).reshape(-1, 85).max(1)).max())
    print("B=%d forward rel per image: with masks %.3g, without %.3g" % (B, r, r0))
    assert r <= REG_BAR and r0 <= REG_BAR


@pytest.mark.parametrize("last_only", [False, True])
@pytest.mark.parametrize("with_drop", [False, True])
@pytest.mark.parametrize("B", T.BATCHES)
def test_backward_accuracy(engine, pool, B, with_drop, last_only):
    feat, drop, gt = T.case(B, with_drop, last_only)
    want, want_f = reference(pool, B, with_drop, last_only)
    # sentinels behind grad_flat and behind row B of grad_features
    gflat = torch.full((N + 64,), SENTINEL, device="cuda")
    gfeat = torch.full((B + 1, 2048), SENTINEL, device="cuda")
    f, d, g = gpu(feat), gpu(drop), gpu(gt)
    lib, h = engine.lib, engine._h
    rc = lib.hpe_regressor_backward(h, f.data_ptr(), B, d.data_ptr() if d is not None else None, g.data_ptr(), gflat.data_ptr(), gfeat.data_ptr(),
                                    engine._stream())
    assert rc == 0, lib.hpe_last_error()
    torch.cuda.synchronize()
    sent = bits(torch.full((1,), SENTINEL))[0]
    assert bool((bits(gflat[N:]).cpu() == sent).all()) and bool((bits(gfeat[B:]).cpu() == sent).all())
    errs = T.per_tensor_errors(gflat[:N].cpu().numpy(), want, gfeat[:B].cpu().numpy(), want_f)
    msg = "B=%d drop=%d last_only=%d: " % (B, with_drop, last_only) + "  ".join("%s %.3g" % kv for kv in errs)
    print(msg)
    assert len(errs) == 8
    for key, e in errs:
        assert e <= TOL, msg
    # grad_features not requested: the same parameter gradient, bit for bit
    only, none = engine.regressor_backward(f, g, d, want_grad_features=False)
    assert none is None and torch.equal(bits(only), bits(gflat[:N]))
    if last_only and not with_drop:  # a NULL cotangent is zero
        zero, zf = engine.regressor_backward(f, None)
        assert float(zero.abs().max()) == 0.0 and float(zf.abs().max()) == 0.0


def test_bitwise_repeatable(engine, pool):
    feat, drop, gt = T.case(65, True, False)
    other = T.case(5, False, True)
    f, d, g = gpu(feat), gpu(drop), gpu(gt)
    a, af = engine.regressor_backward(f, g, d)
    a, af = a.clone(), af.clone()
    engine.regressor_backward(gpu(other[0]), gpu(other[2]))
    engine.regressor_forward_train(gpu(other[0]))
    b, bf = engine.regressor_backward(f, g, d)
    assert torch.equal(bits(a), bits(b)) and torch.equal(bits(af), bits(bf))


def test_param_round_trip(pool):
    """get after set returns the bits; after set_regressor_params the tail gives the bits of an engine that loaded the same values"""
    other = synthetic.make_regressor_params(seed=9, variant="bounded")
    mean2 = (pool["mean"] * np.float32(1.01)).astype(np.float32)
    a, b = make_engine(pool["params"], pool["mean"], 8), make_engine(other, mean2, 8)
    try:
        flat_a = torch.from_numpy(pool["flat"]).cuda()
        flat_b = torch.from_numpy(regressor_spec.params_to_flat(other, mean2)).cuda()
        assert torch.equal(bits(a.regressor_params()), bits(flat_a)) and torch.equal(bits(b.regressor_params()), bits(flat_b))
        want_all = ("theta", "verts", "kp2d")
        for B in (3, 8):
            f = gpu(pool["feat"][:B])
            assert not torch.equal(a.tail(f, want=("theta",))[0]["theta"], b.tail(f, want=("theta",))[0]["theta"])
        a.set_regressor_params(flat_b)
        assert torch.equal(bits(a.regressor_params()), bits(flat_b))
        for B in (3, 8):
            f = gpu(pool["feat"][:B])
            oa, ob = a.tail(f, all_stages=True, want=want_all), b.tail(f, all_stages=True, want=want_all)
            for sa, sb in zip(oa, ob):
                for k in want_all:
                    assert torch.equal(bits(sa[k]), bits(sb[k])), (B, k)
            assert torch.equal(bits(a.regress_stage(f)), bits(b.regress_stage(f)))
            g = torch.ones((S, B, 85), device="cuda")
            ga, gb = a.regressor_backward(f, g), b.regressor_backward(f, g)
            assert torch.equal(bits(ga[0]), bits(gb[0])) and torch.equal(bits(ga[1]), bits(gb[1]))
        back = regressor_spec.flat_to_params(a.regressor_params())
        for key in other:
            assert np.array_equal(back[key], other[key]), key
        assert np.array_equal(back["mean_theta"], mean2)
        with pytest.raises(ValueError):
            a.set_regressor_params(flat_b[:-1])
    finally:
        a.close()
        b.close()


def test_autograd(engine, pool):
    B = 5
    feat, drop, _ = T.case(B, True, False)
    f = gpu(feat).requires_grad_(True)
    d = gpu(drop)
    params = engine.regressor_params().requires_grad_(True)
    th = hpe_amd.regressor_thetas(engine, f, params, d)
    assert th.grad_fn is not None and tuple(th.shape) == (S, B, 85)
    th.sum().backward()
    gflat, gfeat = engine.regressor_backward(f.detach(), torch.ones((S, B, 85), device="cuda"), d)
    assert torch.equal(bits(params.grad), bits(gflat)) and torch.equal(bits(f.grad), bits(gfeat))
    # features without grad: only params.grad
    p2 = engine.regressor_params().requires_grad_(True)
    hpe_amd.regressor_thetas(engine, f.detach(), p2, d).sum().backward()
    assert torch.equal(bits(p2.grad), bits(gflat))
    with pytest.raises(ValueError):
        hpe_amd.regressor_thetas(engine, f, params[:-1], d)


def test_graph_capture(pool):
    """hpe_regressor_backward + hpe_regressor_set_params_dev captured once (one stream: no parallel branches) and replayed twice"""
    B = 8
    feat, drop, gt = T.case(B, True, False)
    f, d, g = gpu(feat), gpu(drop), gpu(gt)
    e = make_engine(pool["params"], pool["mean"], 8)
    try:
        new = torch.from_numpy(regressor_spec.params_to_flat(synthetic.make_regressor_params(seed=9, variant="bounded"), pool["mean"])).cuda()
        start = e.regressor_params().clone()
        eager, eager_f = (t.clone() for t in e.regressor_backward(f, g, d))
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            cap, cap_f = e.regressor_backward(f, g, d)
            e.set_regressor_params(new)
        e.set_regressor_params(start)  # the capture enqueued nothing: the replays start from the first weights
        replays = []
        for _ in range(2):
            e.set_regressor_params(start)
            cap.zero_()
            cap_f.zero_()
            graph.replay()
            torch.cuda.synchronize()
            replays.append((cap.clone(), cap_f.clone()))
            assert torch.equal(bits(e.regressor_params()), bits(new))
        assert torch.equal(bits(replays[0][0]), bits(replays[1][0])) and torch.equal(bits(replays[0][1]), bits(replays[1][1]))
        assert torch.equal(bits(replays[0][0]), bits(eager)) and torch.equal(bits(replays[0][1]), bits(eager_f))
    finally:
        e.close()


def test_training(pool):
    """10 GeneratorTrainer steps from features at B = 8 (keypoint loss + critic term, fixed masks) against the float64 torch loop; the
    bound is 4x the deviation of the fp32 torch restatement of the same loop from the float64 loop"""
    B, steps, lr = 8, 10, 0.0001
    smpl_model, critic = synthetic.make_smpl_model(), synthetic.make_critic_params(seed=6)
    feat, drop, _ = T.case(B, True, True)
    with torch.no_grad():
        kp = SmplTorch(smpl_model, torch.float64)(torch.from_numpy(make_theta(B, seed=77, special=False)).double())["kp2d"].numpy()
    vis = np.ones((B, kp.shape[1], 1))
    vis[1, 3] = vis[4, 0] = vis[6, 11] = 0.0
    kp_gt = np.concatenate([kp, vis], 2).astype(np.float32)
    l64, flat64 = T.generator_loop(pool["flat"], feat, kp_gt, drop, smpl_model, critic, steps, lr, torch.float64)
    l32, _ = T.generator_loop(pool["flat"], feat, kp_gt, drop, smpl_model, critic, steps, lr, torch.float32)
    e = make_engine(pool["params"], pool["mean"], B, critic=critic)
    fresh = None
    try:
        tr = hpe_amd.GeneratorTrainer(e, lr=lr)
        assert torch.equal(bits(tr.params.detach()), bits(e.regressor_params()))
        f, d, gt = gpu(feat), gpu(drop), gpu(kp_gt)
        got = []
        for _ in range(steps):
            r = tr.step(f, gt, drop=d)
            assert sorted(r) == ["generated_cams", "generator_critic_losses", "grad_features", "kpr_losses", "mr_losses", "pred_keypoints", "thetas"]
            assert len(r["kpr_losses"]) == S and len(r["generator_critic_losses"]) == S and r["mr_losses"] == []
            assert tuple(r["grad_features"].shape) == (B, 2048) and len(r["thetas"]) == S and tuple(r["thetas"][0].shape) == (B, 85)
            assert tuple(r["pred_keypoints"].shape) == (B, kp.shape[1], 2) and tuple(r["generated_cams"].shape) == (B, 3)
            got.append([float(r["kpr_losses"][-1]), float(r["generator_critic_losses"][-1])])
        got = np.asarray(got, np.float64)
        assert torch.equal(bits(tr.params.detach()), bits(e.regressor_params()))
        trained = regressor_spec.flat_to_params(tr.params)
        fresh = make_engine(trained, trained["mean_theta"], B, critic=critic)
        oa, ob = e.tail(f, want=("theta", "kp2d")), fresh.tail(f, want=("theta", "kp2d"))
        for k in ("theta", "kp2d"):
            assert torch.equal(bits(oa[0][k]), bits(ob[0][k])), k
        drift = float(np.abs(tr.params.detach().cpu().numpy() - flat64).max())
    finally:
        e.close()
        if fresh is not None:
            fresh.close()
    tot, t64, t32 = got.sum(1), l64.sum(1), l32.sum(1)
    report = []
    for name, a, b, c in (("kpr loss", got[:, 0], l64[:, 0], l32[:, 0]), ("critic term", got[:, 1], l64[:, 1], l32[:, 1]), ("sum", tot, t64, t32)):
        scale = np.abs(b).max()
        report.append("%s over %d steps: library vs float64 %.3g, fp32 torch vs float64 %.3g (bound 4x)" % (name, steps, np.abs(a - b).max() / scale,
                                                                                                      np.abs(c - b).max() / scale))
    report.append("float64 loss per step: " + " ".join("%.6g" % v for v in t64))
    report.append("library loss per step: " + " ".join("%.6g" % v for v in tot))
    report.append("largest parameter difference to the float64 loop after %d steps: %.3g" % (steps, drift))
    msg = "\n".join(report)
    print(msg)
    for a, b, c in ((got[:, 0], l64[:, 0], l32[:, 0]), (got[:, 1], l64[:, 1], l32[:, 1]), (tot, t64, t32)):
        assert np.abs(a - b).max() <= 4 * np.abs(c - b).max(), msg
    assert tot[-1] < tot[0] and t64[-1] < t64[0], msg


def test_errors(engine, pool):
    z = lambda *s: torch.zeros(s, device="cuda")  # noqa: E731
    f, th, g, gf = z(2, 2048), z(S, 2, 85), z(N), z(2, 2048)
    lib, h = engine.lib, engine._h
    bwd = lambda hh, fp, B, out: lib.hpe_regressor_backward(hh, fp, B, None, th.data_ptr(), out, gf.data_ptr(), None)  # noqa: E731
    assert bwd(h, f.data_ptr(), MAX_BATCH + 1, g.data_ptr()) == 1  # HPE_ERR_INVALID
    assert bwd(h, f.data_ptr(), 0, g.data_ptr()) == 1 and bwd(h, f.data_ptr(), -3, g.data_ptr()) == 1
    assert bwd(h, None, 2, g.data_ptr()) == 1 and bwd(h, f.data_ptr(), 2, None) == 1
    assert lib.hpe_regressor_forward_train(h, None, 2, None, th.data_ptr(), None) == 1
    assert lib.hpe_regressor_forward_train(h, f.data_ptr(), 2, None, None, None) == 1
    assert lib.hpe_regressor_forward_train(h, f.data_ptr(), MAX_BATCH + 1, None, th.data_ptr(), None) == 1
    assert lib.hpe_regressor_get_params(h, None, None) == 1 and lib.hpe_regressor_set_params_dev(h, None, None) == 1
    assert bwd(h, f.data_ptr(), 2, g.data_ptr()) == 0
    bare = hpe_amd.HpeEngine(device=0, max_batch=8)  # not finalized: HPE_ERR_STATE
    try:
        bare.load_regressor(pool["params"])
        bare.load_mean_theta(pool["mean"])
        assert bwd(bare._h, f.data_ptr(), 2, g.data_ptr()) == 3
        assert lib.hpe_regressor_forward_train(bare._h, f.data_ptr(), 2, None, th.data_ptr(), None) == 3
        assert lib.hpe_regressor_get_params(bare._h, g.data_ptr(), None) == 3
        assert lib.hpe_regressor_set_params_dev(bare._h, g.data_ptr(), None) == 3
    finally:
        bare.close()
    with pytest.raises(ValueError):
        engine.regressor_backward(f, z(S, 3, 85))
    with pytest.raises(ValueError):
        engine.regressor_forward_train(f, z(2, 3, 1024))
    torch.cuda.synchronize()
