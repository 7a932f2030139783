"""Mixed-precision encoder training with batch statistics on the GPU (precision="mixed", bn="batch": hpe_encoder_*_batchnorm_mixed)
against the CPU restatements of tests/encoder_bn_train_ref.py (float64 / float32, with the kernels replaced by W16 = RNE(W)) and
tests/encoder_bn_mixed_ref.py (float32 with the roundings of the contract).  Every bar comes from those restatements on the same inputs,
never from the code under test:

  fp32 results (dbeta, dgamma, dW)   norm-relative error below 4 x that of the same restatement in float32; where that is 0 only an exact
                                     result passes.  dW's restatements read dzraw16 as the contract's point 5 gives it, reproduced here
                                     in float32 from the GPU's own statistics, dgamma and dbeta (the elementwise passes fuse no product
                                     into a sum, so it is reproducible: a mismatch would show as a dW error of 2^-8 / sqrt(M N), far
                                     above these bars)
  mu, var                            against float64 statistics of the GPU's own z16, within 2^-22 (tests/test_gpu_encoder_bn_train.py)
  bf16 results (z16, y16, dx)        per element: 2^-8 |ref| for the one final rounding plus the fp32 part -- the project's per-layer
                                     forward bar (z16), 4 x the float32 restatement's worst error (y16), 4 x e32 x A (dx,
                                     tests/gemm_ref.py)
  the whole network's gradient       norm-relative error below 4 x that of network_backward_mixed on the same stashes"""
import threading

import numpy as np
import pytest
import torch

import encoder_bn_mixed_ref as XB
import encoder_bn_train_ref as RB
import encoder_mixed_ref as X
import encoder_train_ref as R
import hpe_amd
from gemm_ref import BF16_ULP, ORDER_MARGIN
from hpe_amd import _lib, resnet_spec, synthetic
from hpe_amd.resnet_spec import CONV_SPECS, ENCODER_PARAM_OFFSETS, ENCODER_STAT_OFFSETS
from oracle import hmr_oracle as O
from test_gpu_encoder_bn_reduce import Meeting
from test_gpu_encoder_train import FORWARD_BAR, MARGIN, make_engine, make_params
from test_gpu_trainer import STAGES, data, make_trainer, result_tensors, same, tensors_of, weights  # noqa: F401  (data, weights: fixtures)
from test_gpu_trainer import B as TRAINER_B

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
ULP4 = 2.0 ** -22  # four half-ulps of float32
N_LAYERS = len(CONV_SPECS)
EPS32 = np.float32(1e-3)


@pytest.fixture(scope="module")
def params():
    return make_params()


@pytest.fixture(scope="module")
def engine(params):
    e = make_engine(params)  # fp32, max_batch 4, fp32 reserve of 3
    e.reserve_encoder_train(3, batch_norm=True, precision="mixed")
    yield e
    e.close()


def _dev16(t):
    return t.to(BF).cuda()


def _p16(params):
    p16 = dict(params)
    for s in CONV_SPECS:
        p16[s.name + "/kernel"] = X.rne(torch.from_numpy(np.asarray(params[s.name + "/kernel"], np.float32))).numpy()
    return p16


def _stats_errors(mu, var, z):
    mu64, var64 = RB.batch_stats(z.double())
    emu = float(((mu.double() - mu64).abs() / torch.maximum(mu64.abs(), var64.sqrt())).max())
    evar = float(((var.double() - var64).abs() / var64).max())
    return emu, evar


def _check_forward(s, tag, x16, res, relu, z, y, mu, var, lt16):
    """z16, the statistics and y16 of one layer (all CPU float32 tensors holding the GPU's values) against float64"""
    lt64 = [t.double() for t in lt16]
    z64 = RB.layer_raw(s, x16.double(), lt64)
    scale = float(z64.abs().max())
    wz = float(((z.double() - z64).abs() / (BF16_ULP * z64.abs() + FORWARD_BAR * scale)).max())
    emu, evar = _stats_errors(mu, var, z)
    r64 = res.double() if res is not None else None
    ref = RB.layer_apply(z.double(), mu.double(), var.double(), lt64[2], lt64[3], r64, relu)
    f32 = RB.layer_apply(z, mu, var, lt16[2], lt16[3], res, relu)
    e32 = float((f32.double() - ref).abs().max())
    wy = float(((y.double() - ref).abs() / (BF16_ULP * ref.abs() + MARGIN * e32)).max())
    print("%s %-16s z16 worst element at %.3g of its bound  mu %.3g  var %.3g (bar %.3g)  y16 worst element at %.3g of its bound (e32 %.3g)"
          % (tag, s.name, wz, emu, evar, ULP4, wy, e32))
    assert wz <= 1.0, (s.name, wz)
    assert emu <= ULP4 and evar <= ULP4, (s.name, emu, evar)
    assert wy <= 1.0, (s.name, wy)


def _dzraw16(z, y, dy, mu, var, gamma, dgamma, dbeta, M):
    """rounding point 5 in float32, operation for operation as bn_bwd_apply_bf16_kernel: r as bn_finish_channel rounds it"""
    r = torch.from_numpy((1.0 / np.sqrt(var.numpy().astype(np.float64) + np.float64(EPS32))).astype(np.float32))
    Mf = torch.tensor(float(M), dtype=torch.float32)
    dz = dy * (y > 0).to(dy.dtype) if y is not None else dy
    xh = (z - mu) * r
    return X.rne((gamma * r) * ((dz - dbeta / Mf) - xh * (dgamma / Mf)))


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("idx", range(N_LAYERS))
def test_layer(engine, params, idx, B):
    s = CONV_SPECS[idx]
    g = torch.Generator().manual_seed(3000 * B + idx)
    x = torch.randn(B, s.hin, s.hin, s.cin, generator=g)
    x = x if idx == 0 else X.rne(x)  # conv1 takes the float32 images
    res = X.rne(torch.randn(B, s.hout, s.hout, s.cout, generator=g)) if s.name.endswith("2c") else None
    dy = X.rne(torch.randn(B, s.hout, s.hout, s.cout, generator=g))
    shortcut = s.name.endswith("branch1")
    xd = x.cuda() if idx == 0 else _dev16(x)
    y16, z16, st = engine.debug_conv_batchnorm(idx, xd, _dev16(res) if res is not None else None, relu=True, precision="mixed")
    assert y16.dtype == BF and z16.dtype == BF and st.dtype == torch.float32
    y, z, st = y16.float().cpu(), z16.float().cpu(), st.cpu()
    mu, var = st[:s.cout], st[s.cout:]
    lt = R.layer_tensors(params, s, torch.float32)
    lt16 = X.weights16(lt)
    x16 = X.rne(x) if idx == 0 else x  # the bf16 pad rounds the pixels
    _check_forward(s, "layer %2d B=%d" % (idx, B), x16, res, True, z, y, mu, var, lt16)
    M = B * s.hout * s.hout
    A = R.im2col(s, x16)
    for tag, yy in [("gated  ", y)] + ([("ungated", None)] if shortcut else []):  # as the network runs a projection shortcut: dz = dy
        dx, gl = engine.debug_conv_backward_batchnorm(idx, xd, z16, y16 if yy is not None else None, _dev16(dy), precision="mixed")
        torch.cuda.synchronize()
        got = R.split_layer_grad(s, gl.cpu())
        assert float(got["db"].abs().max()) == 0.0
        ref = RB.layer_backward(s, x16.double(), z.double(), yy, dy.double(), [t.double() for t in lt16], want_dx=False, gated=yy is not None)
        f32 = RB.layer_backward(s, x16, z, yy, dy, lt16, want_dx=False, gated=yy is not None)
        dzraw = _dzraw16(z, yy, dy, mu, var, lt[2], got["dgamma"], got["dbeta"], M).reshape(M, s.cout)
        ref["dW"], f32["dW"] = (A.double().t() @ dzraw.double()).reshape(-1), (A.t() @ dzraw).reshape(-1)
        for k in ("dbeta", "dgamma", "dW"):
            e, bar = R.rel(got[k], ref[k].reshape(-1)), MARGIN * R.rel(f32[k].reshape(-1), ref[k].reshape(-1))
            print("layer %2d %-16s B=%d %-6s %s gpu %.3g  bar %.3g" % (idx, s.name, B, k, tag, e, bar))
            assert e < bar or e == 0.0, (s.name, k, e, bar)
        if idx == 0:
            assert dx is None
            continue
        assert dx.dtype == BF
        W16 = lt16[0]
        dzr = dzraw.reshape(B, s.hout, s.hout, s.cout)
        dref = X.data_grad_mixed(s, dzr.double(), W16.double(), B, rounding=False)
        Ab = X.data_grad_mixed(s, dzr.abs().double(), W16.abs().double(), B, rounding=False)
        d32 = X.data_grad_mixed(s, dzr, W16, B, rounding=False).double()
        live = Ab > 0
        e32 = float(((d32 - dref).abs()[live] / Ab[live]).max())
        err = (dx.float().cpu().double() - dref).abs()
        bound = BF16_ULP * dref.abs() + ORDER_MARGIN * e32 * Ab
        worst = float((err[live] / bound[live]).max())
        print("layer %2d %-16s B=%d dx     %s worst element at %.3g of its bound (e32 %.3g)" % (idx, s.name, B, tag, worst, e32))
        assert bool((err <= bound).all()), (s.name, worst)  # where A == 0 (the odd pixels of a stride-2 layer) only an exact 0 passes
        if s.stride == 2:
            d = dx.float().cpu()
            assert float(d[:, 1::2].abs().max()) == 0.0 and float(d[:, :, 1::2].abs().max()) == 0.0


@pytest.fixture(scope="module")
def whole(engine, params):
    """B = 2: one mixed batch-statistics forward and backward, the stashes they left, and the float64 / mixed restatements they drive"""
    B = 2
    img = synthetic.make_images(B, seed=31)
    gf = torch.randn(B, 2048, generator=torch.Generator().manual_seed(3))
    imgs = torch.from_numpy(img).cuda()
    feat = engine.encoder_forward_train(imgs, bn="batch", precision="mixed").cpu()
    grad = engine.encoder_backward(imgs, gf.cuda(), bn="batch", precision="mixed").cpu()
    assert engine.lib.hpe_debug_encoder_stash_batch_mixed(engine._h) == B
    st16 = [engine.encoder_stash(i, precision="mixed") for i in range(N_LAYERS)]
    z16 = [engine.encoder_stash_raw(i, precision="mixed") for i in range(N_LAYERS)]
    assert all(t.dtype == BF for t in st16 + z16)
    stash, zstash = [t.float().cpu() for t in st16], [t.float().cpu() for t in z16]
    pooled = engine.encoder_stash(-1, precision="mixed").float().cpu()
    bstats = engine.encoder_batch_stats().cpu()
    win = R.maxpool_winners(stash[0])
    p16 = _p16(params)
    img16 = X.rne(torch.from_numpy(img))
    ref = RB.network_backward(p16, img16, zstash, stash, pooled, win, gf)
    mixed = XB.network_backward_mixed(params, torch.from_numpy(img), zstash, stash, pooled, win, gf)
    return dict(img=img, img16=img16, feat=feat, grad=grad, stash=stash, zstash=zstash, pooled=pooled, bstats=bstats, ref=ref, mixed=mixed, gf=gf,
                p16=p16)


def _layer_inputs_of(stash, pooled, img16):
    bl = R.blocks()
    inputs, resid = {0: img16}, {}
    for k, (i2a, i2b, i2c, i1) in enumerate(bl):
        xin = pooled if k == 0 else stash[bl[k - 1][2]]
        inputs[i2a], inputs[i2b], inputs[i2c] = xin, stash[i2a], stash[i2b]
        resid[i2c] = xin if i1 is None else stash[i1]
        if i1 is not None:
            inputs[i1] = xin
    return inputs, resid


def test_stash_consistency(whole):
    """every stashed z16, statistic and y16 from its stashed input, as in test_layer; the pooled map is the max pool of stashed conv1"""
    st, zs, b = whole["stash"], whole["zstash"], whole["bstats"]
    inputs, resid = _layer_inputs_of(st, whole["pooled"], whole["img16"])
    for i, s in enumerate(CONV_SPECS):
        om, ov = ENCODER_STAT_OFFSETS[i]
        lt16 = R.layer_tensors(whole["p16"], s, torch.float32)
        _check_forward(s, "net layer %2d" % i, inputs[i], resid.get(i, None), not s.name.endswith("branch1"), zs[i], st[i], b[om:om + s.cout],
                       b[ov:ov + s.cout], lt16)
    pool_ref = torch.nn.functional.max_pool2d(torch.nn.functional.pad(st[0].permute(0, 3, 1, 2), (1, 1, 1, 1)), 3, 2).permute(0, 2, 3, 1)
    assert torch.equal(whole["pooled"], pool_ref)


def _check_network_grad(grad, ref, mixed, tag):
    worst = (0.0, None)
    for i, (s, off) in enumerate(zip(CONV_SPECS, ENCODER_PARAM_OFFSETS)):
        n = s.kh * s.kw * s.cin * s.cout + 3 * s.cout
        got, rr, mx = (R.split_layer_grad(s, t[off[0]:off[0] + n]) for t in (grad, ref, mixed))
        assert float(got.pop("db").abs().max()) == 0.0
        for k in got:
            e, bar = R.rel(got[k], rr[k]), MARGIN * R.rel(mx[k], rr[k])
            print("%s layer %2d %-16s %-6s gpu %.3g  bar %.3g" % (tag, i, s.name, k, e, bar))
            if e / bar > worst[0]:
                worst = (e / bar, (s.name, k, e, bar))
            assert e < bar, (s.name, k, e, bar)
    print(tag, "worst layer against its bar:", worst)


def test_network_backward(whole):
    _check_network_grad(whole["grad"], whole["ref"], whole["mixed"], "net")


def test_forward_features(whole, params):
    """the features are the fp32 mean of the 49 stashed bf16 values (49 additions and one division, each within 2^-24 of the running
    magnitude); end to end they are within 4 x the distance of the CPU mixed restatement from the float64 whole-forward restatement on the
    same images, measured here"""
    last = whole["stash"][R.blocks()[-1][2]].double().reshape(2, 49, 2048)
    mean = last.sum(1) / 49
    err = (whole["feat"].double() - mean).abs()
    assert bool((err <= 51 * 2.0 ** -24 * last.abs().sum(1) / 49).all()), float(err.max())
    ti = torch.from_numpy(whole["img"])
    ref, _ = RB.network_forward(params, ti)
    cpu, _ = XB.network_forward_mixed(params, ti)
    dist = lambda a: float((a.double() - ref).abs().max() / ref.abs().max())  # noqa: E731
    e, d = dist(whole["feat"]), dist(cpu)
    print("mixed batch-mode features against the float64 restatement: gpu %.3g, the CPU mixed restatement %.3g, bar %.3g" % (e, d, MARGIN * d))
    assert e < MARGIN * d


def test_deterministic_and_capturable(engine, whole):
    imgs = torch.from_numpy(whole["img"]).cuda()
    gf = whole["gf"].cuda()
    kw = dict(bn="batch", precision="mixed")
    a = engine.encoder_backward(imgs, gf, **kw)
    engine.encoder_backward(imgs[:1].contiguous(), gf[:1].contiguous() * 2, **kw)  # another call in between
    b = engine.encoder_backward(imgs, gf, **kw)
    assert torch.equal(a, b) and torch.equal(a.cpu(), whole["grad"])
    out = torch.empty_like(a)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            _lib.check(engine.lib.hpe_encoder_backward_batchnorm_mixed(engine._h, imgs.data_ptr(), 2, gf.data_ptr(), out.data_ptr(), engine._stream()))
        for _ in range(2):
            out.zero_()
            graph.replay()
            side.synchronize()
            assert torch.equal(out, a)
    torch.cuda.current_stream().wait_stream(side)


def test_interleaved_with_the_other_walks(engine, whole):
    """mixed batch, fp32 frozen, fp32 batch and bf16 frozen backwards on one context, which share the statistics slots, the reduction
    partials and the weight gradient's scratch: each gives the bits of its first call whatever ran before it; an fp32 forward leaves the
    mixed stashes and their counter alone; precision="mixed" with frozen statistics is precision="bf16", bit for bit"""
    imgs = torch.from_numpy(whole["img"]).cuda()
    gf = whole["gf"].cuda()
    run = {"x": lambda: engine.encoder_backward(imgs, gf, bn="batch", precision="mixed"), "f": lambda: engine.encoder_backward(imgs, gf),
           "b": lambda: engine.encoder_backward(imgs, gf, bn="batch"), "m": lambda: engine.encoder_backward(imgs, gf, precision="bf16")}
    first = {}
    for k in "xfbmxbxmfxxbmfx":
        r = run[k]()
        assert torch.equal(r, first.setdefault(k, r)), k
    assert torch.equal(first["x"].cpu(), whole["grad"])
    assert len({tuple(v[:64].tolist()) for v in first.values()}) == 4  # four different walks
    assert torch.equal(engine.encoder_backward(imgs, gf, bn="frozen", precision="mixed"), first["m"])
    assert torch.equal(engine.encoder_forward_train(imgs, precision="mixed"), engine.encoder_forward_train(imgs, precision="bf16"))
    run["x"]()
    engine.encoder_forward_train(imgs[:1].contiguous())              # fp32 forwards of another batch, frozen ...
    assert engine.lib.hpe_debug_encoder_stash_batch(engine._h) == 1 and engine.lib.hpe_debug_encoder_stash_batch_mixed(engine._h) == 2
    assert torch.equal(engine.encoder_stash(3, precision="mixed").float().cpu(), whole["stash"][3])
    assert torch.equal(engine.encoder_stash_raw(3, precision="mixed").float().cpu(), whole["zstash"][3])
    engine.encoder_forward_train(imgs[:1].contiguous(), bn="batch")  # ... and with batch statistics: the statistics are now its own
    assert engine.lib.hpe_debug_encoder_stash_batch_mixed(engine._h) == 2
    assert torch.equal(engine.encoder_stash_raw(7, precision="mixed").float().cpu(), whole["zstash"][7])
    assert engine.encoder_stash_raw(7).shape[0] == 1
    assert not torch.equal(engine.encoder_batch_stats().cpu(), whole["bstats"])
    run["x"]()
    assert torch.equal(engine.encoder_batch_stats().cpu(), whole["bstats"])
    with pytest.raises(_lib.HpeError, match="mixed-precision one"):  # the fp32 z stash does not hold what these statistics were taken of
        engine.encoder_stash_raw(7)


def test_params_update_reaches_the_walk(params):
    """after set_encoder_params_dev(q) the next call computes with RNE(q) and q's gamma, beta and bias: it equals a fresh context that loaded q"""
    kw = dict(bn="batch", precision="mixed")
    e = make_engine(params, max_batch=2, reserve=0)
    try:
        e.reserve_encoder_train(2, batch_norm=True, precision="mixed")
        img = torch.from_numpy(synthetic.make_images(2, seed=9)).cuda()
        p = e.encoder_params().cpu()
        f0 = e.encoder_forward_train(img, **kw).cpu()
        d = torch.randn(p.shape, generator=torch.Generator().manual_seed(2))
        q = p + d * (1e-2 * float(p.norm()) / float(d.norm()))
        e.set_encoder_params_dev(q.cuda())
        f1 = e.encoder_forward_train(img, **kw).cpu()
        g1 = e.encoder_backward(img, torch.ones(2, 2048, device="cuda"), **kw).cpu()
        fresh = make_engine(resnet_spec.flat_to_params(q, params), max_batch=2, reserve=0)
        try:
            fresh.reserve_encoder_train(2, batch_norm=True, precision="mixed")
            f2 = fresh.encoder_forward_train(img, **kw).cpu()
            g2 = fresh.encoder_backward(img, torch.ones(2, 2048, device="cuda"), **kw).cpu()
        finally:
            fresh.close()
        assert torch.equal(f1, f2) and torch.equal(g1, g2)
        assert not torch.equal(f1, f0)
    finally:
        e.close()


def test_every_batch_up_to_the_reserve(params):
    e = make_engine(params, max_batch=17, reserve=0)
    try:
        e.reserve_encoder_train(17, batch_norm=True, precision="mixed")
        img = torch.from_numpy(synthetic.make_images(17, seed=4)).cuda()
        gf = torch.randn(17, 2048, device="cuda")
        for B in range(1, 18):
            g = e.encoder_backward(img[:B].contiguous(), gf[:B].contiguous(), bn="batch", precision="mixed")
            assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, B
            assert e.lib.hpe_debug_encoder_stash_batch_mixed(e._h) == B
    finally:
        e.close()


def test_autograd_function(engine, whole):
    """encoder_features(bn="batch", precision="mixed"): one .backward() fills the flat tensor's .grad with the bits of the C call"""
    imgs = torch.from_numpy(whole["img"]).cuda()
    p = engine.encoder_params().requires_grad_(True)
    f = hpe_amd.encoder_features(engine, imgs, p, bn="batch", precision="mixed")
    assert f.dtype == torch.float32 and torch.equal(f.cpu(), whole["feat"])
    (f * whole["gf"].cuda()).sum().backward()
    assert p.grad.dtype == torch.float32 and torch.equal(p.grad.cpu(), whole["grad"])


def test_update_stats(engine, params):
    """update_encoder_stats after a mixed batch forward at B = 3 against the float64 formula on the batch statistics, each layer's own M"""
    img = torch.from_numpy(synthetic.make_images(3, seed=17)).cuda()
    engine.encoder_forward_train(img, bn="batch", precision="mixed")
    stats0 = engine.encoder_stats()
    assert np.array_equal(stats0.cpu().numpy(), resnet_spec.params_to_stats(params))
    batch = engine.encoder_batch_stats().cpu().double()
    for unbiased in (False, True):
        t = stats0.clone()
        assert engine.update_encoder_stats(t, momentum=0.9, unbiased=unbiased) is t
        ref = RB.momentum_update(stats0.cpu().double(), batch, 3, 0.9, unbiased)
        e = float(((t.cpu().double() - ref).abs() / ref.abs()).max())
        print("update_encoder_stats after a mixed forward, unbiased=%s: worst relative error %.3g (bar %.3g)" % (unbiased, e, ULP4))
        assert e <= ULP4
        assert not torch.equal(t, stats0)
    assert torch.equal(engine.encoder_stats(), stats0)  # nothing was installed
    fresh = make_engine(params, max_batch=2, reserve=0)
    try:
        fresh.reserve_encoder_train(1, batch_norm=True, precision="mixed")
        with pytest.raises(_lib.HpeError):  # no batch-mode forward of either precision has run
            fresh.update_encoder_stats(fresh.encoder_stats())
        fresh.encoder_forward_train(img[:1].contiguous(), precision="mixed")  # a frozen one does not count
        with pytest.raises(_lib.HpeError):
            fresh.update_encoder_stats(fresh.encoder_stats())
    finally:
        fresh.close()


def test_identity_hook_is_bit_exact(engine):
    """an identity hook with G = B: features, grad_flat, the batch statistics and the moved statistics have the bits of the path without a
    hook; 53 hook calls per forward, 2 x 53 per backward, each on the layer's 2 * cout doubles"""
    img = torch.from_numpy(synthetic.make_images(2, seed=31)).cuda()
    gf = torch.randn(2, 2048, generator=torch.Generator().manual_seed(3)).cuda()
    kw = dict(bn="batch", precision="mixed")

    def run():
        feat = engine.encoder_forward_train(img, **kw)
        n_fwd = len(calls)
        grad = engine.encoder_backward(img, gf, **kw)
        moved = engine.update_encoder_stats(engine.encoder_stats(), momentum=0.9, unbiased=True)
        return (feat, grad, engine.encoder_batch_stats(), moved), n_fwd

    calls = []
    plain, _ = run()
    assert calls == []
    hook = _lib.REDUCE_FN(lambda user, ptr, count, stream: calls.append(count) or 0)
    engine.set_encoder_reduce(hook, 2)
    try:
        hooked, n_fwd = run()
        assert n_fwd == N_LAYERS and len(calls) == 3 * N_LAYERS
        assert sorted(calls[:N_LAYERS]) == sorted(2 * s.cout for s in CONV_SPECS)
        # B above the global batch; a stream in capture: both refused before any launch or hook call
        lib, h, n = engine.lib, engine._h, len(calls)
        three = torch.zeros(3, 224, 224, 3, device="cuda")
        out, gflat = torch.empty(3, 2048, device="cuda"), torch.empty(resnet_spec.ENCODER_PARAM_FLOATS, device="cuda")
        assert lib.hpe_encoder_forward_batchnorm_mixed(h, three.data_ptr(), 3, out.data_ptr(), engine._stream()) == 1
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                rc_f = lib.hpe_encoder_forward_batchnorm_mixed(h, img.data_ptr(), 2, out.data_ptr(), engine._stream())
                msg = lib.hpe_last_error().decode()
                rc_b = lib.hpe_encoder_backward_batchnorm_mixed(h, img.data_ptr(), 2, gf.data_ptr(), gflat.data_ptr(), engine._stream())
                out.zero_()  # the graph is not empty
        torch.cuda.current_stream().wait_stream(side)
        assert (rc_f, rc_b) == (3, 3) and "captured" in msg and len(calls) == n
    finally:
        engine.set_encoder_reduce(None)
    for a, b in zip(plain, hooked):
        assert torch.equal(a, b)
    n = len(calls)
    again, _ = run()  # the hook cleared: the plain path, bit for bit, and no call
    assert len(calls) == n
    for a, b in zip(plain, again):
        assert torch.equal(a, b)


def _run_two_ranks(params, images, shards, gf):
    """test_gpu_encoder_bn_reduce.run_two_ranks on the mixed walk: one engine and one Python thread per rank, the hooks meet in a Meeting"""
    G = images.shape[0]
    meet = Meeting()
    engines = [make_engine(params, max_batch=2, reserve=0) for _ in shards]
    out, failures = [None] * len(shards), []
    kw = dict(bn="batch", precision="mixed")

    def work(r):
        try:
            e, (lo, hi) = engines[r], shards[r]
            img = images[lo:hi].contiguous().cuda()
            out[r] = {"feat": e.encoder_forward_train(img, **kw), "grad": e.encoder_backward(img, gf[lo:hi].contiguous().cuda(), **kw)}
        except BaseException as e:  # noqa: B902
            failures.append((r, repr(e)))
            meet.barrier.abort()

    try:
        hooks = [meet.hook(r) for r in range(len(shards))]
        for e, h, (lo, hi) in zip(engines, hooks, shards):
            e.reserve_encoder_train(hi - lo, batch_norm=True, precision="mixed")
            e.set_encoder_reduce(h, G)
        threads = [threading.Thread(target=work, args=(r,)) for r in range(len(shards))]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=120)
        assert not any(t.is_alive() for t in threads), "a rank did not finish"
        assert not failures and not meet.errors, (failures, meet.errors)
        torch.cuda.synchronize()
        for e, o in zip(engines, out):
            o["stash"] = [e.encoder_stash(i, precision="mixed").float().cpu() for i in range(N_LAYERS)]
            o["zstash"] = [e.encoder_stash_raw(i, precision="mixed").float().cpu() for i in range(N_LAYERS)]
            o["pooled"], o["bstats"] = e.encoder_stash(-1, precision="mixed").float().cpu(), e.encoder_batch_stats().cpu()
            o["feat"], o["grad"] = o["feat"].cpu(), o["grad"].cpu()
    finally:
        for e in engines:
            e.close()
    return out


def test_two_ranks(params):
    """shards 1 + 1 of the G = 2 images of ``whole``: every rank holds the same statistics bits, those of the concatenated z16; the sum of
    the two flat gradients (what one SUM all-reduce leaves on every rank) against the restatements driven by the concatenated stashes"""
    img = synthetic.make_images(2, seed=31)
    images = torch.from_numpy(img)
    gf = torch.randn(2, 2048, generator=torch.Generator().manual_seed(3))
    ranks = _run_two_ranks(params, images, [(0, 1), (1, 2)], gf)
    assert torch.equal(ranks[0]["bstats"], ranks[1]["bstats"])
    cat = lambda k: [torch.cat([r[k][i] for r in ranks]) for i in range(N_LAYERS)]  # noqa: E731
    stash, zstash, pooled = cat("stash"), cat("zstash"), torch.cat([r["pooled"] for r in ranks])
    b, worst = ranks[0]["bstats"], 0.0
    for i, (s, (om, ov)) in enumerate(zip(CONV_SPECS, ENCODER_STAT_OFFSETS)):
        emu, evar = _stats_errors(b[om:om + s.cout], b[ov:ov + s.cout], zstash[i])
        worst = max(worst, emu, evar)
        assert emu <= ULP4 and evar <= ULP4, (s.name, emu, evar)
    print("two ranks 1 + 1, mixed: statistics worst %.3g (bar %.3g)" % (worst, ULP4))
    win = R.maxpool_winners(stash[0])
    ref = RB.network_backward(_p16(params), X.rne(images), zstash, stash, pooled, win, gf)
    mixed = XB.network_backward_mixed(params, images, zstash, stash, pooled, win, gf)
    _check_network_grad(ranks[0]["grad"] + ranks[1]["grad"], ref, mixed, "two ranks")


def test_refusals(engine, params):
    lib, h = engine.lib, engine._h
    img = torch.zeros(4, 224, 224, 3, device="cuda")
    gf = torch.zeros(4, 2048, device="cuda")
    out = torch.zeros(resnet_spec.ENCODER_PARAM_FLOATS, device="cuda")
    stats = torch.zeros(resnet_spec.ENCODER_STAT_FLOATS, device="cuda")
    x16 = torch.zeros(1, 112, 112, 64, dtype=BF, device="cuda")
    st = engine._stream()
    i, g, o, t, x = img.data_ptr(), gf.data_ptr(), out.data_ptr(), stats.data_ptr(), x16.data_ptr()
    fwd, bwd = lib.hpe_encoder_forward_batchnorm_mixed, lib.hpe_encoder_backward_batchnorm_mixed
    assert bwd(h, None, 1, g, o, st) == 1 and bwd(h, i, 1, None, o, st) == 1 and bwd(h, i, 1, g, None, st) == 1
    assert bwd(h, i, 0, g, o, st) == 1 and bwd(h, i, 4, g, o, st) == 1  # reserved for 3
    assert fwd(h, i, 4, g, st) == 1 and fwd(h, i, 0, g, st) == 1 and fwd(h, None, 1, g, st) == 1 and fwd(h, i, 1, None, st) == 1
    assert lib.hpe_encoder_train_reserve_batchnorm_mixed(h, 2) == 0 and lib.hpe_encoder_train_reserve_batchnorm_mixed(h, 4) == 3  # a no-op; larger
    dbg, dbw = lib.hpe_debug_conv_batchnorm_mixed, lib.hpe_debug_conv_backward_batchnorm_mixed
    assert dbg(h, 53, x, 1, None, 1, x, x, t, st) == 1 and dbg(h, -1, x, 1, None, 1, x, x, t, st) == 1
    assert dbg(h, 1, x, 4, None, 1, x, x, t, st) == 1 and dbg(h, 1, x, 0, None, 1, x, x, t, st) == 1
    assert dbg(h, 1, None, 1, None, 1, x, x, t, st) == 1 and dbg(h, 1, x, 1, None, 1, None, x, t, st) == 1
    assert dbg(h, 1, x, 1, None, 1, x, None, t, st) == 1 and dbg(h, 1, x, 1, None, 1, x, x, None, st) == 1
    assert dbw(h, 0, i, x, x, x, 1, x, o, st) == 1  # conv1 has no data gradient
    assert dbw(h, 1, x, None, x, x, 1, None, o, st) == 1 and dbw(h, 1, None, x, x, x, 1, None, o, st) == 1
    assert dbw(h, 1, x, x, x, None, 1, None, o, st) == 1 and dbw(h, 1, x, x, x, x, 1, None, None, st) == 1
    assert dbw(h, 53, x, x, x, x, 1, None, o, st) == 1 and dbw(h, 1, x, x, x, x, 4, None, o, st) == 1
    raw = lib.hpe_debug_encoder_stash_raw_mixed
    assert raw(h, -1, o, st) == 1 and raw(h, 53, o, st) == 1 and raw(h, 0, None, st) == 1
    with pytest.raises(ValueError):
        engine.encoder_forward_train(img[:1], bn="batch", precision="fp16")
    for first in ({"precision": "bf16"}, {"batch_norm": True}):  # only the mixed reserve / only the batch-norm reserve
        one = make_engine(params, max_batch=2, reserve=0)
        try:
            one.reserve_encoder_train(1, **first)
            f = one._h
            assert bwd(f, i, 1, g, o, st) == 3 and fwd(f, i, 1, g, st) == 3
            assert dbg(f, 1, x, 1, None, 1, x, x, t, st) == 3 and dbw(f, 1, x, x, x, x, 1, None, o, st) == 3 and raw(f, 1, o, st) == 3
            assert lib.hpe_encoder_train_reserve_batchnorm_mixed(f, 3) == 1  # above max_batch
            assert lib.hpe_encoder_train_reserve_batchnorm_mixed(f, 2) == 3  # the reserve it shares was made for 1
            one.reserve_encoder_train(1, batch_norm=True, precision="mixed")  # ... and beside it for 1
            assert raw(f, 1, o, st) == 3  # no mixed batch-mode forward yet
            assert fwd(f, i, 1, g, st) == 0 and raw(f, 1, o, st) == 0
        finally:
            one.close()
    bf = make_engine(params, max_batch=2, reserve=0, encoder_dtype="bf16")
    try:
        assert lib.hpe_encoder_train_reserve_batchnorm_mixed(bf._h, 1) == 3
        assert bwd(bf._h, i, 1, g, o, st) == 3 and fwd(bf._h, i, 1, g, st) == 3
        assert dbg(bf._h, 1, x, 1, None, 1, x, x, t, st) == 3
    finally:
        bf.close()


def test_generator_trainer():
    """GeneratorTrainer(train_encoder=True, encoder_bn="batch", encoder_precision="mixed") on the fixed batch of 4 and fixed masks of
    tests/test_gpu_encoder_bn_train.py::test_trainer (synthetic.py's own encoder)"""
    params = synthetic.make_encoder_params()
    e = hpe_amd.HpeEngine(device=0, max_batch=4)
    try:
        e.load_smpl(synthetic.make_smpl_model())
        e.load_encoder(params)
        e.load_regressor(synthetic.make_regressor_params(variant="bounded"))
        e.load_mean_theta(O.load_mean_param(synthetic.make_mean_params()))
        e.finalize()
        e.reserve_encoder_train(4, batch_norm=True, precision="mixed")
        img = torch.from_numpy(synthetic.make_images(4, seed=13)).cuda()
        g = torch.Generator().manual_seed(4)
        kp = torch.cat([torch.rand(4, 19, 2, generator=g) * 1.2 - 0.6, torch.ones(4, 19, 1)], 2).cuda()
        tr = hpe_amd.GeneratorTrainer(e, dropout=0.5, generator=torch.Generator(device="cuda").manual_seed(1), train_encoder=True, encoder_bn="batch",
                                      encoder_precision="mixed")
        masks = tr.draw_masks(4)
        p0, s0 = tr.encoder_params.detach().clone(), tr.encoder_stats.clone()
        losses = [float(tr.step(img, kp, use_critic=False, drop=masks)["kpr_losses"][-1])]
        # after step one: the momentum formula (Keras' 0.99, unbiased) on that step's batch statistics
        ref = RB.momentum_update(s0.cpu().double(), e.encoder_batch_stats().cpu().double(), 4, 0.99, True)
        assert float(((tr.encoder_stats.cpu().double() - ref).abs() / ref.abs()).max()) <= ULP4
        losses += [float(tr.step(img, kp, use_critic=False, drop=masks)["kpr_losses"][-1]) for _ in range(4)]
        print("60 * kp loss over 5 steps with the encoder in the update, mixed precision, batch statistics:", losses)
        assert losses[-1] < losses[0]
        now = tr.encoder_params.detach()
        assert not torch.equal(now, p0) and torch.equal(e.encoder_params(), now)
        assert not torch.equal(tr.encoder_stats, s0) and torch.equal(e.encoder_stats(), tr.encoder_stats)
        feat = e.encoder(img)
        fresh = hpe_amd.HpeEngine(device=0, max_batch=4)
        try:
            fresh.load_encoder(resnet_spec.flat_to_params(now.cpu(), resnet_spec.stats_to_params(tr.encoder_stats)))
            fresh.finalize()
            assert torch.equal(feat, fresh.encoder(img))
        finally:
            fresh.close()
    finally:
        e.close()


def _trainer_inputs(tr, steps):
    """one fixed batch and fixed draws, as tests/test_gpu_trainer.py's ``runs``"""
    images, segs, kp = tr._load_images(next(iter(tr.dataset)))
    real = tr._load_mocap(next(iter(tr.mocap_dataset)))
    g = torch.Generator(device="cuda").manual_seed(3)
    drops = [tr.generator.draw_masks(TRAINER_B) for _ in range(steps)]
    N = TRAINER_B * STAGES
    interps = [(torch.rand((N, 14, 3), generator=g, device="cuda"), torch.rand((N, 10), generator=g, device="cuda"),
                torch.rand((N, 24, 3, 3), generator=g, device="cuda")) for _ in range(steps)]
    return images, segs, kp, real, drops, interps


def test_trainer_mixed_steps_and_checkpoint(weights, data, tmp_path):  # noqa: F811
    """a Trainer with config.encoder_precision = "mixed": two train_steps move every tensor, and save() / restore() round-trips into a
    second one (the masters are fp32: the checkpoint is the fp32 Trainer's)"""
    a = make_trainer(weights, data, tmp_path / "a", encoder_precision="mixed")
    try:
        assert a.generator.encoder_precision == "mixed" and a.generator.encoder_bn == "batch"
        images, segs, kp, real, drops, interps = _trainer_inputs(a, 3)
        start = tensors_of(a)
        for i in range(2):
            r = a.train_step(images, segs, kp, *real, drop=drops[i], interp=interps[i])
            assert all(bool(torch.isfinite(t).all()) for t in result_tensors(r))
        after2 = tensors_of(a)
        for k in start:
            assert not torch.equal(start[k], after2[k]), k
        assert a.engine.lib.hpe_debug_encoder_stash_batch_mixed(a.engine._h) == TRAINER_B  # the mixed walk ran
        prefix = a.save()
        third = result_tensors(a.train_step(images, segs, kp, *real, drop=drops[2], interp=interps[2]))
    finally:
        a.engine.close()
    b = make_trainer(weights, data, tmp_path / "b", encoder_precision="mixed")
    try:
        assert b.restore(str(tmp_path / "a"), verify=False) == prefix
        for k, t in after2.items():
            assert same(tensors_of(b)[k], t), k
        for x, y in zip(third, result_tensors(b.train_step(images, segs, kp, *real, drop=drops[2], interp=interps[2]))):
            assert same(x, y)
    finally:
        b.engine.close()


def test_trainer_fp32_is_the_default(weights, data, tmp_path):  # noqa: F811
    """config.encoder_precision = "fp32" is a Trainer without the attribute, bit for bit over two steps; anything else is refused"""
    outs = []
    for n, kw in enumerate(({}, {"encoder_precision": "fp32"})):
        tr = make_trainer(weights, data, tmp_path / str(n), **kw)
        try:
            images, segs, kp, real, drops, interps = _trainer_inputs(tr, 2)
            res = [result_tensors(tr.train_step(images, segs, kp, *real, drop=drops[i], interp=interps[i])) for i in range(2)]
            outs.append(res[0] + res[1] + list(tensors_of(tr).values()))
            assert tr.engine.lib.hpe_debug_encoder_stash_batch_mixed(tr.engine._h) == 0
        finally:
            tr.engine.close()
    assert len(outs[0]) == len(outs[1])
    for x, y in zip(*outs):
        assert same(x, y)
    with pytest.raises(ValueError, match="encoder_precision"):
        make_trainer(weights, data, tmp_path / "bad", encoder_precision="bf16")
