"""Mixed-precision encoder training on the GPU: bf16 walks on an fp32 context (hpe_encoder_*_mixed) against the CPU restatements of
tests/encoder_train_ref.py (float64, with the kernels replaced by W16 = RNE(W)) and tests/encoder_mixed_ref.py (float32 with the
roundings of the contract).  Every bar comes from those restatements on the same inputs, never from the code under test:

  fp32 results (dW, db, dgamma, dbeta)  norm-relative error below 4 x that of the same restatement in float32 (the rule and the margin of
                                        tests/test_gpu_encoder_train.py)
  bf16 results (dx, the stash)          per element, the bound of tests/gemm_ref.py: 2^-8 |ref| for the one final rounding, plus 4 x the
                                        float32 restatement's own error (dx) or the project's per-layer forward bar (the stash)
  the whole network's gradient          norm-relative error below 4 x that of network_backward_mixed on the same stash"""
import ctypes as C

import numpy as np
import pytest
import torch

import encoder_mixed_ref as X
import encoder_train_ref as R
import hpe_amd
from gemm_ref import BF16_ULP, ORDER_MARGIN
from hpe_amd import _lib, resnet_spec, synthetic
from hpe_amd.resnet_spec import CONV_SPECS, ENCODER_PARAM_OFFSETS
from oracle import hmr_oracle as O
from test_gpu_encoder_train import FORWARD_BAR, MARGIN, make_engine, make_params

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


@pytest.fixture(scope="module")
def params():
    return make_params()


@pytest.fixture(scope="module")
def engine(params):
    e = make_engine(params)  # fp32, max_batch 4, fp32 reserve of 3
    e.reserve_encoder_train(3, precision="bf16")
    yield e
    e.close()


def _dev16(t):
    return t.to(BF).cuda()


def _w16(params, s):
    lt = R.layer_tensors(params, s, torch.float32)
    return lt, X.weights16(lt)


def _check_layer(engine, params, idx, B, x, y, dy, tag):
    """one debug_conv_backward(precision="bf16") call against the restatements; y None: ungated"""
    s = CONV_SPECS[idx]
    gated = y is not None
    xd = x.cuda() if idx == 0 else _dev16(x)
    dx, gl = engine.debug_conv_backward(idx, xd, _dev16(y) if gated else None, _dev16(dy), precision="bf16")
    torch.cuda.synchronize()
    lt, lt16 = _w16(params, s)
    x16 = X.rne(x) if idx == 0 else x  # the bf16 pad rounds the pixels
    ref = R.layer_backward(s, x16.double(), y, dy.double(), [t.double() for t in lt16], want_dx=False, gated=gated)
    f32 = R.layer_backward(s, x16, y, dy, lt16, want_dx=False, gated=gated)
    got = R.split_layer_grad(s, gl.cpu())
    for k, v in got.items():
        e, bar = R.rel(v, ref[k]), MARGIN * R.rel(f32[k], ref[k])
        print("layer %2d %-16s B=%d %-6s %s gpu %.3g  bar %.3g" % (idx, s.name, B, k, tag, e, bar))
        # a sum of a few hundred bf16 values is exact in fp32 (dbeta on the small maps): the restatement's error, and so the bar, is 0 there,
        # and only an exact result passes
        assert e < bar or e == 0.0, (s.name, k, e, bar)
    if idx == 0:
        assert dx is None
        return
    # dx: float64 on the operands the GEMM read -- dzs as rounding point 5 gives it (one fp32 multiply by the context's folded scale, one
    # rounding: bit-reproducible here) and W16 -- with the element-wise bound of tests/gemm_ref.py
    assert dx.dtype == BF
    dzs = X.rne(f32["dz"] * X.folded_scale(lt))
    W16 = lt16[0]
    dref = X.data_grad_mixed(s, dzs.double(), W16.double(), B, rounding=False)
    A = X.data_grad_mixed(s, dzs.abs().double(), W16.abs().double(), B, rounding=False)
    d32 = X.data_grad_mixed(s, dzs, W16, B, rounding=False).double()  # the float32 restatement before the final rounding
    live = A > 0
    e32 = float(((d32 - dref).abs()[live] / A[live]).max())
    err = (dx.float().cpu().double() - dref).abs()
    bound = BF16_ULP * dref.abs() + ORDER_MARGIN * e32 * A
    worst = float((err[live] / bound[live]).max())
    print("layer %2d %-16s B=%d dx     %s worst element at %.3g of its bound (e32 %.3g)" % (idx, s.name, B, tag, worst, e32))
    assert bool((err <= bound).all()), (s.name, worst)  # where A == 0 (the odd pixels of a stride-2 layer) only an exact 0 passes


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("idx", range(len(CONV_SPECS)))
def test_layer_backward(engine, params, idx, B):
    s = CONV_SPECS[idx]
    g = torch.Generator().manual_seed(2000 * B + idx)
    x = torch.randn(B, s.hin, s.hin, s.cin, generator=g)
    x = x if idx == 0 else X.rne(x)  # conv1 takes the float32 images
    dy = X.rne(torch.randn(B, s.hout, s.hout, s.cout, generator=g))
    y = X.rne(torch.relu(torch.randn(B, s.hout, s.hout, s.cout, generator=g)))  # its sign is the gate
    _check_layer(engine, params, idx, B, x, y, dy, "gated  ")
    if s.name.endswith("branch1"):  # as the network runs a projection shortcut: no activation, y_dev NULL, dz = dy
        _check_layer(engine, params, idx, B, x, None, dy, "ungated")
    if B * s.hout * s.hout > 256:  # more than one slice of pixels: the fix-up sums partials
        assert engine.lib.hpe_encoder_wg_slices(idx, B) > 1
    if idx == 0 or (B == 3 and s.hout == 56):
        assert engine.lib.hpe_encoder_wg_slices(idx, B) > 1


def test_pool_backwards(engine):
    """the tie and all-zero-window cases of test_gpu_encoder_train.py::test_pool_backwards on bf16 inputs: exactly the restatement's RNE"""
    g = torch.Generator().manual_seed(5)
    x = X.rne(torch.relu(torch.randn(2, 16, 16, 8, generator=g)))
    x[0, 4:9, 4:9, :] = 1.5   # exact positive ties
    x[1, :6, :6, :] = 0.0     # all-zero windows, on the border and inside
    dy = X.rne(torch.randn(2, 8, 8, 8, generator=g))
    got = engine.debug_maxpool_backward(_dev16(x), _dev16(dy), precision="bf16")
    assert got.dtype == BF
    got = got.float().cpu()
    ref = X.rne(R.maxpool_backward(R.maxpool_winners(x), dy, 16))
    assert torch.equal(got, ref)
    assert float(got[0, 6, 6].abs().max()) == 0.0 and float(got[0, 5, 5].abs().min()) > 0.0
    dyf = torch.randn(3, 64, generator=g)
    got = engine.debug_avgpool_backward(dyf.cuda(), 49, precision="bf16")
    assert got.dtype == BF
    assert torch.equal(got.float().cpu(), X.rne(R.avgpool_backward(dyf, 49)))


@pytest.fixture(scope="module")
def whole(engine, params):
    """B = 2: one mixed forward and backward, the mixed stash, and the float64 / mixed restatements driven by that stash"""
    B = 2
    img = synthetic.make_images(B, seed=31)
    gf = torch.randn(B, 2048, generator=torch.Generator().manual_seed(3))
    imgs = torch.from_numpy(img).cuda()
    feat = engine.encoder_forward_train(imgs, precision="bf16").cpu()
    grad = engine.encoder_backward(imgs, gf.cuda(), precision="bf16").cpu()
    assert engine.lib.hpe_debug_encoder_stash_batch_mixed(engine._h) == B
    st16 = [engine.encoder_stash(i, precision="bf16") for i in range(len(CONV_SPECS))]
    assert all(t.dtype == BF for t in st16)
    stash = [t.float().cpu() for t in st16]
    pooled = engine.encoder_stash(-1, precision="bf16").float().cpu()
    win = R.maxpool_winners(stash[0])
    p16 = dict(params)
    for s in CONV_SPECS:
        p16[s.name + "/kernel"] = X.rne(torch.from_numpy(np.asarray(params[s.name + "/kernel"], np.float32))).numpy()
    img16 = X.rne(torch.from_numpy(img))
    ref = R.network_backward(p16, img16, stash, pooled, win, gf)
    mixed = X.network_backward_mixed(params, torch.from_numpy(img), stash, pooled, win, gf)
    return dict(img=img, img16=img16, feat=feat, grad=grad, stash=stash, pooled=pooled, ref=ref, mixed=mixed, gf=gf, p16=p16)


def test_stash_consistency(whole):
    """every stashed layer output against float64 from its stashed input with W16, within 2^-8 |value| (the one rounding) + the project's
    per-layer forward bar; the gates may differ only where the float64 value is inside that bound of zero"""
    st, bl = whole["stash"], R.blocks()
    inputs = {0: whole["img16"]}
    resid = {}
    for k, (i2a, i2b, i2c, i1) in enumerate(bl):
        xin = whole["pooled"] if k == 0 else st[bl[k - 1][2]]
        inputs[i2a], inputs[i2b], inputs[i2c] = xin, st[i2a], st[i2b]
        resid[i2c] = xin if i1 is None else st[i1]
        if i1 is not None:
            inputs[i1] = xin
    for i, s in enumerate(CONV_SPECS):
        relu = not s.name.endswith("branch1")
        z = R.layer_forward(s, inputs[i].double(), R.layer_tensors(whole["p16"], s), resid.get(i, None), relu=False)
        scale = float(st[i].abs().max())
        value = torch.relu(z) if relu else z
        worst = float(((st[i].double() - value).abs() / (BF16_ULP * value.abs() + FORWARD_BAR * scale)).max())
        if relu:
            differ = (st[i] > 0) != (z > 0)
            print("layer %2d %-16s gate mismatches %d of %d, worst element at %.3g of its bound" % (i, s.name, int(differ.sum()), differ.numel(), worst))
            if differ.any():
                assert bool((z[differ].abs() <= BF16_ULP * z[differ].abs() + FORWARD_BAR * scale).all())
        assert worst <= 1.0, (s.name, worst)
    pool_ref = torch.nn.functional.max_pool2d(torch.nn.functional.pad(st[0].permute(0, 3, 1, 2), (1, 1, 1, 1)), 3, 2).permute(0, 2, 3, 1)
    assert torch.equal(whole["pooled"], pool_ref)


def test_network_backward(whole):
    worst = (0.0, None)
    for i, (s, off) in enumerate(zip(CONV_SPECS, ENCODER_PARAM_OFFSETS)):
        n = s.kh * s.kw * s.cin * s.cout + 3 * s.cout
        got, ref, mx = (R.split_layer_grad(s, whole[k][off[0]:off[0] + n]) for k in ("grad", "ref", "mixed"))
        for k in got:
            e, bar = R.rel(got[k], ref[k]), MARGIN * R.rel(mx[k], ref[k])
            print("net layer %2d %-16s %-6s gpu %.3g  bar %.3g" % (i, s.name, k, e, bar))
            if e / bar > worst[0]:
                worst = (e / bar, (s.name, k, e, bar))
            assert e < bar, (s.name, k, e, bar)
    print("worst layer against its bar:", worst)


def test_forward_train_features(whole, params):
    """the features are the fp32 sum of the 49 stashed bf16 values over 49 (the sum's own fp32 error: 49 additions and one division, each
    within 2^-24 of the running magnitude), and, end to end, within one bf16 rounding (2^-8, rel-L2) of the float64 oracle run with the
    same rounding points: the two chains differ by fp32 summation order only, which moves an element by a bf16 ulp where a sum falls on a
    tie, a perturbation of the size of the roundings both chains make anyway"""
    last = whole["stash"][R.blocks()[-1][2]].double().reshape(2, 49, 2048)
    mean = last.sum(1) / 49
    err = (whole["feat"].double() - mean).abs()
    assert bool((err <= 51 * 2.0 ** -24 * last.abs().sum(1) / 49).all()), float(err.max())
    ref = O.resnet50_features(whole["img"], params, dtype=np.float64, act_round="bf16")
    f = whole["feat"].numpy().astype(np.float64)
    l2 = float(np.linalg.norm(f - ref) / np.linalg.norm(ref))
    print("mixed forward_train features vs the bf16-rounding float64 oracle: rel-L2 %.3g (bar 2^-8 = %.3g)" % (l2, BF16_ULP))
    assert l2 < BF16_ULP


def test_deterministic_and_capturable(engine, whole):
    imgs = torch.from_numpy(whole["img"]).cuda()
    gf = whole["gf"].cuda()
    a = engine.encoder_backward(imgs, gf, precision="bf16")
    engine.encoder_backward(imgs[:1].contiguous(), gf[:1].contiguous() * 2, precision="bf16")  # another call in between
    b = engine.encoder_backward(imgs, gf, precision="bf16")
    assert torch.equal(a, b) and torch.equal(a.cpu(), whole["grad"])
    out = torch.empty_like(a)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            _lib.check(engine.lib.hpe_encoder_backward_mixed(engine._h, imgs.data_ptr(), 2, gf.data_ptr(), out.data_ptr(), engine._stream()))
        for _ in range(2):
            out.zero_()
            graph.replay()
            side.synchronize()
            assert torch.equal(out, a)
    torch.cuda.current_stream().wait_stream(side)


def test_interleaved_with_fp32_walks(engine, whole):
    """mixed, fp32 frozen and fp32 batch-statistics backwards on one context, which share the weight gradient's scratch: each gives the
    bits it gives whatever ran before it, and the mixed stash counter is its own"""
    engine.reserve_encoder_train(3, batch_norm=True)
    imgs = torch.from_numpy(whole["img"]).cuda()
    gf = whole["gf"].cuda()
    run = {"m": lambda: engine.encoder_backward(imgs, gf, precision="bf16"), "f": lambda: engine.encoder_backward(imgs, gf),
           "b": lambda: engine.encoder_backward(imgs, gf, bn="batch")}
    first = {}
    for k in "mfbmbfmffbbm":
        r = run[k]()
        assert torch.equal(r, first.setdefault(k, r)), k
    assert torch.equal(first["m"].cpu(), whole["grad"])
    assert not torch.equal(first["m"], first["f"])
    engine.encoder_forward_train(imgs[:1].contiguous())  # an fp32 forward of another batch
    assert engine.lib.hpe_debug_encoder_stash_batch(engine._h) == 1 and engine.lib.hpe_debug_encoder_stash_batch_mixed(engine._h) == 2
    assert torch.equal(engine.encoder_stash(3, precision="bf16").float().cpu(), whole["stash"][3])


def test_params_update_reaches_the_mixed_walk(params):
    """after set_encoder_params_dev(q) / set_encoder_params(q) the next mixed call computes with RNE(q), with no further call: its features
    equal those of a fresh context that loaded q"""
    e = make_engine(params, max_batch=2, reserve=0)
    try:
        e.reserve_encoder_train(2, precision="bf16")
        img = torch.from_numpy(synthetic.make_images(2, seed=9)).cuda()
        p = e.encoder_params().cpu()
        f0 = e.encoder_forward_train(img, precision="bf16").cpu()
        d = torch.randn(p.shape, generator=torch.Generator().manual_seed(2))
        q = p + d * (1e-2 * float(p.norm()) / float(d.norm()))
        e.set_encoder_params_dev(q.cuda())
        f1 = e.encoder_forward_train(img, precision="bf16").cpu()
        g1 = e.encoder_backward(img, torch.ones(2, 2048, device="cuda"), precision="bf16").cpu()
        e.set_encoder_params(p)
        assert torch.equal(e.encoder_forward_train(img, precision="bf16").cpu(), f0)  # the host setter, back to p
        fresh = make_engine(resnet_spec.flat_to_params(q, params), max_batch=2, reserve=0)
        try:
            fresh.reserve_encoder_train(2, precision="bf16")
            f2 = fresh.encoder_forward_train(img, precision="bf16").cpu()
            g2 = fresh.encoder_backward(img, torch.ones(2, 2048, device="cuda"), precision="bf16").cpu()
        finally:
            fresh.close()
        assert torch.equal(f1, f2) and torch.equal(g1, g2)
        assert not torch.equal(f1, f0)
    finally:
        e.close()


def test_every_batch_up_to_the_reserve(params):
    e = make_engine(params, max_batch=17, reserve=0)
    try:
        e.reserve_encoder_train(17, precision="bf16")
        img = torch.from_numpy(synthetic.make_images(17, seed=4)).cuda()
        gf = torch.randn(17, 2048, device="cuda")
        for B in range(1, 18):
            g = e.encoder_backward(img[:B].contiguous(), gf[:B].contiguous(), precision="bf16")
            assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, B
            assert e.lib.hpe_debug_encoder_stash_batch_mixed(e._h) == B
    finally:
        e.close()


def test_refusals(engine, params):
    lib, h = engine.lib, engine._h
    img = torch.zeros(4, 224, 224, 3, device="cuda")
    gf = torch.zeros(4, 2048, device="cuda")
    out = torch.zeros(resnet_spec.ENCODER_PARAM_FLOATS, device="cuda")
    st = engine._stream()
    assert lib.hpe_encoder_backward_mixed(h, None, 1, gf.data_ptr(), out.data_ptr(), st) == 1
    assert lib.hpe_encoder_backward_mixed(h, img.data_ptr(), 1, None, out.data_ptr(), st) == 1
    assert lib.hpe_encoder_backward_mixed(h, img.data_ptr(), 1, gf.data_ptr(), None, st) == 1
    assert lib.hpe_encoder_backward_mixed(h, img.data_ptr(), 0, gf.data_ptr(), out.data_ptr(), st) == 1
    assert lib.hpe_encoder_backward_mixed(h, img.data_ptr(), 4, gf.data_ptr(), out.data_ptr(), st) == 1  # reserved for 3
    assert lib.hpe_encoder_forward_train_mixed(h, img.data_ptr(), 4, gf.data_ptr(), st) == 1
    assert lib.hpe_encoder_forward_train_mixed(h, None, 1, gf.data_ptr(), st) == 1
    assert lib.hpe_encoder_train_reserve_mixed(h, 2) == 0 and lib.hpe_encoder_train_reserve_mixed(h, 4) == 3  # a no-op; larger: refused
    x16 = torch.zeros(1, 112, 112, 64, dtype=BF, device="cuda")
    assert lib.hpe_debug_conv_backward_mixed(h, 0, img.data_ptr(), x16.data_ptr(), x16.data_ptr(), 1, x16.data_ptr(), out.data_ptr(), st) == 1  # conv1 with dx
    assert lib.hpe_debug_conv_backward_mixed(h, 1, None, None, x16.data_ptr(), 1, None, out.data_ptr(), st) == 1
    assert lib.hpe_debug_conv_backward_mixed(h, 53, x16.data_ptr(), None, x16.data_ptr(), 1, None, out.data_ptr(), st) == 1
    assert lib.hpe_debug_encoder_stash_mixed(h, 0, None, st) == 1
    fresh = make_engine(params, max_batch=2, reserve=1)  # the fp32 reserve alone
    try:
        assert lib.hpe_encoder_backward_mixed(fresh._h, img.data_ptr(), 1, gf.data_ptr(), out.data_ptr(), st) == 3
        assert lib.hpe_encoder_forward_train_mixed(fresh._h, img.data_ptr(), 1, gf.data_ptr(), st) == 3
        assert lib.hpe_debug_encoder_stash_mixed(fresh._h, 0, out.data_ptr(), st) == 3
        assert lib.hpe_debug_encoder_stash_batch_mixed(fresh._h) == 0
        assert lib.hpe_encoder_train_reserve_mixed(fresh._h, 3) == 1  # above max_batch
        with pytest.raises(ValueError, match="follow-up"):
            fresh.encoder_backward(img[:1], gf[:1], bn="batch", precision="bf16")
        with pytest.raises(ValueError, match="follow-up"):
            fresh.reserve_encoder_train(1, batch_norm=True, precision="bf16")
        with pytest.raises(ValueError):
            fresh.encoder_forward_train(img[:1], precision="fp16")
    finally:
        fresh.close()
    bf = make_engine(params, max_batch=2, reserve=0, encoder_dtype="bf16")
    try:
        assert lib.hpe_encoder_train_reserve_mixed(bf._h, 1) == 3
        assert lib.hpe_encoder_backward_mixed(bf._h, img.data_ptr(), 1, gf.data_ptr(), out.data_ptr(), st) == 3
        assert lib.hpe_encoder_forward_train_mixed(bf._h, img.data_ptr(), 1, gf.data_ptr(), st) == 3
    finally:
        bf.close()


def test_autograd_function(engine, whole):
    """encoder_features(precision="bf16"): one .backward() fills the flat tensor's .grad with the bits of the mixed backward"""
    imgs = torch.from_numpy(whole["img"]).cuda()
    p = engine.encoder_params().requires_grad_(True)
    f = hpe_amd.encoder_features(engine, imgs, p, precision="bf16")
    assert f.dtype == torch.float32 and torch.equal(f.cpu(), whole["feat"])
    (f * whole["gf"].cuda()).sum().backward()
    assert p.grad.dtype == torch.float32 and torch.equal(p.grad.cpu(), whole["grad"])
    with pytest.raises(ValueError, match="follow-up"):
        hpe_amd.encoder_features(engine, imgs, p, bn="batch", precision="bf16")


def test_trainer():
    """GeneratorTrainer(train_encoder=True, encoder_precision="bf16") lowers the 60 * kp loss over 5 steps on the fixed batch and masks of
    test_gpu_encoder_train.py::test_trainer; with encoder_precision="fp32" two steps equal a trainer built without the argument, bit for bit"""
    params = synthetic.make_encoder_params()

    def build(precision):
        e = hpe_amd.HpeEngine(device=0, max_batch=4)
        e.load_smpl(synthetic.make_smpl_model())
        e.load_encoder(params)
        e.load_regressor(synthetic.make_regressor_params(variant="bounded"))
        e.load_mean_theta(O.load_mean_param(synthetic.make_mean_params()))
        e.finalize()
        e.reserve_encoder_train(4, precision=precision)
        return e

    img = torch.from_numpy(synthetic.make_images(4, seed=13)).cuda()
    g = torch.Generator().manual_seed(4)
    kp = torch.cat([torch.rand(4, 19, 2, generator=g) * 1.2 - 0.6, torch.ones(4, 19, 1)], 2).cuda()
    outs = []
    for kw in ({}, {"encoder_precision": "fp32"}):
        e = build("fp32")
        try:
            tr = hpe_amd.GeneratorTrainer(e, dropout=0.5, generator=torch.Generator(device="cuda").manual_seed(1), train_encoder=True, **kw)
            masks = tr.draw_masks(4)
            r = [tr.step(img, kp, use_critic=False, drop=masks) for _ in range(2)]
            outs.append((r[-1]["kpr_losses"][-1].cpu(), r[-1]["pred_keypoints"].cpu(), r[-1]["grad_features"].cpu(), tr.params.detach().cpu(),
                         tr.encoder_params.detach().cpu()))
            with pytest.raises(ValueError, match="follow-up"):
                hpe_amd.GeneratorTrainer(e, train_encoder=True, encoder_bn="batch", encoder_precision="bf16")
        finally:
            e.close()
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    e = build("bf16")
    try:
        tr = hpe_amd.GeneratorTrainer(e, dropout=0.5, generator=torch.Generator(device="cuda").manual_seed(1), train_encoder=True, encoder_precision="bf16")
        masks = tr.draw_masks(4)
        p0 = tr.encoder_params.detach().clone()
        losses = [float(tr.step(img, kp, use_critic=False, drop=masks)["kpr_losses"][-1]) for _ in range(5)]
        print("60 * kp loss over 5 steps with the encoder in the update, bf16 walks:", losses)
        assert losses[-1] < losses[0]
        assert not torch.equal(tr.encoder_params.detach(), p0) and torch.equal(e.encoder_params(), tr.encoder_params.detach())
        assert not torch.equal(tr.encoder_params.detach().cpu(), outs[0][4])  # not the fp32 walk's update
    finally:
        e.close()
