"""Encoder training on the GPU (fp32, frozen BatchNorm statistics): every layer's gate / weight gradient / data gradient, the pool
backwards, the stash, the whole-network backward, the call contract and the parameter update, against the float64 restatement of
tests/encoder_train_ref.py.  Every bar is 4 x the error of the SAME restatement run in float32 on the CPU on the same inputs (the margin
is for a different but equally valid summation order), never a figure of the code under test."""
import ctypes as C

import numpy as np
import pytest
import torch

import encoder_train_ref as R
import hpe_amd
from hpe_amd import _lib, resnet_spec, synthetic
from hpe_amd.resnet_spec import CONV_SPECS, ENCODER_PARAM_OFFSETS
from oracle import hmr_oracle as O

pytestmark = pytest.mark.gpu
MARGIN = 4.0
FORWARD_BAR = 5e-5  # tests/test_gpu_parity.py: per-layer max error over the layer's largest output


def make_params():
    """synthetic.py's encoder with gamma in [0.5, 1.5] on every layer, non-trivial mean / var / bias"""
    p = synthetic.make_encoder_params(seed=7)
    g = np.random.default_rng(11)
    for s in CONV_SPECS:
        p[s.bn_name + "/gamma"] = g.uniform(0.5, 1.5, s.cout).astype(np.float32)
    return p


def make_engine(params, max_batch=4, reserve=3, **kw):
    e = hpe_amd.HpeEngine(device=0, max_batch=max_batch, **kw)
    e.load_encoder(params)
    e.finalize()
    if reserve:
        e.reserve_encoder_train(reserve)
    return e


@pytest.fixture(scope="module")
def params():
    return make_params()


@pytest.fixture(scope="module")
def engine(params):
    e = make_engine(params)
    yield e
    e.close()


def _t(a):
    return torch.as_tensor(np.asarray(a))


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("idx", range(len(CONV_SPECS)))
def test_layer_backward(engine, params, idx, B):
    s = CONV_SPECS[idx]
    g = torch.Generator().manual_seed(1000 * B + idx)
    x = torch.randn(B, s.hin, s.hin, s.cin, generator=g)
    res = torch.randn(B, s.hout, s.hout, s.cout, generator=g) if s.name.endswith("2c") else None
    dy = torch.randn(B, s.hout, s.hout, s.cout, generator=g)
    y = engine.debug_conv(idx, x.cuda(), res.cuda() if res is not None else None, relu=True)
    dx, gl = engine.debug_conv_backward(idx, x.cuda(), y, dy.cuda())
    torch.cuda.synchronize()
    y = y.cpu()  # the SAME fp32 y gates the restatement: the gates agree by construction
    ref = R.layer_backward(s, x.double(), y, dy.double(), R.layer_tensors(params, s))
    f32 = R.layer_backward(s, x, y, dy, R.layer_tensors(params, s, torch.float32))
    got = R.split_layer_grad(s, gl.cpu())
    if idx != 0:
        got["dx"] = dx.cpu()
    for k, v in got.items():
        e, bar = R.rel(v, ref[k]), MARGIN * R.rel(f32[k], ref[k])
        print("layer %2d %-16s B=%d %-6s gpu %.3g  bar %.3g" % (idx, s.name, B, k, e, bar))
        assert e < bar, (s.name, k, e, bar)
    if s.name.endswith("branch1"):  # as the network runs a projection shortcut: no activation, y_dev NULL, dz = dy
        dx, gl = engine.debug_conv_backward(idx, x.cuda(), None, dy.cuda())
        ref = R.layer_backward(s, x.double(), None, dy.double(), R.layer_tensors(params, s), gated=False)
        f32 = R.layer_backward(s, x, None, dy, R.layer_tensors(params, s, torch.float32), gated=False)
        got = dict(R.split_layer_grad(s, gl.cpu()), dx=dx.cpu())
        for k, v in got.items():
            e, bar = R.rel(v, ref[k]), MARGIN * R.rel(f32[k], ref[k])
            print("layer %2d %-16s B=%d %-6s ungated gpu %.3g  bar %.3g" % (idx, s.name, B, k, e, bar))
            assert e < bar, (s.name, k, e, bar)
    if B * s.hout * s.hout > 256:  # more than one slice of pixels: the fix-up sums partials
        assert engine.lib.hpe_encoder_wg_slices(idx, B) > 1
    if idx == 0 or (B == 3 and s.hout == 56):
        assert engine.lib.hpe_encoder_wg_slices(idx, B) > 1


def test_pool_backwards(engine):
    g = torch.Generator().manual_seed(5)
    x = torch.relu(torch.randn(2, 16, 16, 8, generator=g))
    x[0, 4:9, 4:9, :] = 1.5   # exact positive ties
    x[1, :6, :6, :] = 0.0     # all-zero windows, on the border and inside
    dy = torch.randn(2, 8, 8, 8, generator=g)
    got = engine.debug_maxpool_backward(x.cuda(), dy.cuda()).cpu()
    ref = R.maxpool_backward(R.maxpool_winners(x.double()), dy.double(), 16)
    assert torch.equal(got.double(), ref.to(torch.float32).double()) or R.rel(got, ref) < 1e-7
    # the window of rows 5..7, columns 5..7 is all 1.5: (5, 5) receives, (6, 6), which no other window holds, does not
    assert float(got[0, 6, 6].abs().max()) == 0.0 and float(got[0, 5, 5].abs().min()) > 0.0
    dyf = torch.randn(3, 64, generator=g)
    got = engine.debug_avgpool_backward(dyf.cuda(), 49).cpu()
    assert R.rel(got, R.avgpool_backward(dyf.double(), 49)) < 1e-7


@pytest.fixture(scope="module")
def whole(engine, params):
    """B = 2: one backward, the stash it left, and the float64 / float32 restatements driven by that stash"""
    B = 2
    img = synthetic.make_images(B, seed=31)
    gf = torch.randn(B, 2048, generator=torch.Generator().manual_seed(3))
    imgs = torch.from_numpy(img).cuda()
    feat = engine.encoder_forward_train(imgs).cpu()
    grad = engine.encoder_backward(imgs, gf.cuda()).cpu()
    stash = [engine.encoder_stash(i).cpu() for i in range(len(CONV_SPECS))]
    pooled = engine.encoder_stash(-1).cpu()
    win = R.maxpool_winners(stash[0])
    ref = R.network_backward(params, torch.from_numpy(img), stash, pooled, win, gf)
    f32 = R.network_backward(params, torch.from_numpy(img), stash, pooled, win, gf, dtype=torch.float32)
    return dict(img=img, feat=feat, grad=grad, stash=stash, pooled=pooled, ref=ref, f32=f32, gf=gf)


def test_stash_consistency(whole, params):
    """every stashed layer output against float64 from its stashed input: the gates may differ only where the float64 value is within the
    project's per-layer forward bar of zero"""
    st, bl = whole["stash"], R.blocks()
    inputs = {0: torch.from_numpy(whole["img"])}
    resid = {}
    for k, (i2a, i2b, i2c, i1) in enumerate(bl):
        xin = whole["pooled"] if k == 0 else st[bl[k - 1][2]]
        inputs[i2a], inputs[i2b], inputs[i2c] = xin, st[i2a], st[i2b]
        resid[i2c] = xin if i1 is None else st[i1]
        if i1 is not None:
            inputs[i1] = xin
    for i, s in enumerate(CONV_SPECS):
        relu = not s.name.endswith("branch1")
        z = R.layer_forward(s, inputs[i].double(), R.layer_tensors(params, s), resid.get(i, None), relu=False)
        scale = float(st[i].abs().max())
        if not relu:
            assert float((st[i].double() - z).abs().max()) <= FORWARD_BAR * scale
            continue
        differ = (st[i] > 0) != (z > 0)
        print("layer %2d %-16s gate mismatches %d of %d" % (i, s.name, int(differ.sum()), differ.numel()))
        assert float(z[differ].abs().max()) <= FORWARD_BAR * scale if differ.any() else True
        assert float((st[i].double() - torch.relu(z)).abs().max()) <= FORWARD_BAR * scale
    pool_ref = torch.nn.functional.max_pool2d(torch.nn.functional.pad(st[0].permute(0, 3, 1, 2), (1, 1, 1, 1)), 3, 2).permute(0, 2, 3, 1)
    assert torch.equal(whole["pooled"], pool_ref)


def test_network_backward(whole):
    worst = (0.0, None)
    for i, (s, off) in enumerate(zip(CONV_SPECS, ENCODER_PARAM_OFFSETS)):
        n = s.kh * s.kw * s.cin * s.cout + 3 * s.cout
        got, ref, f32 = (R.split_layer_grad(s, whole[k][off[0]:off[0] + n]) for k in ("grad", "ref", "f32"))
        for k in got:
            e, bar = R.rel(got[k], ref[k]), MARGIN * R.rel(f32[k], ref[k])
            print("net layer %2d %-16s %-6s gpu %.3g  bar %.3g" % (i, s.name, k, e, bar))
            if e / bar > worst[0]:
                worst = (e / bar, (s.name, k, e, bar))
            assert e < bar, (s.name, k, e, bar)
    print("worst layer against its bar:", worst)


def test_forward_train_features(whole, params):
    ref = O.resnet50_features(whole["img"], params, dtype=np.float64)
    e = float(np.abs(whole["feat"].numpy().astype(np.float64) - ref).max() / np.abs(ref).max())
    print("forward_train features vs fp64 oracle %.3g" % e)
    assert e < 2e-5


def test_deterministic_and_capturable(engine, whole):
    imgs = torch.from_numpy(whole["img"]).cuda()
    gf = whole["gf"].cuda()
    a = engine.encoder_backward(imgs, gf)
    engine.encoder_backward(imgs[:1].contiguous(), gf[:1].contiguous() * 2)  # another call in between
    b = engine.encoder_backward(imgs, gf)
    assert torch.equal(a, b) and torch.equal(a.cpu(), whole["grad"])
    out = torch.empty_like(a)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            _lib.check(engine.lib.hpe_encoder_backward(engine._h, imgs.data_ptr(), 2, gf.data_ptr(), out.data_ptr(), engine._stream()))
        for _ in range(2):
            out.zero_()
            graph.replay()
            side.synchronize()
            assert torch.equal(out, a)
    torch.cuda.current_stream().wait_stream(side)


def test_autograd_function(engine, whole):
    """encoder_features: one .backward() fills the flat tensor's .grad with the bits of encoder_backward"""
    imgs = torch.from_numpy(whole["img"]).cuda()
    p = engine.encoder_params().requires_grad_(True)
    f = hpe_amd.encoder_features(engine, imgs, p)
    assert torch.equal(f.cpu(), whole["feat"])
    (f * whole["gf"].cuda()).sum().backward()
    assert torch.equal(p.grad.cpu(), whole["grad"])


def test_smaller_batches_after_reserve(params):
    """batches below the reserved one run: the partial buffer covers the slice count of each (the count is not monotone in the batch)"""
    e = make_engine(params, max_batch=17, reserve=17)
    try:
        s = CONV_SPECS[0]
        x = torch.randn(16, 224, 224, 3, device="cuda")
        y = e.debug_conv(0, x, None, relu=True)
        dy = torch.randn(16, 112, 112, 64, device="cuda")
        _, g16 = e.debug_conv_backward(0, x, y, dy)
        _, g2 = e.debug_conv_backward(0, x[:2].contiguous(), y[:2].contiguous(), dy[:2].contiguous())
        assert bool(torch.isfinite(g16).all()) and bool(torch.isfinite(g2).all())
    finally:
        e.close()


def test_refusals(engine, params):
    lib, h = engine.lib, engine._h
    img = torch.zeros(4, 224, 224, 3, device="cuda")
    gf = torch.zeros(4, 2048, device="cuda")
    out = torch.zeros(resnet_spec.ENCODER_PARAM_FLOATS, device="cuda")
    st = engine._stream()
    assert lib.hpe_encoder_backward(h, None, 1, gf.data_ptr(), out.data_ptr(), st) == 1
    assert lib.hpe_encoder_backward(h, img.data_ptr(), 1, None, out.data_ptr(), st) == 1
    assert lib.hpe_encoder_backward(h, img.data_ptr(), 1, gf.data_ptr(), None, st) == 1
    assert lib.hpe_encoder_backward(h, img.data_ptr(), 0, gf.data_ptr(), out.data_ptr(), st) == 1
    assert lib.hpe_encoder_backward(h, img.data_ptr(), 4, gf.data_ptr(), out.data_ptr(), st) == 1  # reserved for 3
    assert lib.hpe_encoder_forward_train(h, img.data_ptr(), 4, gf.data_ptr(), st) == 1
    fresh = make_engine(params, max_batch=2, reserve=0)
    try:
        assert lib.hpe_encoder_backward(fresh._h, img.data_ptr(), 1, gf.data_ptr(), out.data_ptr(), st) == 3  # before reserve
        assert lib.hpe_encoder_get_params(fresh._h, out.data_ptr(), st) == 3
        assert lib.hpe_encoder_train_reserve(fresh._h, 3) == 1  # above max_batch
    finally:
        fresh.close()
    bf = make_engine(params, max_batch=2, reserve=0, encoder_dtype="bf16")
    try:
        assert lib.hpe_encoder_train_reserve(bf._h, 1) == 3
        assert lib.hpe_encoder_backward(bf._h, img.data_ptr(), 1, gf.data_ptr(), out.data_ptr(), st) == 3
        assert lib.hpe_encoder_set_params(bf._h, out.cpu().numpy().ctypes.data_as(C.c_void_p)) == 3
    finally:
        bf.close()


def test_update(params):
    e = make_engine(params, max_batch=2, reserve=1)
    try:
        img = torch.from_numpy(synthetic.make_images(2, seed=9)).cuda()
        p = e.encoder_params().cpu()
        assert np.array_equal(p.numpy(), resnet_spec.params_to_flat(params))
        f0 = e.encoder(img).cpu()
        g = torch.Generator().manual_seed(2)
        d = torch.randn(p.shape, generator=g)
        q = p + d * (1e-2 * float(p.norm()) / float(d.norm()))
        e.set_encoder_params(q)
        assert torch.equal(e.encoder_params().cpu(), q)
        f1 = e.encoder(img).cpu()
        fresh = make_engine(resnet_spec.flat_to_params(q, params), max_batch=2, reserve=0)
        try:
            f2 = fresh.encoder(img).cpu()
        finally:
            fresh.close()
        assert torch.equal(f1, f2)
        moved = float((f1 - f0).abs().max() / f0.abs().max())
        print("features moved by %.3g" % moved)
        assert moved > 2e-5  # the forward bar on features: the packings really were rewritten
    finally:
        e.close()


def test_trainer():
    """GeneratorTrainer(train_encoder=True) lowers the 60 * kp loss over 5 steps on a fixed batch of 4 with fixed masks; with the default
    its outputs equal those of a trainer built without the argument, bit for bit.  The encoder is synthetic.py's own (small gammas on the
    last BatchNorm of every bottleneck): with gamma in [0.5, 1.5] there the activations grow through the 16 residual adds and the
    untrained regressor's keypoints are off the image by orders of magnitude, which is no training problem."""
    params = synthetic.make_encoder_params()

    def build():
        e = hpe_amd.HpeEngine(device=0, max_batch=4)
        e.load_smpl(synthetic.make_smpl_model())
        e.load_encoder(params)
        e.load_regressor(synthetic.make_regressor_params(variant="bounded"))
        e.load_mean_theta(O.load_mean_param(synthetic.make_mean_params()))
        e.finalize()
        return e

    img = torch.from_numpy(synthetic.make_images(4, seed=13)).cuda()
    g = torch.Generator().manual_seed(4)
    kp = torch.cat([torch.rand(4, 19, 2, generator=g) * 1.2 - 0.6, torch.ones(4, 19, 1)], 2).cuda()
    outs = []
    for kw in ({}, {"train_encoder": False}):
        e = build()
        try:
            tr = hpe_amd.GeneratorTrainer(e, dropout=0.5, generator=torch.Generator(device="cuda").manual_seed(1), **kw)
            masks = tr.draw_masks(4)
            r = [tr.step(img, kp, use_critic=False, drop=masks) for _ in range(2)]
            outs.append((r[-1]["kpr_losses"][-1].cpu(), r[-1]["pred_keypoints"].cpu(), r[-1]["grad_features"].cpu(), tr.params.detach().cpu()))
        finally:
            e.close()
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    e = build()
    try:
        e.reserve_encoder_train(4)
        tr = hpe_amd.GeneratorTrainer(e, dropout=0.5, generator=torch.Generator(device="cuda").manual_seed(1), train_encoder=True)
        masks = tr.draw_masks(4)
        p0 = tr.encoder_params.detach().clone()
        losses = [float(tr.step(img, kp, use_critic=False, drop=masks)["kpr_losses"][-1]) for _ in range(5)]
        print("60 * kp loss over 5 steps with the encoder in the update:", losses)
        assert losses[-1] < losses[0]
        assert not torch.equal(tr.encoder_params.detach(), p0) and torch.equal(e.encoder_params(), tr.encoder_params.detach())
    finally:
        e.close()
