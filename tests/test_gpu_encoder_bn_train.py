"""Encoder training with batch statistics on the GPU (fp32): every layer's raw output, statistics, apply and backward, the whole-network
forward and backward, the moving-statistics update and its installation, the call contract and the trainer, against the float64
restatement of tests/encoder_bn_train_ref.py.  The statistics are held to four half-ulps of float (the sums are accumulated in double);
every other bar is 4 x the error of the SAME restatement run in float32 on the CPU on the same inputs (the margin is for a different but
equally valid operation order), never a figure of the code under test.

Figures of one run on an MI355X (worst over the 53 layers, GPU error / its bar): see DESIGN.md "Encoder training with batch statistics"."""
import numpy as np
import pytest
import torch

import encoder_bn_train_ref as RB
import encoder_train_ref as R
import hpe_amd
from hpe_amd import _lib, resnet_spec, synthetic
from hpe_amd.resnet_spec import CONV_SPECS, ENCODER_PARAM_OFFSETS, ENCODER_STAT_OFFSETS
from oracle import hmr_oracle as O

pytestmark = pytest.mark.gpu
MARGIN = 4.0
FORWARD_BAR = 5e-5  # tests/test_gpu_encoder_train.py: per-layer max error over the layer's largest output
FEATURE_BAR = 2e-5  # the frozen training forward's bar on the features
ULP4 = 2.0 ** -22   # four half-ulps of float32
PACKINGS = _lib.ENCODER_PACKINGS
PLANS = {"A": {}, "B": {"f32_split": 15, "wino_f4": 15}, "C": {"f32_split": 0, "wino_f4": 0, "dual_gemm": 0}}  # tests/test_gpu_encoder_repack.py


def make_params():
    """synthetic.py's encoder with gamma in [0.5, 1.5] on every layer, non-trivial mean / var / bias"""
    p = synthetic.make_encoder_params(seed=7)
    g = np.random.default_rng(11)
    for s in CONV_SPECS:
        p[s.bn_name + "/gamma"] = g.uniform(0.5, 1.5, s.cout).astype(np.float32)
    return p


def make_engine(params, max_batch=4, reserve=3, batch_norm=True, **kw):
    e = hpe_amd.HpeEngine(device=0, max_batch=max_batch, **kw)
    e.load_encoder(params)
    e.finalize()
    if reserve:
        e.reserve_encoder_train(reserve, batch_norm=batch_norm)
    return e


@pytest.fixture(scope="module")
def params():
    return make_params()


@pytest.fixture(scope="module")
def engine(params):
    e = make_engine(params)
    yield e
    e.close()


def _layer_inputs(s, idx, B):
    g = torch.Generator().manual_seed(1000 * B + idx)
    x = torch.randn(B, s.hin, s.hin, s.cin, generator=g)
    res = torch.randn(B, s.hout, s.hout, s.cout, generator=g) if s.name.endswith("2c") else None
    dy = torch.randn(B, s.hout, s.hout, s.cout, generator=g)
    return x, res, dy


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("idx", range(len(CONV_SPECS)))
def test_layer_forward(engine, params, idx, B):
    s = CONV_SPECS[idx]
    x, res, _ = _layer_inputs(s, idx, B)
    relu = not s.name.endswith("branch1")
    y, z, st = engine.debug_conv_batchnorm(idx, x.cuda(), res.cuda() if res is not None else None, relu=relu)
    torch.cuda.synchronize()
    y, z, st = y.cpu(), z.cpu(), st.cpu()
    lt = R.layer_tensors(params, s)
    lt32 = R.layer_tensors(params, s, torch.float32)
    # the raw output against the float64 convolution
    z64 = RB.layer_raw(s, x.double(), lt)
    ez = float((z.double() - z64).abs().max() / z64.abs().max())
    # the statistics against float64 statistics of the GPU's own z
    mu64, var64 = RB.batch_stats(z.double())
    mu, var = st[:s.cout].double(), st[s.cout:].double()
    emu = float(((mu - mu64).abs() / torch.maximum(mu64.abs(), var64.sqrt())).max())
    evar = float(((var - var64).abs() / var64).max())
    # the apply against the float64 apply on that z and those statistics
    r64 = res.double() if res is not None else None
    ref = RB.layer_apply(z.double(), mu64, var64, lt[2], lt[3], r64, relu)
    mu32, var32 = RB.batch_stats(z)
    f32 = RB.layer_apply(z, mu32, var32, lt32[2], lt32[3], res, relu)
    ey, bar = R.rel(y, ref), MARGIN * R.rel(f32, ref)
    print("layer %2d %-16s B=%d z %.3g (bar %.3g)  mu %.3g  var %.3g (bar %.3g)  y %.3g (bar %.3g)" % (idx, s.name, B, ez, FORWARD_BAR, emu, evar, ULP4, ey, bar))
    assert ez <= FORWARD_BAR, (s.name, ez)
    assert emu <= ULP4 and evar <= ULP4, (s.name, emu, evar)
    assert ey < bar, (s.name, ey, bar)
    if s.hout >= 56:  # more than one slice of pixels: the finish sums partials
        assert engine.lib.hpe_debug_encoder_bn_slices(idx, B) > 1


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("idx", range(len(CONV_SPECS)))
def test_layer_backward(engine, params, idx, B):
    s = CONV_SPECS[idx]
    x, res, dy = _layer_inputs(s, idx, B)
    y, z, _ = engine.debug_conv_batchnorm(idx, x.cuda(), res.cuda() if res is not None else None, relu=True)
    cases = [("gated", y)] + ([("ungated", None)] if s.name.endswith("branch1") else [])  # as the network runs a projection shortcut
    for tag, yy in cases:
        dx, gl = engine.debug_conv_backward_batchnorm(idx, x.cuda(), z, yy, dy.cuda())
        torch.cuda.synchronize()
        # the SAME fp32 z and y drive the restatement: the gates and xhat agree by construction
        zc, yc = z.cpu(), (yy.cpu() if yy is not None else None)
        ref = RB.layer_backward(s, x.double(), zc.double(), yc, dy.double(), R.layer_tensors(params, s), gated=yy is not None)
        f32 = RB.layer_backward(s, x, zc, yc, dy, R.layer_tensors(params, s, torch.float32), gated=yy is not None)
        got = R.split_layer_grad(s, gl.cpu())
        assert float(got.pop("db").abs().max()) == 0.0
        if idx != 0:
            got["dx"] = dx.cpu()
        for k, v in got.items():
            e, bar = R.rel(v, ref[k]), MARGIN * R.rel(f32[k], ref[k])
            print("layer %2d %-16s B=%d %-7s %-6s gpu %.3g  bar %.3g" % (idx, s.name, B, tag, k, e, bar))
            assert e < bar, (s.name, tag, k, e, bar)


@pytest.fixture(scope="module")
def whole(engine, params):
    """B = 2: one batch-mode forward and backward, the stashes they left, and the float64 / float32 restatements"""
    B = 2
    img = synthetic.make_images(B, seed=31)
    gf = torch.randn(B, 2048, generator=torch.Generator().manual_seed(3))
    imgs = torch.from_numpy(img).cuda()
    feat = engine.encoder_forward_train(imgs, bn="batch").cpu()
    grad = engine.encoder_backward(imgs, gf.cuda(), bn="batch").cpu()
    stash = [engine.encoder_stash(i).cpu() for i in range(len(CONV_SPECS))]
    zstash = [engine.encoder_stash_raw(i).cpu() for i in range(len(CONV_SPECS))]
    pooled = engine.encoder_stash(-1).cpu()
    bstats = engine.encoder_batch_stats().cpu()
    win = R.maxpool_winners(stash[0])
    ti = torch.from_numpy(img)
    ref = RB.network_backward(params, ti, zstash, stash, pooled, win, gf)
    f32 = RB.network_backward(params, ti, zstash, stash, pooled, win, gf, dtype=torch.float32)
    return dict(img=img, feat=feat, grad=grad, stash=stash, zstash=zstash, pooled=pooled, bstats=bstats, ref=ref, f32=f32, gf=gf)


def test_forward_features(whole, params):
    """The whole forward against the float64 restatement.  The frozen forward's bar of 2e-5 on the features is valid only for inputs on
    which the float32 restatement itself stays below a quarter of it.  With gamma in [0.5, 1.5] on every layer it does not, at any image
    seed (3.1e-5 to 3.5e-5 at seeds 31, 32, 33): with unit gain everywhere and every layer normalised again by its own batch, rounding
    error grows by about 1.1 x per layer through the 53 layers.  Another seed, which is what the issue asks for in that case, does not
    help, so this test departs from it: the 2e-5 bar is held on synthetic.py's own encoder (small gammas on the last BatchNorm of every
    bottleneck, the encoder of the trainer tests), where the float32 restatement is at 2.0e-6 to 2.5e-6 (it depends on the host's
    float32 matrix product; asserted below a quarter of the bar here), and the [0.5, 1.5] context is held to the project's rule,
    4 x the float32 restatement's error."""
    ti = torch.from_numpy(whole["img"])
    ref, _ = RB.network_forward(params, ti)
    f32, _ = RB.network_forward(params, ti, torch.float32)
    err = lambda a: float((a.double() - ref).abs().max() / ref.abs().max())  # noqa: E731
    e, bar = err(whole["feat"]), MARGIN * err(f32)
    print("batch-mode features, gamma in [0.5, 1.5]: gpu %.3g, bar %.3g (4 x the float32 restatement)" % (e, bar))
    assert e < bar
    own = synthetic.make_encoder_params()
    ref, _ = RB.network_forward(own, ti)
    f32, _ = RB.network_forward(own, ti, torch.float32)
    budget = err(f32)
    eng = make_engine(own, max_batch=2, reserve=2)
    try:
        e = err(eng.encoder_forward_train(ti.cuda(), bn="batch").cpu())
    finally:
        eng.close()
    print("batch-mode features, synthetic.py's own encoder: gpu %.3g, float32 restatement %.3g, bar %.3g" % (e, budget, FEATURE_BAR))
    assert budget < FEATURE_BAR / 4  # the bar is valid for these inputs
    assert e < FEATURE_BAR
    # the batch statistics of the call: those of its own stashed z, layer by layer
    for s, (om, ov), z in zip(CONV_SPECS, ENCODER_STAT_OFFSETS, whole["zstash"]):
        mu64, var64 = RB.batch_stats(z.double())
        mu, var = whole["bstats"][om:om + s.cout].double(), whole["bstats"][ov:ov + s.cout].double()
        assert bool(((mu - mu64).abs() <= ULP4 * torch.maximum(mu64.abs(), var64.sqrt())).all()), s.name
        assert bool(((var - var64).abs() <= ULP4 * var64).all()), s.name


def test_network_backward(whole):
    worst = (0.0, None)
    for i, (s, off) in enumerate(zip(CONV_SPECS, ENCODER_PARAM_OFFSETS)):
        n = s.kh * s.kw * s.cin * s.cout + 3 * s.cout
        got, ref, f32 = (R.split_layer_grad(s, whole[k][off[0]:off[0] + n]) for k in ("grad", "ref", "f32"))
        assert float(got.pop("db").abs().max()) == 0.0
        for k in got:
            e, bar = R.rel(got[k], ref[k]), MARGIN * R.rel(f32[k], ref[k])
            print("net layer %2d %-16s %-6s gpu %.3g  bar %.3g" % (i, s.name, k, e, bar))
            if e / bar > worst[0]:
                worst = (e / bar, (s.name, k, e, bar))
            assert e < bar, (s.name, k, e, bar)
    print("worst layer against its bar:", worst)


def test_deterministic_and_capturable(engine, whole):
    imgs = torch.from_numpy(whole["img"]).cuda()
    gf = whole["gf"].cuda()
    a = engine.encoder_backward(imgs, gf, bn="batch")
    engine.encoder_backward(imgs[:1].contiguous(), gf[:1].contiguous() * 2, bn="batch")  # another call in between
    b = engine.encoder_backward(imgs, gf, bn="batch")
    assert torch.equal(a, b) and torch.equal(a.cpu(), whole["grad"])
    out = torch.empty_like(a)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            _lib.check(engine.lib.hpe_encoder_backward_batchnorm(engine._h, imgs.data_ptr(), 2, gf.data_ptr(), out.data_ptr(), engine._stream()))
        for _ in range(2):
            out.zero_()
            graph.replay()
            side.synchronize()
            assert torch.equal(out, a)
    torch.cuda.current_stream().wait_stream(side)


def test_autograd_function(engine, whole):
    """encoder_features(bn="batch"): one .backward() fills the flat tensor's .grad with the bits of encoder_backward(bn="batch")"""
    imgs = torch.from_numpy(whole["img"]).cuda()
    p = engine.encoder_params().requires_grad_(True)
    f = hpe_amd.encoder_features(engine, imgs, p, bn="batch")
    assert torch.equal(f.cpu(), whole["feat"])
    (f * whole["gf"].cuda()).sum().backward()
    assert torch.equal(p.grad.cpu(), whole["grad"])


def test_every_batch_below_the_reserve(params):
    e = make_engine(params, max_batch=17, reserve=17)
    try:
        g = torch.Generator().manual_seed(8)
        img = torch.from_numpy(synthetic.make_images(17, seed=2)).cuda()
        gf = torch.randn(17, 2048, generator=g).cuda()
        for B in range(1, 18):
            grad = e.encoder_backward(img[:B].contiguous(), gf[:B].contiguous(), bn="batch")
            assert bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 0.0, B
    finally:
        e.close()


def test_modes_interleave(params):
    """Both modes run one walk over one set of work buffers: calls of the two modes at different batches, interleaved on one context,
    give the bits of the same call on a context that has only ever run that mode at that batch"""
    img = torch.from_numpy(synthetic.make_images(2, seed=5)).cuda()
    gf = torch.randn(2, 2048, generator=torch.Generator().manual_seed(6)).cuda()
    calls = [("backward", "batch", 2), ("backward", "frozen", 1), ("backward", "batch", 2), ("backward", "frozen", 2), ("forward", "batch", 1),
             ("forward", "frozen", 2)]

    def run(e, what, bn, B):
        if what == "forward":
            return e.encoder_forward_train(img[:B].contiguous(), bn=bn)
        return e.encoder_backward(img[:B].contiguous(), gf[:B].contiguous(), bn=bn)

    want = {}
    for bn, B in sorted({(bn, B) for _, bn, B in calls}):
        e = make_engine(params, max_batch=2, reserve=B, batch_norm=bn == "batch")
        try:
            want.update({c: run(e, *c) for c in calls if c[1:] == (bn, B)})
        finally:
            e.close()
    e = make_engine(params, max_batch=2, reserve=2)
    try:
        for c in calls:
            assert torch.equal(run(e, *c), want[c]), c
        with pytest.raises(_lib.HpeError, match="refilled the stash"):  # the frozen forward of B = 2, since the batch forward of B = 1
            e.encoder_stash_raw(1)
    finally:
        e.close()


def test_refusals(engine, params):
    lib, h = engine.lib, engine._h
    img = torch.zeros(4, 224, 224, 3, device="cuda")
    gf = torch.zeros(4, 2048, device="cuda")
    out = torch.zeros(resnet_spec.ENCODER_PARAM_FLOATS, device="cuda")
    stats = torch.zeros(resnet_spec.ENCODER_STAT_FLOATS, device="cuda")
    st = engine._stream()
    i, g, o, t = img.data_ptr(), gf.data_ptr(), out.data_ptr(), stats.data_ptr()
    assert lib.hpe_encoder_backward_batchnorm(h, None, 1, g, o, st) == 1
    assert lib.hpe_encoder_backward_batchnorm(h, i, 1, None, o, st) == 1
    assert lib.hpe_encoder_backward_batchnorm(h, i, 1, g, None, st) == 1
    assert lib.hpe_encoder_backward_batchnorm(h, i, 0, g, o, st) == 1
    assert lib.hpe_encoder_backward_batchnorm(h, i, 4, g, o, st) == 1  # reserved for 3
    assert lib.hpe_encoder_forward_batchnorm(h, i, 4, g, st) == 1
    assert lib.hpe_encoder_forward_batchnorm(h, None, 1, g, st) == 1 and lib.hpe_encoder_forward_batchnorm(h, i, 1, None, st) == 1
    assert lib.hpe_encoder_get_stats(h, None, st) == 1 and lib.hpe_encoder_set_stats_dev(h, None, st) == 1
    assert lib.hpe_encoder_update_stats(h, None, 0.9, 1, st) == 1
    for m in (-0.01, 1.01, float("nan")):
        assert lib.hpe_encoder_update_stats(h, t, m, 1, st) == 1
    assert lib.hpe_debug_conv_batchnorm(h, 53, i, 1, None, 1, o, o, t, st) == 1 and lib.hpe_debug_conv_batchnorm(h, -1, i, 1, None, 1, o, o, t, st) == 1
    assert lib.hpe_debug_conv_batchnorm(h, 1, i, 4, None, 1, o, o, t, st) == 1 and lib.hpe_debug_conv_batchnorm(h, 1, i, 1, None, 1, o, None, t, st) == 1
    assert lib.hpe_debug_conv_backward_batchnorm(h, 0, i, i, i, i, 1, o, o, st) == 1  # conv1 has no data gradient
    assert lib.hpe_debug_conv_backward_batchnorm(h, 1, i, None, i, i, 1, None, o, st) == 1
    assert lib.hpe_debug_encoder_stash_raw(h, -1, o, st) == 1 and lib.hpe_debug_encoder_stash_raw(h, 53, o, st) == 1
    assert lib.hpe_debug_encoder_batch_stats(h, None, st) == 1
    with pytest.raises(ValueError):
        engine.encoder_forward_train(img[:1], bn="moving")
    with pytest.raises(ValueError):
        engine.set_encoder_stats_dev(stats[:-1])
    frozen = make_engine(params, max_batch=2, reserve=1, batch_norm=False)  # the ordinary reserve only
    try:
        f = frozen._h
        assert lib.hpe_encoder_backward_batchnorm(f, i, 1, g, o, st) == 3 and lib.hpe_encoder_forward_batchnorm(f, i, 1, g, st) == 3
        assert lib.hpe_encoder_get_stats(f, t, st) == 3 and lib.hpe_encoder_set_stats_dev(f, t, st) == 3
        assert lib.hpe_encoder_update_stats(f, t, 0.9, 1, st) == 3 and lib.hpe_debug_encoder_batch_stats(f, t, st) == 3
        assert lib.hpe_encoder_train_reserve_batchnorm(f, 3) == 1  # above max_batch
        assert lib.hpe_encoder_train_reserve_batchnorm(f, 2) == 3  # the ordinary reserve was made for 1
        frozen.reserve_encoder_train(1, batch_norm=True)           # ... and beside it for 1
        assert lib.hpe_encoder_update_stats(f, t, 0.9, 1, st) == 3  # no batch-mode forward yet
        assert lib.hpe_debug_encoder_batch_stats(f, t, st) == 3 and lib.hpe_debug_encoder_stash_raw(f, 1, o, st) == 3
        assert lib.hpe_encoder_get_stats(f, t, st) == 0
    finally:
        frozen.close()
    fresh = make_engine(params, max_batch=2, reserve=0)
    try:
        assert lib.hpe_encoder_backward_batchnorm(fresh._h, i, 1, g, o, st) == 3  # before any reserve
        fresh.reserve_encoder_train(2, batch_norm=True)  # does the ordinary reserve too
        assert fresh.encoder_params().shape == (resnet_spec.ENCODER_PARAM_FLOATS,)
    finally:
        fresh.close()
    bf = make_engine(params, max_batch=2, reserve=0, encoder_dtype="bf16")
    try:
        assert lib.hpe_encoder_train_reserve_batchnorm(bf._h, 1) == 3
        assert lib.hpe_encoder_backward_batchnorm(bf._h, i, 1, g, o, st) == 3 and lib.hpe_encoder_set_stats_dev(bf._h, t, st) == 3
    finally:
        bf.close()


def test_update_stats(engine, params):
    """update_encoder_stats against the float64 formula on the batch statistics of a B = 3 forward, each layer's own M"""
    img = torch.from_numpy(synthetic.make_images(3, seed=17)).cuda()
    engine.encoder_forward_train(img, bn="batch")
    stats0 = engine.encoder_stats()
    assert np.array_equal(stats0.cpu().numpy(), resnet_spec.params_to_stats(params))
    batch = engine.encoder_batch_stats().cpu().double()
    for unbiased in (False, True):
        t = stats0.clone()
        assert engine.update_encoder_stats(t, momentum=0.9, unbiased=unbiased) is t
        ref = RB.momentum_update(stats0.cpu().double(), batch, 3, 0.9, unbiased)
        e = float(((t.cpu().double() - ref).abs() / ref.abs()).max())
        print("update_encoder_stats unbiased=%s: worst relative error %.3g (bar %.3g)" % (unbiased, e, ULP4))
        assert e <= ULP4
        assert not torch.equal(t, stats0)
    assert torch.equal(engine.encoder_stats(), stats0)  # nothing was installed


def snapshot(e):
    """{(layer, packing name): uint8 CUDA tensor} of every packing the context holds"""
    out = {}
    for i in range(len(CONV_SPECS)):
        for w, name in enumerate(PACKINGS):
            t = e.encoder_packing(i, w)
            if t is not None:
                out[(i, name)] = t
    return out


def assert_same_packings(a, b):
    assert set(a) == set(b), sorted(set(a) ^ set(b))
    bad = [k for k in a if a[k].shape != b[k].shape or not torch.equal(a[k], b[k])]
    assert not bad, bad


def check_batch_forward(e, params, img):
    """after a batch-mode forward: every layer's stashed z against the float64 convolution of its stashed input (the per-layer forward
    bar), the batch statistics against float64 statistics of that z, and y against the float64 apply (4 x the float32 restatement)"""
    n = len(CONV_SPECS)
    st, zs = [e.encoder_stash(i).cpu() for i in range(n)], [e.encoder_stash_raw(i).cpu() for i in range(n)]
    pooled, bstats = e.encoder_stash(-1).cpu(), e.encoder_batch_stats().cpu()
    bl = R.blocks()
    inputs, resid = {0: img}, {}
    for k, (i2a, i2b, i2c, i1) in enumerate(bl):
        xin = pooled if k == 0 else st[bl[k - 1][2]]
        inputs[i2a], inputs[i2b], inputs[i2c] = xin, st[i2a], st[i2b]
        resid[i2c] = xin if i1 is None else st[i1]
        if i1 is not None:
            inputs[i1] = xin
    for i, s in enumerate(CONV_SPECS):
        lt, lt32 = R.layer_tensors(params, s), R.layer_tensors(params, s, torch.float32)
        z64 = RB.layer_raw(s, inputs[i].double(), lt)
        assert float((zs[i].double() - z64).abs().max()) <= FORWARD_BAR * float(z64.abs().max()), s.name
        mu64, var64 = RB.batch_stats(zs[i].double())
        om, ov = ENCODER_STAT_OFFSETS[i]
        mu, var = bstats[om:om + s.cout].double(), bstats[ov:ov + s.cout].double()
        assert bool(((mu - mu64).abs() <= ULP4 * torch.maximum(mu64.abs(), var64.sqrt())).all()), s.name
        assert bool(((var - var64).abs() <= ULP4 * var64).all()), s.name
        relu, res = not s.name.endswith("branch1"), resid.get(i)
        ref = RB.layer_apply(zs[i].double(), mu64, var64, lt[2], lt[3], res.double() if res is not None else None, relu)
        f32 = RB.layer_apply(zs[i], *RB.batch_stats(zs[i]), lt32[2], lt32[3], res, relu)
        assert R.rel(st[i], ref) < MARGIN * R.rel(f32, ref), s.name


@pytest.mark.parametrize("plan", sorted(PLANS))
def test_install_stats(params, plan):
    """set_encoder_params_dev(q) and set_encoder_stats_dev(t) in both orders against a fresh context loaded with (q, t)"""
    p = torch.from_numpy(resnet_spec.params_to_flat(params))
    d = torch.randn(p.shape, generator=torch.Generator().manual_seed(2))
    q = p + d * (1e-2 * float(p.norm()) / float(d.norm()))
    img = torch.from_numpy(synthetic.make_images(2, seed=9)).cuda()
    gf = torch.randn(2, 2048, generator=torch.Generator().manual_seed(3)).cuda()
    mk = lambda prm, bn: make_engine(prm, max_batch=2, reserve=2, batch_norm=bn, **PLANS[plan])  # noqa: E731
    e, e2 = mk(params, True), mk(params, True)
    fresh = None
    try:
        # t: the loaded statistics moved by one update -- variances stay positive
        e.encoder_forward_train(img, bn="batch")
        check_batch_forward(e, params, img.cpu())  # the unit scale and the bias as shift through this plan's routes
        t = e.update_encoder_stats(e.encoder_stats(), momentum=0.9, unbiased=True)
        assert float(t[resnet_spec.ENCODER_STAT_CHANNELS:].min()) > 0.0
        fresh = mk(resnet_spec.flat_to_params(q, resnet_spec.stats_to_params(t)), False)
        before = snapshot(e)
        e.set_encoder_params_dev(q.cuda())
        e.set_encoder_stats_dev(t)
        e2.set_encoder_stats_dev(t)
        e2.set_encoder_params_dev(q.cuda())
        ref, got = snapshot(fresh), snapshot(e)
        assert_same_packings(got, ref)
        assert_same_packings(snapshot(e2), ref)
        moved = {n for (i, n) in got if not torch.equal(got[(i, n)], before[(i, n)])}
        assert {"scale", "shift"} <= moved
        assert torch.equal(e.encoder_stats(), t) and torch.equal(e2.encoder_stats(), t)
        run = lambda x: (x.encoder(img), x.encoder_forward_train(img), x.encoder_backward(img, gf))  # noqa: E731
        for a, b, c in zip(run(e), run(fresh), run(e2)):
            assert torch.equal(a, b) and torch.equal(c, b)
        e.set_encoder_params(q)  # the host path folds the installed statistics, not the loaded ones
        assert_same_packings(snapshot(e), ref)
        assert torch.equal(e.encoder_stats(), t)
    finally:
        for x in (e, e2, fresh):
            if x is not None:
                x.close()


def test_trainer():
    """GeneratorTrainer(train_encoder=True, encoder_bn="batch") on the fixed batch of 4 and fixed masks of
    tests/test_gpu_encoder_train.py::test_trainer (synthetic.py's own encoder, for the reason given there)."""
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
    for kw in ({}, {"encoder_bn": "frozen"}):
        e = build()
        try:
            e.reserve_encoder_train(4)
            tr = hpe_amd.GeneratorTrainer(e, dropout=0.5, generator=torch.Generator(device="cuda").manual_seed(1), train_encoder=True, **kw)
            assert tr.encoder_stats is None
            masks = tr.draw_masks(4)
            r = [tr.step(img, kp, use_critic=False, drop=masks) for _ in range(2)]
            outs.append((r[-1]["kpr_losses"][-1].cpu(), r[-1]["pred_keypoints"].cpu(), r[-1]["grad_features"].cpu(), tr.params.detach().cpu(),
                         tr.encoder_params.detach().cpu()))
        finally:
            e.close()
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    e = build()
    try:
        e.reserve_encoder_train(4, batch_norm=True)
        tr = hpe_amd.GeneratorTrainer(e, dropout=0.5, generator=torch.Generator(device="cuda").manual_seed(1), train_encoder=True, encoder_bn="batch")
        masks = tr.draw_masks(4)
        p0, s0 = tr.encoder_params.detach().clone(), tr.encoder_stats.clone()
        assert np.array_equal(s0.cpu().numpy(), resnet_spec.params_to_stats(params))
        losses = [float(tr.step(img, kp, use_critic=False, drop=masks)["kpr_losses"][-1])]
        # after step one: the momentum formula (Keras' 0.99, unbiased) on that step's batch statistics
        ref = RB.momentum_update(s0.cpu().double(), e.encoder_batch_stats().cpu().double(), 4, 0.99, True)
        assert float(((tr.encoder_stats.cpu().double() - ref).abs() / ref.abs()).max()) <= ULP4
        losses += [float(tr.step(img, kp, use_critic=False, drop=masks)["kpr_losses"][-1]) for _ in range(4)]
        print("60 * kp loss over 5 steps with the encoder in the update, batch statistics:", losses)
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
