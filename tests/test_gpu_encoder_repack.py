"""hpe_encoder_set_params_dev on the GPU: after the device update every packing the context holds, and every consumer's output, equals bit
for bit that of a fresh context that loaded the same values (the host packers of hpe_finalize are the reference).  Whole ResNet-50 at
max_batch = 2: the network is the smallest shape there is."""
import numpy as np
import pytest
import torch

import hpe_amd
from hpe_amd import _lib, resnet_spec, synthetic
from hpe_amd.resnet_spec import CONV_SPECS
from oracle import hmr_oracle as O

pytestmark = pytest.mark.gpu
PACKINGS = _lib.ENCODER_PACKINGS
PLANS = {"A": {}, "B": {"f32_split": 15, "wino_f4": 15}, "C": {"f32_split": 0, "wino_f4": 0, "dual_gemm": 0}}
# the library's defaults (hpe_plan.hip): stages 3-5 split, F(4x4) on the 7 / 14 / 28 maps, dual-source conv blocks
DEFAULTS = {"f32_split": 14, "wino_f4": 7, "dual_gemm": 1}


def make_params():
    """synthetic.py's encoder with gamma in [0.5, 1.5] on every layer, non-trivial mean / var / bias"""
    p = synthetic.make_encoder_params(seed=7)
    g = np.random.default_rng(11)
    for s in CONV_SPECS:
        p[s.bn_name + "/gamma"] = g.uniform(0.5, 1.5, s.cout).astype(np.float32)
    return p


def make_engine(params, reserve=1, **kw):
    e = hpe_amd.HpeEngine(device=0, max_batch=2, **kw)
    e.load_encoder(params)
    e.finalize()
    if reserve:
        e.reserve_encoder_train(reserve)
    return e


@pytest.fixture(scope="module")
def params():
    return make_params()


@pytest.fixture(scope="module")
def flats(params):
    """p: the loaded parameters; q: p perturbed by 1e-2 relative (seeded), as test_update does"""
    p = torch.from_numpy(resnet_spec.params_to_flat(params))
    d = torch.randn(p.shape, generator=torch.Generator().manual_seed(2))
    q = p + d * (1e-2 * float(p.norm()) / float(d.norm()))
    return p, q


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


def stage_bit(hout):
    return 1 if hout >= 56 else 2 if hout >= 28 else 4 if hout >= 14 else 8


def f4_bit(hin):
    return 1 if hin <= 7 else 2 if hin <= 14 else 4 if hin <= 28 else 8


def expected_forms(plan):
    """the (layer, name) pairs a reserved fp32 context of this plan must hold, from the layer table and the plan alone"""
    o = dict(DEFAULTS, **plan)
    want = set()
    for i, s in enumerate(CONV_SPECS):
        want |= {(i, "w"), (i, "scale"), (i, "shift"), (i, "flat")}
        if i == 0:
            want.add((i, "stem_w"))
            continue
        want.add((i, "dxw"))
        if s.kh == 1 and o["f32_split"] & stage_bit(s.hout):
            want.add((i, "w_split"))
        if s.kh == 3:
            want.add((i, "wino_u"))  # cin >= 128, or the fused path of the 56 / 28 maps
            if o["wino_f4"] & f4_bit(s.hin):
                want.add((i, "wino4_u"))
        if o["dual_gemm"] and s.name.endswith("a_branch2c"):
            want |= {(i, "w_dual"), (i, "shift_dual")}
            if o["f32_split"] & stage_bit(s.hout):
                want.add((i, "w_dual_split"))
    return want


@pytest.mark.parametrize("plan", sorted(PLANS))
def test_every_packing(params, flats, plan):
    p, q = flats
    e = make_engine(params, **PLANS[plan])
    fresh = make_engine(resnet_spec.flat_to_params(q, params), **PLANS[plan])
    try:
        before = snapshot(e)
        e.set_encoder_params_dev(q.cuda())
        got, ref = snapshot(e), snapshot(fresh)
        assert set(ref) == expected_forms(PLANS[plan]), sorted(set(ref) ^ expected_forms(PLANS[plan]))
        names = {n for _, n in ref}
        if plan == "B":
            assert all((i, "w_split") in ref for i, s in enumerate(CONV_SPECS) if i and s.kh == 1)
        if plan == "C":
            assert not names & {"w_split", "wino4_u", "w_dual", "w_dual_split", "shift_dual"}
        if plan == "A":
            assert {s.hin for (i, n) in ref if n == "wino4_u" for s in [CONV_SPECS[i]]} == {7, 14, 28}
        assert_same_packings(got, ref)
        same = [k for k in got if torch.equal(got[k], before[k])]
        assert not same, same  # every buffer really was rewritten
        for i in range(len(CONV_SPECS)):
            for w in range(len(PACKINGS)):
                assert e.lib.hpe_debug_encoder_packing_bytes(e._h, i, w) == fresh.lib.hpe_debug_encoder_packing_bytes(fresh._h, i, w)
    finally:
        e.close()
        fresh.close()


def test_consumers(params, flats):
    p, q = flats
    img = torch.from_numpy(synthetic.make_images(2, seed=9)).cuda()
    gf = torch.randn(2, 2048, generator=torch.Generator().manual_seed(3)).cuda()
    e = make_engine(params, reserve=2)
    fresh = make_engine(resnet_spec.flat_to_params(q, params), reserve=2)
    try:
        f0 = e.encoder(img)
        run = lambda x: (x.encoder(img), x.encoder_forward_train(img), x.encoder_backward(img, gf))  # noqa: E731
        e.set_encoder_params_dev(q.cuda())
        assert torch.equal(e.encoder_params().cpu(), q)
        dev = run(e)
        ref = run(fresh)
        e.set_encoder_params(q)
        host = run(e)
        for a, b, c in zip(dev, ref, host):
            assert torch.equal(a, b) and torch.equal(a, c)
        moved = float((dev[0] - f0).abs().max() / f0.abs().max())
        print("features moved by %.3g" % moved)
        assert moved > 2e-5  # the forward bar on features
    finally:
        e.close()
        fresh.close()


def test_back_and_forth(params, flats):
    p, q = flats
    e = make_engine(params)
    untouched = make_engine(params)
    try:
        e.set_encoder_params_dev(q.cuda())
        once = snapshot(e)
        e.set_encoder_params_dev(q.cuda())
        assert_same_packings(snapshot(e), once)  # idempotent
        e.set_encoder_params(p)
        e.set_encoder_params_dev(p.cuda())
        assert_same_packings(snapshot(e), snapshot(untouched))
    finally:
        e.close()
        untouched.close()


def test_capture(params, flats):
    p, q = flats
    img = torch.from_numpy(synthetic.make_images(2, seed=9)).cuda()
    e = make_engine(params, reserve=2)
    try:
        eager = {}
        for k, v in (("q", q), ("p", p)):
            e.set_encoder_params_dev(v.cuda())
            eager[k] = e.encoder_forward_train(img).clone()
        assert not torch.equal(eager["p"], eager["q"])
        static = torch.empty_like(p, device="cuda")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            static.copy_(p)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                e.set_encoder_params_dev(static)
                out = e.encoder_forward_train(img)
            for k, v in (("p", p), ("q", q)):
                static.copy_(v)
                graph.replay()
                side.synchronize()
                assert torch.equal(out, eager[k]), k
        torch.cuda.current_stream().wait_stream(side)
        assert torch.equal(e.encoder_params().cpu(), q)
    finally:
        e.close()


def test_refusals(params):
    flat = torch.zeros(resnet_spec.ENCODER_PARAM_FLOATS, device="cuda")
    buf = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    e = make_engine(params, reserve=0)
    try:
        lib, h, st = e.lib, e._h, e._stream()
        assert lib.hpe_encoder_set_params_dev(h, flat.data_ptr(), st) == 3  # before the reserve
        assert lib.hpe_debug_encoder_packing_bytes(h, 1, PACKINGS.index("dxw")) == 0
        e.reserve_encoder_train(1)
        assert lib.hpe_encoder_set_params_dev(h, None, st) == 1
        for idx, which in ((-1, 0), (len(CONV_SPECS), 0), (0, -1), (0, len(PACKINGS))):
            assert lib.hpe_debug_encoder_packing(h, idx, which, buf.data_ptr(), st) == 1
            assert lib.hpe_debug_encoder_packing_bytes(h, idx, which) == 0
        assert lib.hpe_debug_encoder_packing(h, 0, 0, None, st) == 1
        assert lib.hpe_debug_encoder_packing(h, 1, PACKINGS.index("stem_w"), buf.data_ptr(), st) == 3  # a form the layer does not have
        with pytest.raises(ValueError):
            e.set_encoder_params_dev(flat[:-1])
        with pytest.raises(ValueError):
            e.set_encoder_params_dev(flat.cpu())
    finally:
        e.close()
    bf = make_engine(params, reserve=0, encoder_dtype="bf16")
    try:
        assert bf.lib.hpe_encoder_set_params_dev(bf._h, flat.data_ptr(), bf._stream()) == 3
        assert bf.lib.hpe_debug_encoder_packing_bytes(bf._h, 0, 0) == 0
    finally:
        bf.close()


def test_trainer():
    """two steps of GeneratorTrainer(train_encoder=True) on the fixed batch and masks of test_gpu_encoder_train.py::test_trainer: the engine
    holds the optimiser's tensor exactly, and its inference encoder is that of a fresh context built from those parameters"""
    params = synthetic.make_encoder_params()
    e = hpe_amd.HpeEngine(device=0, max_batch=4)
    e.load_smpl(synthetic.make_smpl_model())
    e.load_encoder(params)
    e.load_regressor(synthetic.make_regressor_params(variant="bounded"))
    e.load_mean_theta(O.load_mean_param(synthetic.make_mean_params()))
    e.finalize()
    img = torch.from_numpy(synthetic.make_images(4, seed=13)).cuda()
    g = torch.Generator().manual_seed(4)
    kp = torch.cat([torch.rand(4, 19, 2, generator=g) * 1.2 - 0.6, torch.ones(4, 19, 1)], 2).cuda()
    try:
        e.reserve_encoder_train(4)
        tr = hpe_amd.GeneratorTrainer(e, dropout=0.5, generator=torch.Generator(device="cuda").manual_seed(1), train_encoder=True)
        masks = tr.draw_masks(4)
        p0 = tr.encoder_params.detach().clone()
        for _ in range(2):
            tr.step(img, kp, use_critic=False, drop=masks)
        now = tr.encoder_params.detach()
        assert not torch.equal(now, p0) and torch.equal(e.encoder_params(), now)
        feat = e.encoder(img)
        fresh = hpe_amd.HpeEngine(device=0, max_batch=4)
        try:
            fresh.load_encoder(resnet_spec.flat_to_params(now.cpu(), params))
            fresh.finalize()
            assert torch.equal(feat, fresh.encoder(img))
        finally:
            fresh.close()
    finally:
        e.close()
