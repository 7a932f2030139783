"""The fused F(2x2,3x3) Winograd kernel on the bf16 matrix cores (wino_fused_split_kernel), through debug_conv: against float64 on
inputs with 24 binades of dynamic range, and bit for bit against itself across launches, batch positions and a device parameter
update.  Shapes: res2b_branch2b (56x56, C = 64: 2 tile rows of 28 per workgroup, 14 workgroups per image) at B = 1 and 3 (odd
batch); res3b_branch2b (28x28, C = 128: 4 tile rows of 14 per workgroup -- 14 rows per image, so workgroups straddle two images
from B = 3 on and the last one holds tile rows past the batch; two cout blocks) at B = 1, 3 and 37."""
import functools

import numpy as np
import pytest
import torch

import hpe_amd
from hpe_amd import _lib, resnet_spec, synthetic
from oracle import hmr_oracle as O

pytestmark = pytest.mark.gpu
MAXB = 37
BAR = 5e-6
CASES = [("res2b_branch2b", 1), ("res2b_branch2b", 3), ("res3b_branch2b", 1), ("res3b_branch2b", 3), ("res3b_branch2b", 37)]


def make_engine(params, reserve=0):
    e = hpe_amd.HpeEngine(device=0, max_batch=MAXB, wino_f4=0, wino_min_items=0)
    e.load_encoder(params)
    e.finalize()
    if reserve:
        e.reserve_encoder_train(reserve)
    return e


@pytest.fixture(scope="module")
def params():
    return synthetic.make_encoder_params()


@pytest.fixture(scope="module")
def engine(params):
    e = make_engine(params)
    yield e
    e.close()


def rel(a, b):
    a = np.asarray(a, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


@functools.lru_cache(maxsize=None)
def layer_input(name, B):
    """N(0,1) scaled by 2^-12 .. 2^12 per pixel, a third exact zeros, one corner pixel at 50"""
    idx = resnet_spec.CONV_INDEX[name]
    s = resnet_spec.CONV_SPECS[idx]
    g = np.random.Generator(np.random.Philox(8100 + idx + B))
    x = g.normal(0, 1, (B, s.hin, s.hin, s.cin)) * np.exp2(g.integers(-12, 13, (B, s.hin, s.hin, 1)))
    x[g.random(x.shape) < 1 / 3] = 0.0
    x[0, 0, 0, :] = 50.0
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


def bn_fold(p, s, eps=1e-3):
    g, b = p[s.bn_name + "/gamma"].astype(np.float64), p[s.bn_name + "/beta"].astype(np.float64)
    m, v = p[s.bn_name + "/moving_mean"].astype(np.float64), p[s.bn_name + "/moving_variance"].astype(np.float64)
    return g / np.sqrt(v + eps), b - m * g / np.sqrt(v + eps)


_lin = {}


def reference_fp64(params, name, B):
    """conv + folded BN in float64, before the ReLU; computed once per case"""
    if (name, B) not in _lin:
        s = resnet_spec.CONV_SPECS[resnet_spec.CONV_INDEX[name]]
        sc, sh = bn_fold(params, s)
        _lin[(name, B)] = O.conv2d_nhwc(layer_input(name, B).copy(), params[s.name + "/kernel"], params[s.name + "/bias"], 1, 1, dtype=np.float64) * sc + sh
    return _lin[(name, B)]


def run(e, name, x, relu=True):
    idx = resnet_spec.CONV_INDEX[name]
    assert _lib.CONV_KERNELS[e.conv_route(idx, x.shape[0]).kernel] == "wino_fused"
    return e.debug_conv(idx, x, relu=relu).cpu()


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("name,B", CASES)
def test_dynamic_range_against_fp64(engine, params, name, B, relu):
    lin = reference_fp64(params, name, B)
    ref = np.maximum(lin, 0) if relu else lin
    y = run(engine, name, torch.tensor(layer_input(name, B)).cuda(), relu).numpy()
    assert y.shape == ref.shape
    err = rel(y, ref)
    print("%s B=%d relu=%d: %.3g against fp64 (bar %.3g)" % (name, B, relu, err, BAR))
    assert err < BAR


@pytest.mark.parametrize("name,B", [("res2b_branch2b", 3), ("res3b_branch2b", 3)])
def test_repeatable_and_batch_position_does_not_change_a_bit(engine, name, B):
    x = torch.tensor(layer_input(name, B)).cuda()
    y = run(engine, name, x)
    assert torch.equal(run(engine, name, x), y)
    for i in range(B):
        assert torch.equal(run(engine, name, x[i:i + 1].contiguous())[0], y[i]), i


def test_parameter_update_on_the_device(params):
    """after set_encoder_params_dev both layers compute what a fresh context built from those values computes (an engine of its own:
    the update must not reach the engine the other tests share)"""
    engine = make_engine(params, reserve=1)
    xs = {name: torch.tensor(layer_input(name, 3)).cuda() for name in ("res2b_branch2b", "res3b_branch2b")}
    p = torch.from_numpy(resnet_spec.params_to_flat(params))
    d = torch.randn(p.shape, generator=torch.Generator().manual_seed(5))
    q = p + d * (1e-2 * float(p.norm()) / float(d.norm()))
    fresh = make_engine(resnet_spec.flat_to_params(q, params))
    try:
        before = {n: run(engine, n, x) for n, x in xs.items()}
        engine.set_encoder_params_dev(q.cuda())
        got = {n: run(engine, n, x) for n, x in xs.items()}
        want = {n: run(fresh, n, x) for n, x in xs.items()}
    finally:
        engine.close()
        fresh.close()
    for n in xs:
        assert torch.equal(got[n], want[n]) and not torch.equal(got[n], before[n]), n
