"""The weight-resident streaming split-bf16 kernel (conv_stream_f32s.hip, HPE_STREAM1X1) on its launches -- form 1, the identity-block
expand layers with K <= 128 that are launches of their own, through debug_conv; form 2, the dual-source launch res2a_branch2c +
res2a_branch1, through debug_dual -- against float64 next to the fp32-MFMA kernel on the same inputs (the bars of test_gpu_f32_split.py),
and bit for bit across grid sizes, launches, batch positions and a device parameter update.

Tiles are 32 rows: res2c_branch2c has 98 and 294 whole tiles at B = 1 and 3; res3b_branch2c has 24.5, 73.5 and 906.5 at B = 1, 3 and 37, so
its last tile is partial."""
import contextlib
import functools
import os

import numpy as np
import pytest
import torch

import hpe_amd
from hpe_amd import resnet_spec, synthetic

pytestmark = pytest.mark.gpu

MAXB = 37
CASES = [("res2c_branch2c", 1), ("res2c_branch2c", 3), ("res3b_branch2c", 1), ("res3b_branch2c", 3), ("res3b_branch2c", 37)]
WALK_CASES = [c for c in CASES if c[1] <= 3] + [("res3b_branch2c", 37), ("res2a_branch2c", 1), ("res2a_branch2c", 3)]
DUAL = "res2a_branch2c"  # + res2a_branch1: 98 and 294 whole tiles at B = 1 and 3
FORCED = {"HPE_STREAM1X1": "3", "HPE_STREAM1X1_MIN_M": "1"}  # both forms of the new kernel on every grid size
OFF = {"HPE_STREAM1X1": "0"}


@contextlib.contextmanager
def environment(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def make_engine(params, env, reserve=0):
    """encoder-only fp32 context of the default plan, finalised under env (the plan is resolved once, there)"""
    with environment(env):
        e = hpe_amd.HpeEngine(device=0, max_batch=MAXB)
        e.load_encoder(params)
        e.finalize()
        if reserve:
            e.reserve_encoder_train(reserve)
        for name in {c[0] for c in CASES}:
            idx = resnet_spec.CONV_INDEX[name]
            on = env.get("HPE_STREAM1X1") == "3"
            assert e.conv_stream1x1(idx, 1) == (3 if on else 0), (name, env)
            assert e.conv_stream1x1(idx, 1, residual=False) == (2 if on else 0)  # without its residual the layer is a plain GEMM
        assert e.conv_stream1x1(resnet_spec.CONV_INDEX[DUAL], 1) == (3 if env.get("HPE_STREAM1X1") == "3" else 0), env
    return e


@pytest.fixture(scope="module")
def params():
    return synthetic.make_encoder_params()


@pytest.fixture(scope="module")
def engines(params):
    made = {"off": make_engine(params, OFF), "on": make_engine(params, FORCED)}
    yield made
    for e in made.values():
        e.close()


@functools.lru_cache(maxsize=None)
def inputs(name, B):
    """the recipe of test_gpu_f32_split.py: N(0,1) rows scaled over 2^-12 .. 2^12, a third exact zeros, an fp32 residual"""
    idx = resnet_spec.CONV_INDEX[name]
    s = resnet_spec.CONV_SPECS[idx]
    g = np.random.Generator(np.random.Philox(9100 + 7 * idx + B))
    x = g.normal(0, 1, (B, s.hin, s.hin, s.cin))
    x *= np.exp2(g.integers(-12, 13, (B, s.hin, s.hin, 1)))
    x[g.random(x.shape) < 0.33] = 0.0
    res = g.normal(0, 1, (B, s.hout, s.hout, s.cout)).astype(np.float32)
    x = x.astype(np.float32)
    x.setflags(write=False)
    res.setflags(write=False)
    return x, res


def bn_fold(p, s, eps=1e-3):
    g, b = p[s.bn_name + "/gamma"].astype(np.float64), p[s.bn_name + "/beta"].astype(np.float64)
    m, v = p[s.bn_name + "/moving_mean"].astype(np.float64), p[s.bn_name + "/moving_variance"].astype(np.float64)
    return g / np.sqrt(v + eps), b - m * g / np.sqrt(v + eps)


_ref = {}


def reference_fp64(params, name, B):
    if (name, B) not in _ref:
        s = resnet_spec.CONV_SPECS[resnet_spec.CONV_INDEX[name]]
        x, res = inputs(name, B)
        y = torch.from_numpy(x.astype(np.float64).reshape(-1, s.cin)) @ torch.from_numpy(params[s.name + "/kernel"].astype(np.float64).reshape(s.cin, s.cout))
        sc, sh = bn_fold(params, s)
        y = (y.numpy() + params[s.name + "/bias"].astype(np.float64)) * sc + sh + res.reshape(-1, s.cout)
        _ref[(name, B)] = np.maximum(y, 0).reshape(res.shape)
    return _ref[(name, B)]


def run(e, name, B, x=None, res=None):
    """the launch of `name` at batch B on the shared inputs (or on x / res): an expand layer with its residual, or the dual-source launch
    of res2a on (t2, block input)"""
    if x is None:
        x, res = (torch.from_numpy(a.copy()).cuda() for a in (dual_inputs(B) if name == DUAL else inputs(name, B)))
    if name == DUAL:
        return e.debug_dual(resnet_spec.CONV_INDEX[name], x, res).cpu()
    return e.debug_conv(resnet_spec.CONV_INDEX[name], x, residual=res, relu=True).cpu()


@functools.lru_cache(maxsize=None)
def dual_inputs(B):
    """t2 (the branch2b output) and the block input, both [B,56,56,64], by the same recipe"""
    g = np.random.Generator(np.random.Philox(9300 + B))
    out = []
    for _ in range(2):
        a = g.normal(0, 1, (B, 56, 56, 64)) * np.exp2(g.integers(-12, 13, (B, 56, 56, 1)))
        a[g.random(a.shape) < 0.33] = 0.0
        a = a.astype(np.float32)
        a.setflags(write=False)
        out.append(a)
    return tuple(out)


def dual_reference_fp64(params, B):
    """relu(bn2c(W2c t2 + b2c) + bn1(W1 x + b1)) as ONE float64 GEMM over the concatenated k axis, the BN scales folded into the weights"""
    if (DUAL, B) not in _ref:
        i2c = resnet_spec.CONV_INDEX[DUAL]
        s2, s1 = resnet_spec.CONV_SPECS[i2c], resnet_spec.CONV_SPECS[i2c + 1]
        assert s1.name == "res2a_branch1" and s1.stride == 1
        t2, x = dual_inputs(B)
        sc2, sh2 = bn_fold(params, s2)
        sc1, sh1 = bn_fold(params, s1)
        W = np.concatenate([params[s2.name + "/kernel"].astype(np.float64).reshape(s2.cin, s2.cout) * sc2,
                            params[s1.name + "/kernel"].astype(np.float64).reshape(s1.cin, s1.cout) * sc1], axis=0)
        A = np.concatenate([t2.astype(np.float64).reshape(-1, s2.cin), x.astype(np.float64).reshape(-1, s1.cin)], axis=1)
        y = (torch.from_numpy(A) @ torch.from_numpy(W)).numpy()
        y += params[s2.name + "/bias"].astype(np.float64) * sc2 + sh2 + params[s1.name + "/bias"].astype(np.float64) * sc1 + sh1
        _ref[(DUAL, B)] = np.maximum(y, 0).reshape(B, s2.hout, s2.hout, s2.cout)
    return _ref[(DUAL, B)]


_on = {}


def uncapped(engines, name, B):
    """the forced launch on the default grid, computed once and shared"""
    if (name, B) not in _on:
        _on[(name, B)] = run(engines["on"], name, B)
    return _on[(name, B)]


@pytest.mark.parametrize("name,B", CASES + [(DUAL, 1), (DUAL, 3)])
def test_error_against_fp64_matches_fp32_kernel(engines, params, name, B):
    """max|y - fp64| / max|fp64| < 5e-6 and <= 1.5 x the fp32-MFMA kernel's on the same inputs + 2^-26; both columns are printed.  For
    res2a it is the block output of the dual-source launch against the float64 GEMM over the concatenated k axis"""
    ref = dual_reference_fp64(params, B) if name == DUAL else reference_fp64(params, name, B)
    scale = np.abs(ref).max()
    e_old = float(np.abs(run(engines["off"], name, B).numpy().astype(np.float64) - ref).max() / scale)
    e_new = float(np.abs(uncapped(engines, name, B).numpy().astype(np.float64) - ref).max() / scale)
    print("stream1x1 %-16s B=%2d  fp32 MFMA %.3e  streaming split bf16 %.3e  ratio %.2f" % (name, B, e_old, e_new, e_new / max(e_old, 1e-30)))
    assert e_new < 5e-6, (name, B, e_old, e_new)
    assert e_new <= 1.5 * e_old + 2.0 ** -26, (name, B, e_old, e_new)


@pytest.mark.parametrize("walkers", [1, 9])
def test_walk_does_not_change_a_bit(engines, params, walkers):
    """the grid capped to one workgroup per 128-cout slice (it walks every tile, the partial one included) and to 9 (which divides none of the
    tile counts 98, 294, 25, 74, 907): bit for bit the uncapped launch"""
    e = make_engine(params, dict(FORCED, HPE_STREAM1X1_WALKERS=str(walkers)))
    try:
        for name, B in WALK_CASES:
            assert torch.equal(run(e, name, B), uncapped(engines, name, B)), (name, B, walkers)
    finally:
        e.close()


@pytest.mark.parametrize("name", ["res2c_branch2c", "res3b_branch2c", DUAL])
def test_repeatable_and_batch_position_does_not_change_a_bit(engines, name):
    x, res = (torch.from_numpy(a.copy()).cuda() for a in (dual_inputs(3) if name == DUAL else inputs(name, 3)))
    y = uncapped(engines, name, 3)
    assert torch.equal(run(engines["on"], name, 3), y)
    for i in range(3):
        assert torch.equal(run(engines["on"], name, 1, x[i:i + 1].contiguous(), res[i:i + 1].contiguous())[0], y[i]), i


def test_parameter_update_on_the_device(params):
    """after set_encoder_params_dev the layers compute what a fresh context built from those values computes: the repack kernel rewrites the
    split weights bit-identically -- the w_split packing of stage 3, the derived image behind w of res2c_branch2c and the one behind
    w_dual of res2a"""
    engine = make_engine(params, FORCED, reserve=1)
    names = ("res2c_branch2c", "res3b_branch2c", DUAL)
    p = torch.from_numpy(resnet_spec.params_to_flat(params))
    d = torch.randn(p.shape, generator=torch.Generator().manual_seed(5))
    q = p + d * (1e-2 * float(p.norm()) / float(d.norm()))
    fresh = make_engine(resnet_spec.flat_to_params(q, params), FORCED)
    try:
        before = {n: run(engine, n, 3) for n in names}
        engine.set_encoder_params_dev(q.cuda())
        got = {n: run(engine, n, 3) for n in names}
        want = {n: run(fresh, n, 3) for n in names}
    finally:
        engine.close()
        fresh.close()
    for n in names:
        assert torch.equal(got[n], want[n]) and not torch.equal(got[n], before[n]), n


def test_encoder_with_the_kernel_matches_the_plan_without_and_is_repeatable(params):
    """the whole encoder at B = 3 with both forms of the kernel forced against the same plan without it: the bound of
    test_split_encoder_matches_fp32_plan_and_is_repeatable, and bitwise equal across two runs"""
    off, on = make_engine(params, OFF), make_engine(params, FORCED)
    try:
        img = torch.from_numpy(synthetic.make_images(3, seed=31)).cuda()
        f0 = off.encoder(img).cpu().numpy().astype(np.float64)
        f1 = on.encoder(img).cpu().numpy()
        f2 = on.encoder(img).cpu().numpy()
        np.testing.assert_array_equal(f1, f2)
        err = float(np.abs(f1 - f0).max() / np.abs(f0).max())
        print("stream1x1 encoder B=3: max rel diff to the plan without it %.3e" % err)
        assert err < 2e-5, err
        assert not np.array_equal(f1, f0.astype(np.float32))  # the other arithmetic ran
    finally:
        off.close()
        on.close()
