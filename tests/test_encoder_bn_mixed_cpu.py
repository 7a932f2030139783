"""The mixed-precision encoder walk with batch statistics without a GPU: the CPU restatement of tests/encoder_bn_mixed_ref.py against
tests/encoder_bn_train_ref.py (bit for bit with the roundings switched off), its distance from float64 per tensor kind (the figures the
GPU bars of tests/test_gpu_encoder_bn_mixed.py are built from), the precision keyword and the host-side ABI of the new reserve."""
import os
import re

import numpy as np
import pytest
import torch

import encoder_bn_mixed_ref as XB
import encoder_bn_train_ref as RB
import encoder_mixed_ref as X
import encoder_train_ref as R
from hpe_amd import _lib, build as hbuild, synthetic
from hpe_amd.resnet_spec import CONV_SPECS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# one layer of each class: conv1, 1x1, 1x1 stride 2, 3x3, projection shortcut
CLASSES = {"conv1": "conv1", "1x1": "res2a_branch2a", "1x1 stride 2": "res3a_branch2a", "3x3": "res2a_branch2b", "shortcut": "res2a_branch1"}
NEW_NAMES = ("hpe_encoder_train_reserve_batchnorm_mixed", "hpe_encoder_train_ws_floats_batchnorm_mixed", "hpe_encoder_forward_batchnorm_mixed",
             "hpe_encoder_backward_batchnorm_mixed", "hpe_debug_conv_batchnorm_mixed", "hpe_debug_conv_backward_batchnorm_mixed",
             "hpe_debug_encoder_stash_raw_mixed")


def _idx(name):
    return [s.name for s in CONV_SPECS].index(name)


@pytest.fixture(scope="module")
def params():
    p = synthetic.make_encoder_params(seed=7)
    g = np.random.default_rng(11)
    for s in CONV_SPECS:
        p[s.bn_name + "/gamma"] = g.uniform(0.5, 1.5, s.cout).astype(np.float32)
    return p


def _layer_inputs(s, B, seed, bf16):
    g = torch.Generator().manual_seed(seed)
    q = X.rne if bf16 else (lambda t: t)
    x = torch.randn(B, s.hin, s.hin, s.cin, generator=g)
    x = x if s.kh == 7 else q(x)  # conv1's x is the float32 image
    res = q(torch.randn(B, s.hout, s.hout, s.cout, generator=g)) if s.name.endswith("2c") else None
    dy = q(torch.randn(B, s.hout, s.hout, s.cout, generator=g))
    return x, res, dy


@pytest.mark.parametrize("cls", list(CLASSES))
def test_roundings_off_is_the_float32_restatement(params, cls):
    """with the roundings switched off the layer's forward and backward are encoder_bn_train_ref's in float32, bit for bit"""
    idx = _idx(CLASSES[cls])
    s = CONV_SPECS[idx]
    gated = cls != "shortcut"
    x, res, dy = _layer_inputs(s, 1, 300 + idx, bf16=False)
    lt = R.layer_tensors(params, s, torch.float32)
    ref_f = RB.layer_forward(s, x, lt, res, gated)
    got_f = XB.layer_forward_mixed(s, x, lt, res, gated, rounding=False)
    for a, b in zip(got_f, ref_f):
        assert torch.equal(a, b), cls
    y, z = ref_f[0], ref_f[1]
    ref = RB.layer_backward(s, x, z, y if gated else None, dy, lt, gated=gated)
    got = XB.layer_backward_mixed(s, x, z, y if gated else None, dy, lt, gated=gated, rounding=False)
    for k in ref:
        assert torch.equal(got[k], ref[k]), (cls, k)
    assert ("dx" in ref) == (idx != 0)
    # with the roundings on something really is rounded: the statistics are those of another tensor
    on = XB.layer_forward_mixed(s, x, lt, res, gated)
    assert not torch.equal(on[1], z) and not torch.equal(on[2], ref_f[2])
    assert torch.equal(on[1], X.rne(on[1])) and torch.equal(on[0], X.rne(on[0]))


def test_network_roundings_off_is_the_float32_restatement(params):
    """network_backward_mixed with the roundings off against encoder_bn_train_ref.network_backward in float32, bit for bit, on stashes of
    random values (the backward is driven by whatever the stashes hold: no forward is needed)"""
    g = torch.Generator().manual_seed(78)
    zstash = [torch.randn(1, s.hout, s.hout, s.cout, generator=g) for s in CONV_SPECS]
    stash = [torch.relu(torch.randn(1, s.hout, s.hout, s.cout, generator=g)) for s in CONV_SPECS]
    pooled = torch.nn.functional.max_pool2d(torch.nn.functional.pad(stash[0].permute(0, 3, 1, 2), (1, 1, 1, 1)), 3, 2).permute(0, 2, 3, 1).contiguous()
    img = torch.from_numpy(synthetic.make_images(1, seed=5))
    gf = torch.randn(1, 2048, generator=g)
    win = R.maxpool_winners(stash[0])
    ref = RB.network_backward(params, img, zstash, stash, pooled, win, gf, dtype=torch.float32)
    got = XB.network_backward_mixed(params, img, zstash, stash, pooled, win, gf, rounding=False)
    assert torch.equal(got, ref)


@pytest.mark.parametrize("cls", list(CLASSES))
def test_distance_from_float64(params, cls):
    """how far the mixed restatement and the float32 one are from float64 on bf16 inputs with W16 as the kernel, per tensor kind.  Driven
    by the same z16 and y16, dbeta and dgamma of the two float32 restatements are the same numbers (nothing of them is rounded); dW
    and dx see the rounding of dzraw16, dx one more"""
    idx = _idx(CLASSES[cls])
    s = CONV_SPECS[idx]
    gated = cls != "shortcut"
    x, res, dy = _layer_inputs(s, 1, 400 + idx, bf16=True)
    lt = R.layer_tensors(params, s, torch.float32)
    lt16 = X.weights16(lt)
    x16 = X.rne(x)
    y, z, mu, var = XB.layer_forward_mixed(s, x, lt, res, gated)
    # forward: z16 within half a bf16 ulp of the float64 convolution (+ its fp32 part), the statistics those of z16
    z64 = RB.layer_raw(s, x16.double(), [t.double() for t in lt16])
    assert bool(((z.double() - z64).abs() <= 2.0 ** -8 * z64.abs() + 1e-5 * float(z64.abs().max())).all())
    mu64, var64 = RB.batch_stats(z.double())
    assert float(((mu.double() - mu64).abs() / torch.maximum(mu64.abs(), var64.sqrt())).max()) < 1e-5
    yy = y if gated else None
    ref = RB.layer_backward(s, x16.double(), z.double(), yy, dy.double(), [t.double() for t in lt16], gated=gated)
    f32 = RB.layer_backward(s, x16, z, yy, dy, lt16, gated=gated)
    mixed = XB.layer_backward_mixed(s, x, z, yy, dy, lt, gated=gated)
    assert float(mixed["db"].abs().max()) == 0.0
    for k in ("dW", "dgamma", "dbeta") + (("dx",) if idx else ()):
        e32, emx = R.rel(f32[k], ref[k]), R.rel(mixed[k], ref[k])
        print("%-13s %-16s %-6s float32 %.3g  mixed %.3g" % (cls, s.name, k, e32, emx))
        if k in ("dgamma", "dbeta"):
            assert torch.equal(mixed[k], f32[k])  # rounding point 4: fp32, never rounded to bf16
            assert e32 < 1e-5
        else:
            assert e32 < 1e-5 and emx < 2.0 ** -7  # dzraw16's rounding, and for dx its own: each at most 2^-8 per element


def test_the_precision_keyword():
    """ "mixed" is accepted with both BatchNorm modes; "bf16" stays the frozen-only spelling and its refusal stays as it was"""
    import hpe_amd

    M = hpe_amd.HpeEngine._mixed
    assert M("mixed") is True and M("mixed", "batch") is True and M("mixed", "frozen") is True
    assert M("bf16") is True and M("fp32") is False and M("fp32", "batch") is False
    with pytest.raises(ValueError, match="follow-up"):
        M("bf16", "batch")
    with pytest.raises(ValueError, match="precision"):
        M("half", "batch")
    with pytest.raises(ValueError):
        M("mixed", "moving")
    with pytest.raises(ValueError, match="follow-up"):
        hpe_amd.encoder_features(None, None, None, bn="batch", precision="bf16")


def test_abi_names():
    txt = open(os.path.join(ROOT, "include", "hpe.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    hbuild.build()
    lib = _lib.load()
    for name in NEW_NAMES:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in _lib.declared_symbols(), name
        assert hasattr(lib, name), name


@pytest.mark.parametrize("B", [1, 3, 17])
def test_ws_floats_batchnorm_mixed(B):
    """what the reserve adds to the two it shares: the bf16 raw-output stash (two elements a float) and nothing else.  The two existing
    reports both contain the fp32 reserve, which is counted once"""
    hbuild.build()
    lib = _lib.load()
    base, bn, mixed = lib.hpe_encoder_train_ws_floats(B), lib.hpe_encoder_train_ws_floats_batchnorm(B), lib.hpe_encoder_train_ws_floats_mixed(B)
    both = lib.hpe_encoder_train_ws_floats_batchnorm_mixed(B)
    zstash16 = B * sum(s.hout * s.hout * s.cout for s in CONV_SPECS) // 2
    assert both - (bn + mixed - base) == zstash16
    assert both > bn > base and both > mixed


def test_ws_floats_batchnorm_mixed_refuses_zero():
    hbuild.build()
    lib = _lib.load()
    assert lib.hpe_encoder_train_ws_floats_batchnorm_mixed(0) == 0 and lib.hpe_encoder_train_ws_floats_batchnorm_mixed(-3) == 0
