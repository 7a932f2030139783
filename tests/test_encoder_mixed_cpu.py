"""The mixed-precision encoder walks without a GPU: the CPU restatement of tests/encoder_mixed_ref.py against tests/encoder_train_ref.py
(bit for bit with the roundings switched off), its RNE helper against torch.bfloat16, its distance from float64 (the figures the GPU
bars of tests/test_gpu_encoder_mixed.py multiply), and the host-side ABI of the mixed reserve."""
import os
import re

import numpy as np
import pytest
import torch

import encoder_mixed_ref as X
import encoder_train_ref as R
from hpe_amd import _lib, build as hbuild, synthetic
from hpe_amd.resnet_spec import CONV_SPECS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# one layer of each class: conv1, 1x1, 1x1 stride 2, 3x3, projection shortcut
CLASSES = {"conv1": "conv1", "1x1": "res2a_branch2a", "1x1 stride 2": "res3a_branch2a", "3x3": "res2a_branch2b", "shortcut": "res2a_branch1"}
NEW_NAMES = ("hpe_encoder_train_reserve_mixed", "hpe_encoder_train_ws_floats_mixed", "hpe_encoder_forward_train_mixed", "hpe_encoder_backward_mixed",
             "hpe_debug_conv_backward_mixed", "hpe_debug_maxpool_backward_mixed", "hpe_debug_avgpool_backward_mixed", "hpe_debug_encoder_stash_mixed",
             "hpe_debug_encoder_stash_batch_mixed")


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
    dy = q(torch.randn(B, s.hout, s.hout, s.cout, generator=g))
    y = q(torch.relu(torch.randn(B, s.hout, s.hout, s.cout, generator=g)))
    return x, y, dy


def test_rne_matches_torch_bfloat16():
    g = torch.Generator().manual_seed(1)
    special = torch.tensor([0.0, -0.0, 1.0, -1.0, float("inf"), -float("inf"), 3.4028234663852886e38, -3.4028234663852886e38,
                            1.1754943508222875e-38, 1e-40, -1e-40, 1.401298464324817e-45, 9.183549615799121e-41], dtype=torch.float32)
    # exact ties: a bf16 value plus half of its ulp, on an even and on an odd last bit, both signs, normal and denormal
    hi = torch.tensor([0x3F80, 0x3F81, 0x4049, 0x7F7E, 0x7F7F, 0x0001, 0x0002, 0x007F, 0x0080], dtype=torch.int64)
    ties = ((hi << 16) | 0x8000).to(torch.int32).view(torch.float32)
    near = (((hi << 16) | 0x8001).to(torch.int32).view(torch.float32), ((hi << 16) | 0x7FFF).to(torch.int32).view(torch.float32))
    rand = torch.randn(100000, generator=g) * torch.exp(torch.randn(100000, generator=g) * 20)
    t = torch.cat([special, ties, -ties, near[0], near[1], rand, rand * 1e-39])
    got, ref = X.rne(t), t.to(torch.bfloat16).to(torch.float32)
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32))
    assert bool(torch.isinf(X.rne(torch.tensor([3.4028234663852886e38]))).all())  # the largest finite rounds up to infinity
    assert bool(torch.isnan(X.rne(torch.tensor([float("nan")]))).all())
    assert not torch.equal(X.rne(ties), ties)  # the ties really were between two bf16 values


@pytest.mark.parametrize("cls", list(CLASSES))
def test_roundings_off_is_the_float32_restatement(params, cls):
    """with the roundings switched off layer_backward_mixed is encoder_train_ref.layer_backward in float32, bit for bit"""
    idx = _idx(CLASSES[cls])
    s = CONV_SPECS[idx]
    gated = cls != "shortcut"
    x, y, dy = _layer_inputs(s, 1, 100 + idx, bf16=False)
    lt = R.layer_tensors(params, s, torch.float32)
    ref = R.layer_backward(s, x, y if gated else None, dy, lt, gated=gated)
    got = X.layer_backward_mixed(s, x, y if gated else None, dy, lt, gated=gated, rounding=False)
    for k in ref:
        assert torch.equal(got[k], ref[k]), (cls, k)
    assert ("dx" in ref) == (idx != 0)
    # the forward counterpart, and with the roundings on something really is rounded
    assert torch.equal(X.layer_forward_mixed(s, x, lt, relu=gated, rounding=False), R.layer_forward(s, x, lt, relu=gated))
    on = X.layer_backward_mixed(s, x, y if gated else None, dy, lt, gated=gated)
    assert not torch.equal(on["dgamma"], ref["dgamma"])  # <W16, G>: the rounded kernel enters


def test_network_roundings_off_is_the_float32_restatement(params):
    """network_backward_mixed with the roundings off against encoder_train_ref.network_backward in float32, bit for bit, on a stash of
    random values (the backward is driven by whatever the stash holds: no forward is needed)"""
    g = torch.Generator().manual_seed(77)
    stash = [torch.relu(torch.randn(1, s.hout, s.hout, s.cout, generator=g)) for s in CONV_SPECS]
    pooled = torch.nn.functional.max_pool2d(torch.nn.functional.pad(stash[0].permute(0, 3, 1, 2), (1, 1, 1, 1)), 3, 2).permute(0, 2, 3, 1).contiguous()
    img = torch.from_numpy(synthetic.make_images(1, seed=5))
    gf = torch.randn(1, 2048, generator=g)
    win = R.maxpool_winners(stash[0])
    ref = R.network_backward(params, img, stash, pooled, win, gf, dtype=torch.float32)
    got = X.network_backward_mixed(params, img, stash, pooled, win, gf, rounding=False)
    assert torch.equal(got, ref)


@pytest.mark.parametrize("cls", list(CLASSES))
def test_distance_from_float64(params, cls):
    """how far the mixed restatement and the float32 one are from float64 on bf16 inputs with W16 as the kernel: the float32 figure is what
    the GPU bars multiply by 4; the mixed one differs from it only in dx (one more rounding to bf16)"""
    idx = _idx(CLASSES[cls])
    s = CONV_SPECS[idx]
    gated = cls != "shortcut"
    x, y, dy = _layer_inputs(s, 1, 200 + idx, bf16=True)
    lt = R.layer_tensors(params, s, torch.float32)
    lt16 = X.weights16(lt)
    x16 = X.rne(x)
    yy = y if gated else None
    ref = R.layer_backward(s, x16.double(), yy, dy.double(), [t.double() for t in lt16], gated=gated)
    f32 = R.layer_backward(s, x16, yy, dy, lt16, gated=gated)
    mixed = X.layer_backward_mixed(s, x, yy, dy, lt, gated=gated)
    for k in ("dW", "db", "dgamma", "dbeta") + (("dx",) if idx else ()):
        e32, emx = R.rel(f32[k], ref[k]), R.rel(mixed[k], ref[k])
        print("%-13s %-16s %-6s float32 %.3g  mixed %.3g" % (cls, s.name, k, e32, emx))
        if k != "dx":
            assert torch.equal(mixed[k], f32[k])  # rounding point 8: nothing of the weight gradient is rounded to bf16
            assert 0 < e32 < 1e-5
        else:
            assert emx < 2.0 ** -8  # a norm-relative error cannot exceed the per-element bound of one rounding (+ the fp32 part)


def test_bf16_with_batch_statistics_is_refused():
    """precision="bf16" with bn="batch" raises ValueError naming the follow-up, before anything touches a device"""
    import hpe_amd

    with pytest.raises(ValueError, match="follow-up"):
        hpe_amd.HpeEngine._mixed("bf16", "batch")
    with pytest.raises(ValueError, match="follow-up"):
        hpe_amd.encoder_features(None, None, None, bn="batch", precision="bf16")
    with pytest.raises(ValueError, match="precision"):
        hpe_amd.encoder_features(None, None, None, precision="half")
    assert hpe_amd.HpeEngine._mixed("bf16") is True and hpe_amd.HpeEngine._mixed("fp32", "batch") is False


def test_abi_names():
    txt = open(os.path.join(ROOT, "include", "hpe.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    hbuild.build()
    lib = _lib.load()
    for name in NEW_NAMES:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in _lib.declared_symbols(), name
        assert hasattr(lib, name), name


def _mixed_list_floats(B):
    """the buffer list of hpe_encoder_train_reserve_mixed, in floats (two bf16 elements each)"""
    rup = lambda x, m: (x + m - 1) // m * m
    stash = sum(s.hout * s.hout * s.cout for s in CONV_SPECS) + 56 * 56 * 64
    big, mid, padded = 802816, 200704, 230 * 232 * 4
    n = B * (stash + 3 * big + 3 * mid + padded) // 2
    for i, s in enumerate(CONV_SPECS):
        k_pad = rup(7 * 32 if i == 0 else s.kh * s.kw * s.cin, 64)
        n += rup(s.cout, 128) * k_pad // 2
        if i:
            n += rup(s.cin, 128) * s.kh * s.kw * s.cout // 2
    return n + (2 * len(CONV_SPECS) - 1) * 32 // 4  # the cast table: one 32-byte segment per operand


@pytest.mark.parametrize("B", [1, 3, 17])
def test_ws_floats_mixed(B):
    hbuild.build()
    lib = _lib.load()
    base, mixed = lib.hpe_encoder_train_ws_floats(B), lib.hpe_encoder_train_ws_floats_mixed(B)
    assert mixed > base > 0
    assert mixed - base == _mixed_list_floats(B)
    assert lib.hpe_encoder_train_ws_floats_mixed(0) == 0
