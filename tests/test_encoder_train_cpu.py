"""Encoder training without a GPU: the flat layout against the library, the restatement of tests/encoder_train_ref.py against float64
autograd of conv2d + affine + ReLU on one layer of each class, the max-pool tie rule, and the fp32 error budget of the restatement."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import encoder_train_ref as R
from hpe_amd import _lib, build as hbuild, resnet_spec, synthetic
from hpe_amd.resnet_spec import CONV_SPECS, CONV_INDEX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# one layer of each class: 7x7 s2, 1x1 s1, 3x3, 1x1 s1 with a residual, 1x1 s2 (projection shortcut)
CLASSES = {"conv1": ("conv1", False), "1x1": ("res5b_branch2a", False), "3x3": ("res5b_branch2b", False), "1x1+res": ("res5b_branch2c", True),
           "1x1s2": ("res5a_branch1", False), "1x1s2a": ("res5a_branch2a", False)}


@pytest.fixture(scope="module")
def lib():
    hbuild.build()
    return _lib.load()


def test_abi_exports_encoder_training(lib):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hpe.h")).read(), flags=re.S)
    for name in ("hpe_encoder_param_floats", "hpe_encoder_param_offset", "hpe_encoder_train_reserve", "hpe_encoder_train_ws_floats",
                 "hpe_encoder_forward_train", "hpe_encoder_backward", "hpe_encoder_get_params", "hpe_encoder_set_params",
                 "hpe_debug_conv_backward", "hpe_debug_maxpool_backward", "hpe_debug_avgpool_backward", "hpe_debug_encoder_stash",
                 "hpe_debug_encoder_stash_batch",
                 "hpe_encoder_wg_slices"):
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in _lib.declared_symbols() and hasattr(lib, name), name
    # refusals that need no device: NULL ctx
    assert lib.hpe_encoder_train_reserve(None, 1) == 1
    assert lib.hpe_encoder_backward(None, None, 1, None, None, None) == 1


def test_flat_layout_matches_library(lib):
    assert lib.hpe_encoder_param_floats() == resnet_spec.ENCODER_PARAM_FLOATS
    total = 0
    for i, (s, off) in enumerate(zip(CONV_SPECS, resnet_spec.ENCODER_PARAM_OFFSETS)):
        assert tuple(lib.hpe_encoder_param_offset(i, w) for w in range(4)) == off
        assert off[0] == total
        total += s.kh * s.kw * s.cin * s.cout + 3 * s.cout
    assert total == resnet_spec.ENCODER_PARAM_FLOATS
    assert lib.hpe_encoder_param_offset(53, 0) == -1 and lib.hpe_encoder_param_offset(0, 4) == -1 and lib.hpe_encoder_param_offset(-1, 0) == -1
    assert lib.hpe_encoder_train_ws_floats(1) > 11_000_000 and lib.hpe_encoder_train_ws_floats(0) == 0
    # the documented size is added up from the list the reserve allocates from: the values of commit 03ecb51, which added them up by hand
    want = {1: 64282288, 2: 78082736, 3: 91883184, 8: 163244720, 64: 939739824}
    assert {B: lib.hpe_encoder_train_ws_floats(B) for B in want} == want
    # conv1 and stage 2 at B = 3 are cut into more than one pixel slice; the 7x7 maps at B = 3 (147 pixels) are not
    assert lib.hpe_encoder_wg_slices(0, 3) > 1 and lib.hpe_encoder_wg_slices(2, 3) > 1 and lib.hpe_encoder_wg_slices(52, 3) == 1


def test_flat_round_trip():
    p = synthetic.make_encoder_params(seed=3)
    flat = resnet_spec.params_to_flat(p)
    q = resnet_spec.flat_to_params(flat, p)
    assert set(q) == set(p)
    for k in p:
        assert np.array_equal(np.asarray(p[k], np.float32), q[k]), k
    o = resnet_spec.ENCODER_PARAM_OFFSETS[CONV_INDEX["res3a_branch1"]]
    assert np.array_equal(flat[o[2]:o[3]], p["bn3a_branch1/gamma"])


def _case(name, B=2, seed=0):
    lname, with_res = CLASSES[name]
    s = CONV_SPECS[CONV_INDEX[lname]]
    g = torch.Generator().manual_seed(seed)
    p = synthetic.make_encoder_params(seed=5)
    p[s.bn_name + "/gamma"] = np.random.default_rng(1).uniform(0.5, 1.5, s.cout).astype(np.float32)
    lt = R.layer_tensors(p, s)
    hin = 32 if s.kh == 7 else s.hin  # conv1 on a smaller image: the class, not the size
    s = s._replace(hin=hin, hout=hin // s.stride)
    x = torch.randn(B, s.hin, s.hin, s.cin, generator=g, dtype=torch.float64)
    res = torch.randn(B, s.hout, s.hout, s.cout, generator=g, dtype=torch.float64) if with_res else None
    dy = torch.randn(B, s.hout, s.hout, s.cout, generator=g, dtype=torch.float64)
    return s, lt, x, res, dy


def _autograd(s, lt, x, res, dy):
    W, b, gamma, beta, mean, var = [t.clone().requires_grad_(i < 4) for i, t in enumerate(lt)]
    x = x.clone().requires_grad_(True)
    z = F.conv2d(x.permute(0, 3, 1, 2), W.permute(3, 2, 0, 1), stride=s.stride, padding=(s.kh - 1) // 2).permute(0, 2, 3, 1)
    y = gamma * (z + b - mean) / torch.sqrt(var + R.EPS) + beta
    if res is not None:
        y = y + res
    y = torch.relu(y)
    (y * dy).sum().backward()
    return y.detach(), {"dx": x.grad, "dW": W.grad, "db": b.grad, "dgamma": gamma.grad, "dbeta": beta.grad}


@pytest.mark.parametrize("name", sorted(CLASSES))
def test_restatement_matches_autograd(name):
    """dW = s * G, dgamma through <W, G> (no pre-BN tensor, no division by s), and the flipped-kernel / scatter forms of dx"""
    s, lt, x, res, dy = _case(name)
    y, ref = _autograd(s, lt, x, res, dy)
    assert torch.allclose(R.layer_forward(s, x, lt, res), y, rtol=0, atol=1e-11)
    got = R.layer_backward(s, x, y, dy, lt)
    for k in ("dW", "db", "dgamma", "dbeta") + (("dx",) if s.kh != 7 else ()):
        assert R.rel(got[k], ref[k]) < 1e-12, (k, R.rel(got[k], ref[k]))


def test_maxpool_tie_rule():
    """positive ties go to the first maximum in row-major order; an all-zero window goes to the pad (top / left windows) or to its first
    pixel, where conv1's gate kills it"""
    x = torch.zeros(1, 8, 8, 2, dtype=torch.float64)
    x[0, 3, 3, 0] = x[0, 3, 4, 0] = x[0, 4, 3, 0] = 2.0  # window (ho 2, wo 2) covers rows 3..5, cols 3..5: tie between (3,3), (3,4), (4,3)
    x[0, 5, 5, 1] = x[0, 6, 6, 1] = 1.0
    win = R.maxpool_winners(x)
    assert (int(win[0][0, 2, 2, 0]), int(win[1][0, 2, 2, 0])) == (3, 3)
    assert int(win[0][0, 0, 0, 0]) == -1  # all zero, the pad comes first
    assert (int(win[0][0, 3, 3, 1]), int(win[1][0, 3, 3, 1])) == (5, 5)
    dy = torch.ones(1, 4, 4, 2, dtype=torch.float64)
    dx = R.maxpool_backward(win, dy, 8)
    # away from ties the rule is autograd's
    g = torch.Generator().manual_seed(0)
    xr = torch.rand(2, 8, 8, 3, generator=g, dtype=torch.float64).requires_grad_(True)
    yr = F.max_pool2d(F.pad(xr.permute(0, 3, 1, 2), (1, 1, 1, 1)), 3, 2).permute(0, 2, 3, 1)
    dyr = torch.randn(2, 4, 4, 3, generator=g, dtype=torch.float64)
    (yr * dyr).sum().backward()
    assert torch.equal(R.maxpool_backward(R.maxpool_winners(xr.detach()), dyr, 8), xr.grad)
    assert dx[0, 3, 3, 0] >= 1 and dx[0, 3, 4, 0] == 0 and dx[0, 4, 3, 0] == 0
    assert float(dx.sum()) < float(dy.sum())  # the pad swallowed the all-zero windows on the border


def test_fp32_budget(capsys):
    """the same restatement in float32 against float64 on those inputs: the budget the GPU bars take their margin over"""
    worst = {}
    for name in sorted(CLASSES):
        s, lt, x, res, dy = _case(name, B=3)
        y = R.layer_forward(s, x, lt, res)
        ref = R.layer_backward(s, x, y, dy, lt)
        got = R.layer_backward(s, x.float(), y.float(), dy.float(), [t.float() for t in lt])
        for k in ref:
            if k != "dz":
                worst[(name, k)] = R.rel(got[k], ref[k])
    with capsys.disabled():
        for (name, k), e in sorted(worst.items()):
            print("fp32 restatement vs float64  %-8s %-7s %.3g" % (name, k, e))
    assert max(worst.values()) < 1e-5  # fp32 with a few thousand terms: anything above this is a bug in the restatement, not rounding
