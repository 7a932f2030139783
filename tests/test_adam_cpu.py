"""CPU checks of the optimiser's definition (tests/adam_ref.py), of why it is not torch.optim.Adam, and of the host build of the power
helper of csrc/adam.hip."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import adam_ref as R
from hpe_amd import _lib, build as hbuild

LR, B1, B2, EPS = 1e-4, 0.9, 0.999, 1e-7


def _grads(n, seed):
    rng = np.random.RandomState(seed)
    return rng.standard_normal(n) * rng.choice([1e-6, 1.0, 1e3], n)


def test_first_step_closed_form():
    """from zero moments, step 1 moves every element by lr * g / (|g| + eps / sqrt(1 - beta2)): where epsilon sits in the fused form"""
    g = _grads(4096, 0)
    z = np.zeros_like(g)
    p0 = z  # the update itself, not a difference of two values near 1
    for eps in (1e-7, 1e-3):
        p, _m, _v = R.step64(p0, z, z, g, R.alpha64(LR, B1, B2, 1), 1.0 - B1, 1.0 - B2, eps)
        want = LR * g / (np.abs(g) + eps / math.sqrt(1.0 - B2))
        np.testing.assert_allclose(p0 - p, want, rtol=1e-12, atol=0.0)


def test_float32_restatement_tracks_float64():
    g = _grads(4096, 2).astype(np.float32)
    p32 = p64 = np.random.RandomState(3).standard_normal(g.size).astype(np.float32)
    m32 = v32 = m64 = v64 = np.zeros_like(g)
    o1, o2 = R.one_minus(B1), R.one_minus(B2)
    for t in (1, 2, 3):
        a = R.alpha64(LR, B1, B2, t)
        p32, m32, v32 = R.step32(p32, m32, v32, g, a, o1, o2, EPS)
        p64, m64, v64 = R.step64(p64, m64, v64, g, a, o1, o2, EPS)
    for a, b in ((p32, p64), (m32, m64), (v32, v64)):
        assert R.rel_err(a, b) < 1e-6


def test_differs_from_torch_adam_by_more_than_rounding():
    """torch.optim.Adam divides by sqrt(v) / sqrt(1 - b2^t) + eps, the fused form by sqrt(v) + eps with the correction inside alpha: with
    eps = 1e-3 and gradients near eps the two updates differ by tens of percent, far above float32 rounding (the reason for the kernel);
    with eps -> 0 they agree."""
    g = (np.random.RandomState(4).standard_normal(1024) * 1e-3).astype(np.float32)
    p0 = np.random.RandomState(5).standard_normal(g.size).astype(np.float32)
    for eps, differs in ((1e-3, True), (1e-30, False)):
        tp = torch.from_numpy(p0.copy()).double().requires_grad_(True)
        opt = torch.optim.Adam([tp], lr=LR, betas=(B1, B2), eps=eps)
        p, m, v = p0.astype(np.float64), np.zeros(g.size), np.zeros(g.size)
        for t in (1, 2, 3):
            tp.grad = torch.from_numpy(g).double()
            opt.step()
            p, m, v = R.step64(p, m, v, g, R.alpha64(LR, B1, B2, t), 1.0 - B1, 1.0 - B2, eps)
        d = R.rel_err(p - p0, tp.detach().numpy() - p0)
        assert (d > 0.1) if differs else (d < 1e-9), (eps, d)


def test_host_power_helper_is_pythons_loop():
    hbuild.build()
    lib = _lib.load()
    out = C.c_double()
    for beta in (B1, B2):
        for t in (1, 2, 3, 1000, 2 ** 31 + 1):
            assert lib.hpe_debug_adam_power(beta, t, C.byref(out)) == 0
            assert out.value == R.power(beta, t), (beta, t)
    assert lib.hpe_debug_adam_power(B1, 0, C.byref(out)) == 0 and out.value == 1.0
    # each squaring doubles the relative error it inherits and adds half an ulp: at most t ulp after log2(t) of them
    assert abs(R.power(B2, 1000) / B2 ** 1000 - 1.0) < 1000 * 2.0 ** -52
    assert lib.hpe_debug_adam_power(B1, -1, C.byref(out)) == 1
    assert lib.hpe_debug_adam_power(B1, 1, None) == 1


def test_refusals_need_no_device():
    """the argument checks come before any launch"""
    hbuild.build()
    lib = _lib.load()
    buf = (C.c_double * 4)()
    ptr = C.cast(buf, C.c_void_p)
    assert lib.hpe_adam_advance(None, LR, B1, B2, None) == 1
    assert lib.hpe_adam_advance(ptr, LR, 1.0, B2, None) == 1
    assert lib.hpe_adam_advance(ptr, float("nan"), B1, B2, None) == 1
    assert lib.hpe_adam_set_step(None, 1, B1, B2, None) == 1
    assert lib.hpe_adam_set_step(ptr, -1, B1, B2, None) == 1
    assert lib.hpe_adam_apply(None, ptr, ptr, ptr, 4, ptr, 0.1, 0.001, EPS, None) == 1
    assert lib.hpe_adam_apply(ptr, ptr, ptr, None, 4, ptr, 0.1, 0.001, EPS, None) == 1
    assert lib.hpe_adam_apply(ptr, ptr, ptr, ptr, 4, None, 0.1, 0.001, EPS, None) == 1
    assert lib.hpe_adam_apply(ptr, ptr, ptr, ptr, -1, ptr, 0.1, 0.001, EPS, None) == 1
    assert lib.hpe_adam_apply(ptr, ptr, ptr, ptr, 0, ptr, 0.1, 0.001, EPS, None) == 0  # nothing to do, nothing launched


def test_keras_adam_refuses_host_tensors():
    import hpe_amd

    opt = hpe_amd.KerasAdam(LR)
    with pytest.raises(ValueError):
        opt.add("w", torch.zeros(8))
    with pytest.raises(ValueError):
        hpe_amd.KerasAdam(LR, beta_1=1.0)
    assert opt.iterations == 0
