"""The arithmetic of the split-bf16 fused Winograd kernel (tests/wino_split_ref.py) against an fp64 direct convolution, on inputs
spread over 24 binades: one fp32 accumulator for all six products stays inside the project's 5e-6 bar at k = C <= 128."""
import numpy as np
import pytest

import wino_split_ref as R


def test_split_is_exact_and_rounds_to_nearest():
    g = np.random.Generator(np.random.Philox(1))
    x = (g.normal(0, 1, 4096) * np.exp2(g.integers(-30, 30, 4096))).astype(np.float32)
    x[:8] = [0.0, 1.0, -1.0, 1.00390625, 1.01171875, 3.0e38, 1e-30, -257.0]  # ties: 1 + 2^-8 -> 1 (even), 1 + 3 * 2^-8 -> 1 + 2^-6
    h0, h1, h2 = R.split3(x)
    assert np.array_equal(h0.astype(np.float64) + h1.astype(np.float64) + h2.astype(np.float64), x.astype(np.float64))
    for h in (h0, h1, h2):
        assert not (h.view(np.uint32) & 0xFFFF).any()
    assert h0[3] == 1.0 and h0[4] == np.float32(1.015625)
    nz = x != 0
    assert (np.abs(h1[nz]) <= np.abs(x[nz]) * 2.0 ** -8).all() and (np.abs(h2[nz]) <= np.abs(x[nz]) * 2.0 ** -16).all()


def test_transforms_are_winograd():
    """fp32 transforms + an exact GEMM reproduce the direct convolution to fp32 rounding"""
    g = np.random.Generator(np.random.Philox(2))
    x = g.normal(0, 1, (6, 6, 8)).astype(np.float32)
    w = g.normal(0, 0.1, (3, 3, 8, 4)).astype(np.float32)
    M = np.einsum("ctk,cnk->ctn", R.input_transform(x).astype(np.float64), R.winograd_u(w).astype(np.float64))
    assert R.max_rel(R.output_transform(M.astype(np.float32), 6, 6), R.direct_fp64(x, w)) < 1e-6


@pytest.mark.parametrize("H,C", [(8, 64), (12, 64), (8, 128)])
def test_one_accumulator_within_bar(H, C):
    g = np.random.Generator(np.random.Philox(100 + H + C))
    x = R.dynamic_range_input(g, H, C)
    w = g.normal(0, np.sqrt(2.0 / (9 * C)), (3, 3, C, 16)).astype(np.float32)
    ref = R.direct_fp64(x, w)
    e1 = R.max_rel(R.split_layer(x, w), ref)
    e2 = R.max_rel(R.split_layer(x, w, accumulators=2), ref)
    ef = R.max_rel(R.fp32_mfma_layer(x, w), ref)
    print("H=%d C=%d  split, one accumulator %.3g  (two: %.3g)  fp32-MFMA model %.3g  ratio %.2f" % (H, C, e1, e2, ef, e1 / ef))
    assert e1 < 5e-6


def test_unscaled_inputs():
    g = np.random.Generator(np.random.Philox(7))
    x = g.normal(0, 1, (8, 8, 64)).astype(np.float32)
    w = g.normal(0, np.sqrt(2.0 / (9 * 64)), (3, 3, 64, 16)).astype(np.float32)
    ref = R.direct_fp64(x, w)
    e1, ef = R.max_rel(R.split_layer(x, w), ref), R.max_rel(R.fp32_mfma_layer(x, w), ref)
    print("N(0,1)  split, one accumulator %.3g  fp32-MFMA model %.3g  ratio %.2f" % (e1, ef, e1 / ef))
    assert e1 < 5e-6
