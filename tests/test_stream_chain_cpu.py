"""The arithmetic of the chained streaming kernel (csrc/conv_stream_chain_f32s.hip) restated in NumPy (stream_chain_ref.py) against a
float64 chain, on the inputs the GPU tests use: before any GPU run this shows that the project's single-conv bar, 5e-6 of the largest
output, holds for t3 AND for u1 -- whose operand t3 is itself a rounded result -- at C = 64, in both forms.  And the k order of the reduce
is a permutation."""
import numpy as np
import pytest

import stream_chain_ref as R
import test_gpu_stream1x1 as S
from hpe_amd import resnet_spec, synthetic

BAR = 5e-6


def test_reduce_k_order_is_a_permutation_in_accumulator_order():
    p = R.chain_perm()
    assert sorted(p.tolist()) == list(range(32))
    # the register order of a transposed 32x32 accumulator: register 4 j + i of lane half hi holds row 8 j + 4 hi + i; k-step s takes
    # registers 8 s .. 8 s + 7 of each half
    for s in range(2):
        for hi in range(2):
            regs = [8 * s + t for t in range(8)]
            assert [R.chain_k(s, hi, t) for t in range(8)] == [8 * (r // 4) + 4 * hi + r % 4 for r in regs]


def test_split_gemm_is_independent_of_a_k_order_inside_the_bar():
    g = np.random.Generator(np.random.Philox(77))
    A, W = g.normal(0, 1, (64, 32)).astype(np.float32), g.normal(0, 1, (48, 32)).astype(np.float32)
    ref = A.astype(np.float64) @ W.astype(np.float64).T
    for order in (None, R.chain_perm()):
        got = R.split_gemm(A, W, order)
        assert np.abs(got - ref).max() / np.abs(ref).max() < 1e-6


def operands(params, first):
    """what the library hands the kernel, in fp32: (WA [256,K], scaleA, shiftA, WB [64,256], scaleB, shiftB) of res2a (first) or res2b"""
    i2c = resnet_spec.CONV_INDEX["res2a_branch2c" if first else "res2b_branch2c"]
    s2 = resnet_spec.CONV_SPECS[i2c]
    sn = resnet_spec.CONV_SPECS[i2c + (2 if first else 1)]
    assert sn.name == ("res2b_branch2a" if first else "res2c_branch2a")

    def fold(s):
        sc, sh = S.bn_fold(params, s)
        return sc, sh + params[s.name + "/bias"].astype(np.float64) * sc

    def wt(s):
        return params[s.name + "/kernel"].astype(np.float64).reshape(s.cin, s.cout).T

    sc2, sh2 = fold(s2)
    scn, shn = fold(sn)
    f = lambda a: np.asarray(a, np.float64).astype(np.float32)
    if first:
        s1 = resnet_spec.CONV_SPECS[i2c + 1]
        sc1, sh1 = fold(s1)
        WA = np.concatenate([wt(s2) * sc2[:, None], wt(s1) * sc1[:, None]], axis=1)
        return f(WA), np.ones(256, np.float32), f(sh2 + sh1), f(wt(sn)), f(scn), f(shn)
    return f(wt(s2)), f(sc2), f(sh2), f(wt(sn)), f(scn), f(shn)


@pytest.mark.parametrize("first", [False, True])
def test_model_meets_the_bar_against_fp64(first):
    params = synthetic.make_encoder_params()
    ops = operands(params, first)
    if first:
        t2, x = S.dual_inputs(1)
        a, res = np.concatenate([t2.reshape(-1, 64), x.reshape(-1, 64)], axis=1), None
    else:
        t2, res = S.inputs("res2b_branch2c", 1)
        a, res = t2.reshape(-1, 64), res.reshape(-1, 256)
    WA, scA, shA, WB, scB, shB = ops
    t3, u1 = R.chain_model(a, WA, scA, shA, res, WB, scB, shB)
    r3, r1 = R.chain_fp64(a, WA, scA, shA, res, WB, scB, shB)
    e3 = float(np.abs(t3 - r3).max() / np.abs(r3).max())
    e1 = float(np.abs(u1 - r1).max() / np.abs(r1).max())
    print("stream chain model (%s): t3 %.3e  u1 %.3e of the largest output" % ("conv_block" if first else "identity", e3, e1))
    assert t3.dtype == np.float32 and u1.dtype == np.float32 and (u1 > 0).any() and (t3 > 0).any()
    assert e3 < BAR and e1 < BAR, (e3, e1)
