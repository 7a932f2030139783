"""CPU companion of tests/test_gpu_head.py: the inputs of the head tests are finite in every output, and on them the float32
oracle stays under a quarter of each bar against the float64 oracle, in the per-image metric the GPU tests use.  A bar therefore
leaves a float32 kernel room for another summation order, and an edit of the edge set that breaks this shows here, without a GPU."""
import numpy as np
import pytest

from hpe_amd import synthetic
from oracle import hmr_oracle as O

from test_gpu_head import (BARS, POOL_BAR, POOL_CASES, REG_BAR, make_edge_thetas, pool_input, regress_features, regress_reference,
                           rel_rows, smpl_reference)


def test_edge_thetas_cover_the_nine_kinds():
    th = make_edge_thetas(17, seed=117)
    pose = th[:, 3:75].reshape(17, 24, 3)
    assert (pose == 0).all((1, 2)).any()  # 1. every pose entry 0
    assert ((pose[:, 1:] == 0).all(2).sum(1) == 1).any()  # 2. one non-root joint 0
    assert (pose[:, 0] == np.array([np.pi, 0, 0], np.float32)).all(1).any()  # 3. root rotation (pi, 0, 0)
    assert (pose == np.array([4.0, 4.0, 4.2], np.float32)).all(2).any()  # 4. angle 7.05
    assert (pose == np.array([1e-4, -2e-4, 5e-5], np.float32)).all(2).any()  # 5. a tiny angle
    assert (th[:, 75:] == 3).all(1).any() and (th[:, 75:] == -3).all(1).any()  # 6., 7. beta = +-3
    assert (th[:, 0] == np.float32(-0.03)).any() and (th[:, 0] == np.float32(1e-3)).any()  # 8., 9. camera scale
    assert not (th[:, 3:75] == np.float32(-1e-8)).any()  # batch_rodrigues is NaN there by definition
    for B in (1, 2, 7):  # any B works, and small batches with other seeds start elsewhere in the cycle
        assert make_edge_thetas(B, seed=100 + B).shape == (B, 85)
    assert not np.array_equal(make_edge_thetas(1, seed=101), make_edge_thetas(1, seed=102))


def test_float32_oracle_is_within_a_quarter_of_the_smpl_bars(smpl_model):
    """All six computed outputs hold in the per-image form (none needs the whole-tensor form)."""
    th = make_edge_thetas(17, seed=117)
    r32 = smpl_reference(O.SMPL(smpl_model), th)
    r64 = smpl_reference(O.SMPL(smpl_model, dtype=np.float64), th)
    for k, bar in BARS.items():
        assert r32[k].dtype == np.float32 and r64[k].dtype == np.float64, k
        assert np.isfinite(r32[k]).all() and np.isfinite(r64[k]).all(), k
        e = rel_rows(r32[k], r64[k])
        print("float32 oracle vs float64, edge thetas B=17: %-13s %.3g (bar %.0e)" % (k, e, bar))
        assert e < 0.25 * bar, (k, e)
    for k in ("theta", "cams"):
        np.testing.assert_array_equal(r32[k], r64[k].astype(np.float32))


@pytest.mark.parametrize("variant", ["survey", "bounded"])
@pytest.mark.parametrize("M", [1, 65])
def test_float32_oracle_is_within_a_quarter_of_the_regressor_bar(M, variant):
    reg = synthetic.make_regressor_params(variant=variant)
    mean = O.load_mean_param(synthetic.make_mean_params())
    feat = regress_features(M)
    th32 = np.tile(mean, (M, 1))
    a1 = regress_reference(reg, feat, th32)
    b1 = regress_reference(reg, feat, th32.astype(np.float64))
    prev = b1.astype(np.float32)
    a2 = regress_reference(reg, feat, prev)
    b2 = regress_reference(reg, feat, prev.astype(np.float64))
    assert a1.dtype == np.float32 and b1.dtype == np.float64
    for a, b in ((a1, b1), (a2, b2)):
        assert np.isfinite(a).all() and np.isfinite(b).all()
        e = rel_rows(a, b)
        print("float32 regressor vs float64, %s M=%d: %.3g" % (variant, M, e))
        assert e < 0.25 * REG_BAR, e


@pytest.mark.parametrize("B,HW,C", POOL_CASES)
def test_float32_mean_is_within_the_pool_bar(B, HW, C):
    """A float32 mean in plain sequential order, the longest chain a pool kernel may use (avgpool_kernel does).  The oracle has no
    float32 average pool of its own, and the quarter does NOT hold here: 49 signed terms in sequence sit at 3.7e-7 at (16, 49, 2048),
    per image and over the whole tensor alike (3.5e-7), so the 1e-6 bar leaves a factor of 2.7 for the order, not 4.  Asserted: the
    bar itself, with that order."""
    x = pool_input(B, HW, C)
    s = np.zeros((B, C), np.float32)
    for k in range(HW):
        s = s + x[:, k]
    e = rel_rows(s * np.float32(1.0 / HW), x.astype(np.float64).mean(1))
    print("float32 sequential mean vs float64 (%d, %d, %d): %.3g" % (B, HW, C, e))
    assert np.isfinite(x).all() and e < POOL_BAR, e
