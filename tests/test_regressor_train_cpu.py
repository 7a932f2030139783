"""CPU-side checks of regressor training: the flat parameter layout against regressor_spec and the library's offsets; in float64 the
identity the HIP backward relies on (gates from a > 0, the feature block of W1 hoisted, weight gradients as products over the stacked
rows) against autograd of the IEF loop; the share of generated rows the GPU test keeps; and the headroom of the fp32 torch restatement
under the GPU bars on exactly the rows the GPU test uses."""
import numpy as np
import pytest
import torch

from hpe_amd import regressor_spec

import regressor_train_ref as T

GPU_BAR = 1e-4  # tests/test_gpu_regressor_train.py: per tensor, worst absolute error / largest reference magnitude
FWD_BAR = 5e-6  # ... and its forward bar, rel per image


def test_flat_layout():
    layout = regressor_spec.flat_layout()
    assert [k for k, _o, _s in layout] == ["dense_0/kernel", "dense_0/bias", "dense_1/kernel", "dense_1/bias", "dense_2/kernel", "dense_2/bias",
                                           "mean_theta"]
    assert regressor_spec.PARAM_FLOATS == 2133 * 1024 + 1024 + 1024 * 1024 + 1024 + 1024 * 85 + 85 + 85 == 3322026
    # the library's table (host code: runs without a GPU)
    from hpe_amd import _lib, build as hbuild

    hbuild.build()
    lib = _lib.load()
    assert lib.hpe_regressor_param_floats() == regressor_spec.PARAM_FLOATS
    for i in range(3):
        assert lib.hpe_regressor_param_offset(i, 0) == layout[2 * i][1] and lib.hpe_regressor_param_offset(i, 1) == layout[2 * i + 1][1]
    assert lib.hpe_regressor_param_offset(3, 0) == layout[6][1] == regressor_spec.PARAM_FLOATS - 85
    for bad in ((3, 1), (4, 0), (-1, 0), (-1, 1)):
        assert lib.hpe_regressor_param_offset(*bad) == -1
    # dict <-> flat, both ways
    params, mean = T.fixture_params()
    flat = regressor_spec.params_to_flat(params, mean)
    assert flat.dtype == np.float32 and flat.shape == (regressor_spec.PARAM_FLOATS,)
    assert flat[lib.hpe_regressor_param_offset(0, 0) + 2050 * 1024 + 7] == params["dense_0/kernel"][2050, 7]  # kernels are [in, out], row-major
    assert flat[lib.hpe_regressor_param_offset(2, 0) + 5 * 85 + 84] == params["dense_2/kernel"][5, 84]
    back = regressor_spec.flat_to_params(torch.from_numpy(flat))
    assert sorted(back) == sorted(list(params) + ["mean_theta"])
    for key in params:
        assert back[key].dtype == np.float32 and np.array_equal(back[key], params[key]), key
    assert np.array_equal(back["mean_theta"], mean)
    with pytest.raises(ValueError):
        regressor_spec.flat_to_params(flat[:-1])


def test_kernel_arithmetic_is_the_autograd_gradient():
    """B = 5, cotangents on all stages, dropout on: 1e-12 relative on all seven tensors and on grad_features"""
    P = T.pool()
    feat, drop, gt = T.case(5, with_drop=True, last_only=False)
    want, want_f = T.autograd_grads(P["flat"], feat, drop, gt)
    got, got_f = T.kernel_arithmetic(P["flat"], feat, drop, gt)
    errs = T.per_tensor_errors(got, want, got_f, want_f)
    print("  ".join("%s %.3g" % kv for kv in errs))
    assert len(errs) == 8
    for key, e in errs:
        assert e <= 1e-12, (key, e)
    for key, off, shape in regressor_spec.flat_layout():
        assert np.abs(want[off : off + int(np.prod(shape))]).max() > 0, key
    # the forward's dropout acts at the last stage only
    a, b = T.forward(P["flat"], feat, None), T.forward(P["flat"], feat, drop)
    assert np.array_equal(a[:2], b[:2]) and not np.array_equal(a[2], b[2])


def test_rows_stay_clear_of_the_kinks():
    P = T.pool()
    share = P["kept"] / P["generated"]
    print("rows away from a kink: %d of %d generated (%.1f %%)" % (P["kept"], P["generated"], 100 * share))
    assert share >= 0.90
    assert P["kept"] >= max(T.BATCHES)
    pre = T.kink_distance(P["flat"], P["feat"], drops=(None, P["drop"]))
    assert pre.min() > T.KINK
    with torch.no_grad():
        _, z = T.ief(T.tensors(P["flat"], requires_grad=False), torch.from_numpy(P["feat"]).double())
    print("pre-activation RMS: layer 1 %.3g, layer 2 %.3g" % (float(z[0].pow(2).mean().sqrt()), float(z[1].pow(2).mean().sqrt())))


@pytest.mark.parametrize("B", [5, 65])
def test_fp32_restatement_has_headroom(B):
    """the fp32 torch restatement sits under a quarter of each GPU bar on the GPU test's rows"""
    P = T.pool()
    worst = 0.0
    for with_drop in (False, True):
        for last_only in (False, True):
            feat, drop, gt = T.case(B, with_drop, last_only)
            want, want_f = T.autograd_grads(P["flat"], feat, drop, gt)
            got, got_f = T.autograd_grads(P["flat"], feat, drop, gt, dtype=torch.float32)
            errs = T.per_tensor_errors(got, want, got_f, want_f)
            key, e = max(errs, key=lambda t: t[1])
            print("B=%d drop=%d last_only=%d: worst %.3g (%s)" % (B, with_drop, last_only, e, key))
            worst = max(worst, e)
        th64, th32 = T.forward(P["flat"], feat, drop), T.forward(P["flat"], feat, drop, dtype=torch.float32)
        r = float((np.abs(th32 - th64).reshape(-1, 85).max(1) / np.abs(th64).reshape(-1, 85).max(1)).max())
        print("B=%d drop=%d forward rel per image %.3g" % (B, with_drop, r))
        assert r <= FWD_BAR / 4
    assert worst <= GPU_BAR / 4
