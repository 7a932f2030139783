"""The arithmetic of the split-bf16 fused stem, on the CPU: the packing of its weights and the model of its products and accumulators
(stem_split_ref.py) against float64 on the inputs the GPU test uses -- the arithmetic itself has to meet the per-kernel bar, and by a
margin, before any kernel runs."""
import numpy as np
import pytest

import stem_split_ref as R
from hpe_amd import synthetic
from oracle import hmr_oracle as O


@pytest.fixture(scope="module")
def params():
    return synthetic.make_encoder_params()


@pytest.fixture(scope="module")
def images():
    return R.dynamic_range_images()


@pytest.fixture(scope="module")
def ref64(images, params):
    return R.reference_fp64(images, params)


def test_inputs_are_what_they_claim(images):
    px = images.reshape(-1, 3)
    zero = np.all(px == 0, axis=1)
    assert 0.30 < zero.mean() < 0.36
    mag = np.abs(px[~zero])
    assert mag.max() > 2.0 ** 10 and np.median(mag[mag > 0]) < 1.0 and mag[mag > 0].min() < 2.0 ** -12
    assert np.all(images[0, :5] == 1.0) and np.all(images[1, :, :4] == -1.0)


def test_split_is_exact_and_ordered(images, params):
    for x in (images, params[R.S.name + "/kernel"], np.float32([0.0, -0.0, 1.0, -1.0, 3.0e38, np.pi * 2.0 ** -100, np.pi, 1 + 2.0 ** -23])):
        h = R.split3(x)
        v = R.bf16_value(h).astype(np.float64)
        assert np.array_equal((v[0] + v[1] + v[2]).astype(np.float32), np.asarray(x, np.float32))
        assert np.array_equal(v[0] + v[1] + v[2], np.asarray(x, np.float64))  # no rounding hidden in the sum
        nz = v[0] != 0
        assert np.all(np.abs(v[1][nz]) <= np.abs(v[0][nz]) * 2.0 ** -8) and np.all(np.abs(v[2][nz]) <= np.abs(v[0][nz]) * 2.0 ** -16)


def test_packing(params):
    k = params[R.S.name + "/kernel"]
    wt, ws = R.pack_weights(k)
    assert wt.shape == (64, 7, 32) and ws.shape == (3, 64, 7, 32) and ws.dtype == np.uint16
    v = R.bf16_value(ws).astype(np.float64)
    assert np.array_equal(v[0] + v[1] + v[2], wt.astype(np.float64))  # w0 + w1 + w2 == w, every packed weight
    assert np.array_equal(ws[0], R.bf16_round(wt))
    w6 = ws.reshape(3, 64, 7, 8, 4)
    assert not w6[:, :, :, 7, :].any() and not w6[:, :, :, :, 3].any()  # eighth pixel, pad channel
    for n, kh, kw, ci in ((0, 0, 0, 0), (63, 6, 6, 2), (17, 3, 5, 1)):
        assert wt[n, kh, kw * 4 + ci] == k[kh, kw, ci, n]
    assert np.count_nonzero(wt) == np.count_nonzero(k)


def test_reference_is_the_oracles_layer(images, params, ref64):
    lin = O.conv2d_nhwc(images[:1], params[R.S.name + "/kernel"], params[R.S.name + "/bias"], 2, 3, dtype=np.float64)
    g, b = params[R.S.bn_name + "/gamma"].astype(np.float64), params[R.S.bn_name + "/beta"].astype(np.float64)
    m, v = params[R.S.bn_name + "/moving_mean"].astype(np.float64), params[R.S.bn_name + "/moving_variance"].astype(np.float64)
    sc = g / np.sqrt(v + 1e-3)
    want = R.max_pool(np.maximum(lin * sc + (b - m * sc), 0))
    assert R.rel(ref64[:1], want) < 1e-13


def test_model_meets_the_bar(images, params, ref64):
    y = R.model_fp32(images, params)
    assert y.dtype == np.float32 and y.shape == ref64.shape == (3, 56, 56, 64)
    err = R.rel(y, ref64)
    print("split-bf16 stem model against fp64: %.3g, bar %.3g, margin %.1fx" % (err, R.BAR, R.BAR / err))
    assert err < R.BAR
    # the products the split drops (a1 w2, a2 w1, a2 w2) are below 2^-25 of |a w|: without the rounding of the accumulators the six
    # kept ones reproduce the layer far inside the bar
    a = [R.windows(R.bf16_value(h)).astype(np.float64) for h in R.split3(images[:1])]
    w = [R.bf16_value(h).astype(np.float64) for h in R.pack_weights(params[R.S.name + "/kernel"])[1]]
    kept = sum(np.einsum("bhwrk,nrk->bhwn", a[i], w[j]) for i, j in R.CROSS + ((0, 0),))
    full = np.einsum("bhwrk,nrk->bhwn", a[0] + a[1] + a[2], w[0] + w[1] + w[2])
    assert R.rel(kept, full) < 2.0 ** -24
