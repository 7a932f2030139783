"""GPU tests of the split-bf16 fp32 GEMM (conv_gemm_f32s.hip, plan option f32_split): every 1x1 / strided layer of stages 2-5 against an
fp64 reference next to the fp32-MFMA kernel on the same inputs, at batches where the split kernel runs on whole and partial last tiles;
the whole encoder (dual-source launches included) against the fp32-MFMA plan, and bitwise repeatability."""
import os

import numpy as np
import pytest
import torch

import hpe_amd
from hpe_amd import resnet_spec, synthetic

pytestmark = pytest.mark.gpu

ONE_BY_ONE = [s.name for s in resnet_spec.CONV_SPECS if s.kh == 1 and s.name.startswith("res")]
# B = 37: partial last tiles everywhere; B = 128: the chunk size of the B = 256 step (stage 2, off by default, at B = 37 only)
CASES = [(n, 37) for n in ONE_BY_ONE] + [(n, 128) for n in ONE_BY_ONE if not n.startswith("res2")]


def _engine(enc, max_batch, f32_split, min_tiles=None):
    """encoder-only fp32 context; min_tiles: HPE_F32S_MIN_TILES while the context is finalised (the split kernel on every grid size)"""
    old = os.environ.get("HPE_F32S_MIN_TILES")
    if min_tiles is not None:
        os.environ["HPE_F32S_MIN_TILES"] = str(min_tiles)
    try:
        e = hpe_amd.HpeEngine(device=0, max_batch=max_batch, f32_split=f32_split)
        e.load_encoder(enc)
        e.finalize()
    finally:
        if min_tiles is not None:
            if old is None:
                del os.environ["HPE_F32S_MIN_TILES"]
            else:
                os.environ["HPE_F32S_MIN_TILES"] = old
    return e


@pytest.fixture(scope="module")
def enc():
    return synthetic.make_encoder_params()


@pytest.fixture(scope="module")
def engines(enc):
    made = (_engine(enc, 128, 0), _engine(enc, 128, 15, min_tiles=1))
    yield made
    for e in made:
        e.close()


def _bn_fold(p, s, eps=1e-3):
    g, b = p[s.bn_name + "/gamma"].astype(np.float64), p[s.bn_name + "/beta"].astype(np.float64)
    m, v = p[s.bn_name + "/moving_mean"].astype(np.float64), p[s.bn_name + "/moving_variance"].astype(np.float64)
    return g / np.sqrt(v + eps), b - m * g / np.sqrt(v + eps)


def _inputs(s, B, seed):
    """N(0,1) activations with a wide dynamic range: rows scaled over 2^-12 .. 2^12, a third of the values exact zeros (post-ReLU)"""
    g = np.random.Generator(np.random.Philox(seed))
    x = g.normal(0, 1, (B, s.hin, s.hin, s.cin))
    x *= np.exp2(g.integers(-12, 13, (B, s.hin, s.hin, 1)))
    x[g.random(x.shape) < 0.33] = 0.0
    res = g.normal(0, 1, (B, s.hout, s.hout, s.cout)).astype(np.float32) if s.name.endswith("2c") else None
    return x.astype(np.float32), res


def _ref(enc, s, x, res):
    xs = x[:, :: s.stride, :: s.stride, :].astype(np.float64).reshape(-1, s.cin)
    w = enc[s.name + "/kernel"].astype(np.float64).reshape(s.cin, s.cout)
    y = torch.from_numpy(xs) @ torch.from_numpy(w)
    y = y.numpy() + enc[s.name + "/bias"].astype(np.float64)
    sc, sh = _bn_fold(enc, s)
    y = y * sc + sh
    if res is not None:
        y = y + res.reshape(-1, s.cout)
    return np.maximum(y, 0).reshape(x.shape[0], s.hout, s.hout, s.cout)


@pytest.mark.parametrize("name,B", CASES)
def test_split_layer_error_matches_fp32_kernel(engines, enc, name, B):
    """max|y - ref| / max|ref| of the split kernel <= 1.5 x that of the fp32-MFMA kernel (+ 2^-26 slack for the layers where both are
    near zero) and < 5e-6, on the same inputs; both columns are printed"""
    idx = resnet_spec.CONV_INDEX[name]
    s = resnet_spec.CONV_SPECS[idx]
    x, res = _inputs(s, B, 1000 + 7 * idx + B)
    ref = _ref(enc, s, x, res)
    scale = np.abs(ref).max()
    errs = []
    for e in engines:
        y = e.debug_conv(idx, torch.from_numpy(x).cuda(), residual=None if res is None else torch.from_numpy(res).cuda(), relu=True)
        torch.cuda.synchronize()
        errs.append(float(np.abs(y.cpu().numpy().astype(np.float64) - ref).max() / scale))
    print("f32_split %-16s B=%3d  fp32 MFMA %.3e  split bf16 %.3e  ratio %.2f" % (name, B, errs[0], errs[1], errs[1] / max(errs[0], 1e-30)))
    assert errs[1] < 5e-6, (name, B, errs)
    assert errs[1] <= 1.5 * errs[0] + 2.0 ** -26, (name, B, errs)


def test_split_encoder_matches_fp32_plan_and_is_repeatable(enc):
    """the whole encoder at B = 128 (dual-source launches included, default launch-size rules) against the fp32-MFMA plan, and bitwise
    equal across two runs"""
    B = 128
    base, split = _engine(enc, B, 0), _engine(enc, B, 15)
    try:
        img = torch.from_numpy(synthetic.make_images(B, seed=31)).cuda()
        f0 = base.encoder(img).cpu().numpy().astype(np.float64)
        f1 = split.encoder(img).cpu().numpy()
        f2 = split.encoder(img).cpu().numpy()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(f1, f2)
        err = float(np.abs(f1 - f0).max() / np.abs(f0).max())
        print("f32_split encoder B=%d: max rel diff to the fp32-MFMA plan %.3e" % (B, err))
        assert err < 2e-5, err
    finally:
        base.close()
        split.close()
