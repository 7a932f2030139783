"""The fp32 fused stem on the bf16 matrix cores (stem_fused_f32s_kernel), through debug_stem: against float64 on inputs with 24 binades
of dynamic range, and bit for bit against itself across strip heights (the passes a tall strip is walked in, the conv row kept in
registers between them, the restage), batch positions and a device parameter update."""
import numpy as np
import pytest
import torch

import hpe_amd
import stem_split_ref as R
from hpe_amd import resnet_spec, synthetic

pytestmark = pytest.mark.gpu
B = 3


def make_engine(params, reserve=0):
    e = hpe_amd.HpeEngine(device=0, max_batch=B)
    e.load_encoder(params)
    e.finalize()
    if reserve:
        e.reserve_encoder_train(reserve)
    return e


@pytest.fixture(scope="module")
def params():
    return synthetic.make_encoder_params()


@pytest.fixture(scope="module")
def engine(params):
    e = make_engine(params, reserve=1)
    yield e
    e.close()


@pytest.fixture(scope="module")
def images():
    return R.dynamic_range_images(B)


@pytest.fixture(scope="module")
def ref64(images, params):
    return R.reference_fp64(images, params)


@pytest.fixture(scope="module")
def outputs(engine, images):
    """the stem output per strip height, computed once"""
    x = torch.from_numpy(images).cuda()
    return {r: engine.debug_stem(x, rows_per_strip=r).cpu() for r in (1, 2, 4, 7, 8)}


@pytest.mark.parametrize("rows", [1, 4, 8])
def test_dynamic_range_against_fp64(outputs, ref64, rows):
    y = outputs[rows].numpy()
    assert y.shape == ref64.shape == (B, 56, 56, 64)
    err = R.rel(y, ref64)
    print("R = %d: %.3g against fp64 (bar %.3g)" % (rows, err, R.BAR))
    assert err < R.BAR


@pytest.mark.parametrize("rows", [2, 4, 7, 8])
def test_strip_height_does_not_change_a_bit(outputs, rows):
    assert torch.equal(outputs[rows], outputs[1])


@pytest.mark.parametrize("rows", [0, 8])
def test_batch_position_does_not_change_a_bit(engine, images, outputs, rows):
    x = torch.from_numpy(images).cuda()
    want = outputs[8] if rows else engine.debug_stem(x).cpu()
    for i in range(B):
        alone = engine.debug_stem(x[i:i + 1].contiguous(), rows_per_strip=rows).cpu()
        assert torch.equal(alone[0], want[i]), i


def test_parameter_update_on_the_device(engine, params, images):
    """after set_encoder_params_dev the stem computes what a fresh context built from those values computes (runs last: it leaves the
    module's engine with the new weights)"""
    x = torch.from_numpy(images).cuda()
    p = torch.from_numpy(resnet_spec.params_to_flat(params))
    d = torch.randn(p.shape, generator=torch.Generator().manual_seed(5))
    q = p + d * (1e-2 * float(p.norm()) / float(d.norm()))
    before = engine.debug_stem(x, rows_per_strip=8).cpu()
    engine.set_encoder_params_dev(q.cuda())
    got = engine.debug_stem(x, rows_per_strip=8).cpu()
    fresh = make_engine(resnet_spec.flat_to_params(q, params))
    try:
        want = fresh.debug_stem(x, rows_per_strip=8).cpu()
    finally:
        fresh.close()
    assert torch.equal(got, want) and not torch.equal(got, before)
