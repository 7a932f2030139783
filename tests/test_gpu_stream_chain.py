"""The chained forms of the streaming split-bf16 kernel (conv_stream_chain_f32s.hip, bits 4 and 8 of HPE_STREAM1X1): form 3, res2b_branch2c
+ residual + ReLU chained with res2c_branch2a, and form 4, the dual-source launch of res2a chained with res2b_branch2a -- through
debug_stream_chain against float64 next to the launches they replace (debug_chain; debug_dual then debug_conv), and bit for bit across
layouts, grid sizes, launches, batch positions and a device parameter update.

Tiles are 32 rows and a 56x56 map is 98 of them: B = 1 and B = 3 (98 and 294 tiles) are the smallest launches there are."""
import numpy as np
import pytest
import torch

import hpe_amd
import stream_chain_ref as R
import test_gpu_stream1x1 as S
from hpe_amd import resnet_spec, synthetic

pytestmark = pytest.mark.gpu

FORMS = {"res2b_branch2c": 3, "res2a_branch2c": 4}
FORCED = {"HPE_STREAM1X1": "15", "HPE_STREAM1X1_MIN_M": "1"}
OFF = {"HPE_STREAM1X1": "0"}  # the fp32-MFMA launches: conv_chain_f32.hip, the dual-source GEMM, res2b_branch2a's GEMM


def make_engine(params, env, reserve=0, max_batch=3):
    with S.environment(env):
        e = hpe_amd.HpeEngine(device=0, max_batch=max_batch)
        e.load_encoder(params)
        e.finalize()
        if reserve:
            e.reserve_encoder_train(reserve)
    return e


@pytest.fixture(scope="module")
def params():
    return synthetic.make_encoder_params()


@pytest.fixture(scope="module")
def engines(params):
    made = {"off": make_engine(params, OFF), "on": make_engine(params, FORCED)}
    yield made
    for e in made.values():
        e.close()


def chain_inputs(name, B):
    """(t2, x): x the residual [B,56,56,256] of res2b, or the block input [B,56,56,64] of res2a -- the shared inputs of test_gpu_stream1x1.py"""
    return S.dual_inputs(B) if FORMS[name] == 4 else S.inputs(name, B)


def gpu(a):
    return torch.from_numpy(np.array(a)).cuda()


_ref, _new, _old = {}, {}, {}


def reference_fp64(params, name, B):
    """t3 as test_gpu_stream1x1.py's float64 references have it, u1 = relu(bn(W2a' t3 + b)) of that in float64"""
    if (name, B) not in _ref:
        t3 = S.dual_reference_fp64(params, B) if FORMS[name] == 4 else S.reference_fp64(params, name, B)
        i2c = resnet_spec.CONV_INDEX[name]
        sn = resnet_spec.CONV_SPECS[i2c + (2 if FORMS[name] == 4 else 1)]
        sc, sh = S.bn_fold(params, sn)
        u1 = torch.from_numpy(t3.reshape(-1, sn.cin)) @ torch.from_numpy(params[sn.name + "/kernel"].astype(np.float64).reshape(sn.cin, sn.cout))
        u1 = np.maximum((u1.numpy() + params[sn.name + "/bias"].astype(np.float64)) * sc + sh, 0).reshape(B, 56, 56, sn.cout)
        _ref[(name, B)] = (t3, u1)
    return _ref[(name, B)]


def run(e, name, B, t2=None, x=None, **kw):
    if t2 is None:
        t2, x = (gpu(a) for a in chain_inputs(name, B))
    t3, u1 = e.debug_stream_chain(resnet_spec.CONV_INDEX[name], t2, x, **kw)
    return t3.cpu(), u1.cpu()


def chained(engines, name, B):
    """the forced launch on the default grid, NHWC u1, computed once and shared"""
    if (name, B) not in _new:
        _new[(name, B)] = run(engines["on"], name, B)
    return _new[(name, B)]


def replaced(engines, name, B):
    """the launches the form replaces, on the fp32-MFMA plan: debug_chain; debug_dual then debug_conv of res2b_branch2a"""
    if (name, B) not in _old:
        e, i2c = engines["off"], resnet_spec.CONV_INDEX[name]
        t2, x = (gpu(a) for a in chain_inputs(name, B))
        if FORMS[name] == 3:
            t3, u1, _ = e.debug_chain(i2c, t2, x)
        else:
            t3 = e.debug_dual(i2c, t2, x)
            u1 = e.debug_conv(i2c + 2, t3, relu=True)
        _old[(name, B)] = (t3.cpu(), u1.cpu())
    return _old[(name, B)]


def err(got, ref):
    return float(np.abs(got.numpy().astype(np.float64) - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize("name,B", [(n, B) for n in FORMS for B in (1, 3)])
def test_error_against_fp64_next_to_the_replaced_launches(engines, params, name, B):
    """t3 and u1: max|y - fp64| / max|fp64| <= 5e-6 and <= 1.5 x the replaced fp32 launches' on the same inputs + 2^-26 (the bars of
    test_gpu_f32_split.py and test_gpu_stream1x1.py); both columns are printed"""
    ref, new, old = reference_fp64(params, name, B), chained(engines, name, B), replaced(engines, name, B)
    figures = []
    for what, r, n, o in zip(("t3", "u1"), ref, new, old):
        e_old, e_new = err(o, r), err(n, r)
        print("stream chain form %d %-15s B=%d %s  replaced fp32 %.3e  chained split bf16 %.3e  ratio %.2f" % (FORMS[name], name, B, what, e_old, e_new, e_new / max(e_old, 1e-30)))
        figures.append((what, e_old, e_new))
    for what, e_old, e_new in figures:
        assert e_new <= 5e-6, (name, B, what, e_old, e_new)
        assert e_new <= 1.5 * e_old + 2.0 ** -26, (name, B, what, e_old, e_new)


@pytest.mark.parametrize("name,B", [(n, B) for n in FORMS for B in (1, 3)])
def test_matches_the_replaced_launches(engines, name, B):
    """rel <= 2e-6 on t3 and u1, the bar between the chained and the unchained results of test_f32_chain_matches_oracle_and_two_launches"""
    for what, n, o in zip(("t3", "u1"), chained(engines, name, B), replaced(engines, name, B)):
        rel = float(np.abs(n.numpy().astype(np.float64) - o.numpy()).max() / (np.abs(o.numpy()).max() + 1e-30))
        print("stream chain form %d B=%d %s rel to the replaced launches %.3e" % (FORMS[name], B, what, rel))
        assert rel <= 2e-6, (name, B, what, rel)


@pytest.mark.parametrize("name", list(FORMS))
def test_slab8_is_the_row_major_result_permuted(engines, name):
    for B in (1, 3):
        t3, u1 = chained(engines, name, B)
        t3s, u1s = run(engines["on"], name, B, slab8=True)
        assert torch.equal(t3s, t3), (name, B)
        assert np.array_equal(u1s.numpy(), R.to_slab8(u1.numpy().reshape(-1, 64))), (name, B)


@pytest.mark.parametrize("walkers", [1, 8])
def test_walk_does_not_change_a_bit(engines, params, walkers):
    """the grid capped to one workgroup (it walks all 98 / 294 tiles) and to 8 (which divides neither): bit for bit the uncapped launch"""
    e = make_engine(params, dict(FORCED, HPE_STREAM1X1_WALKERS=str(walkers)))
    try:
        for name in FORMS:
            for B in (1, 3):
                for slab8 in (False, True):
                    want = chained(engines, name, B) if not slab8 else run(engines["on"], name, B, slab8=True)
                    got = run(e, name, B, slab8=slab8)
                    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (name, B, walkers, slab8)
    finally:
        e.close()


@pytest.mark.parametrize("name", list(FORMS))
def test_repeatable_and_batch_position_does_not_change_a_bit(engines, name):
    t2, x = (gpu(a) for a in chain_inputs(name, 3))
    t3, u1 = chained(engines, name, 3)
    for rep in range(5):
        a, b = run(engines["on"], name, 3)
        assert torch.equal(a, t3) and torch.equal(b, u1), rep
    a, b = run(engines["on"], name, 1, t2[1:2].contiguous(), x[1:2].contiguous())
    assert torch.equal(a[0], t3[1]) and torch.equal(b[0], u1[1])


def test_parameter_update_on_the_device(params):
    """after set_encoder_params_dev the launches compute, bit for bit, what a fresh context built from those values computes: the kernel
    splits the fp32 weights the device update rewrites (res2b_branch2c, the folded dual weights of res2a, res2b_branch2a, res2c_branch2a)"""
    engine = make_engine(params, FORCED, reserve=1)
    p = torch.from_numpy(resnet_spec.params_to_flat(params))
    d = torch.randn(p.shape, generator=torch.Generator().manual_seed(6))
    q = p + d * (1e-2 * float(p.norm()) / float(d.norm()))
    fresh = make_engine(resnet_spec.flat_to_params(q, params), FORCED)
    try:
        before = {n: run(engine, n, 1) for n in FORMS}
        engine.set_encoder_params_dev(q.cuda())
        got = {n: run(engine, n, 1) for n in FORMS}
        want = {n: run(fresh, n, 1) for n in FORMS}
    finally:
        engine.close()
        fresh.close()
    for n in FORMS:
        for i in range(2):
            assert torch.equal(got[n][i], want[n][i]) and not torch.equal(got[n][i], before[n][i]), (n, i)


def test_encoder_with_the_forms_matches_the_plan_without_and_is_repeatable(params):
    """the whole encoder at B = 8, the smallest batch the default launch-size bar lets through, with HPE_STREAM1X1=15 against =3: feature
    rel < 5e-6 (the bar of the plan-against-plan comparisons), five repeats bitwise equal"""
    idx = {n: resnet_spec.CONV_INDEX[n] for n in FORMS}
    base, on = make_engine(params, {"HPE_STREAM1X1": "3"}, max_batch=8), make_engine(params, {"HPE_STREAM1X1": "15"}, max_batch=8)
    try:
        # what hpe_debug_conv_route answers does not move with the new bits
        for n, i in idx.items():
            ra, rb = base.conv_route(i, 8, residual=FORMS[n] == 3), on.conv_route(i, 8, residual=FORMS[n] == 3)
            assert (ra.kernel, ra.tile, ra.join, ra.join_kernel, ra.join_tile, ra.next_slab8) == (rb.kernel, rb.tile, rb.join, rb.join_kernel, rb.join_tile, rb.next_slab8)
            assert rb.join == (2 if FORMS[n] == 3 else 1)
        img = torch.from_numpy(synthetic.make_images(8, seed=33)).cuda()
        f0 = base.encoder(img).cpu().numpy().astype(np.float64)
        f1 = on.encoder(img).cpu().numpy()
        for rep in range(5):
            np.testing.assert_array_equal(on.encoder(img).cpu().numpy(), f1)
        rel = float(np.abs(f1 - f0).max() / np.abs(f0).max())
        print("stream chain encoder B=8: max rel diff to HPE_STREAM1X1=3 %.3e" % rel)
        assert rel < 5e-6, rel
        assert not np.array_equal(f1, f0.astype(np.float32))  # the other arithmetic ran
    finally:
        base.close()
        on.close()


def test_launcher_refuses_partial_tiles_and_other_geometry(engines):
    """a row count that is no multiple of 32, rows past the batch and every layer but the two stage-2 joins: the error code comes back and
    nothing is launched (outputs filled with a mark keep it); a whole number of tiles short of the map is the same result, cut"""
    e = engines["on"]
    t2, x = (gpu(a) for a in chain_inputs("res2b_branch2c", 1))
    i2c = resnet_spec.CONV_INDEX["res2b_branch2c"]
    t3 = torch.full((1, 56, 56, 256), -7.0, device="cuda")
    u1 = torch.full((1, 56, 56, 64), -7.0, device="cuda")

    def call(idx, rows):
        return e.lib.hpe_debug_stream_chain(e._h, idx, t2.data_ptr(), x.data_ptr(), 1, t3.data_ptr(), u1.data_ptr(), 0, rows, None)

    for rows in (100, 31, 3136 - 16, 3136 + 32, -32):
        assert call(i2c, rows) != 0, rows
    for other in ("res2c_branch2c", "res3b_branch2c", "res2b_branch2a"):
        assert call(resnet_spec.CONV_INDEX[other], 0) != 0, other
    torch.cuda.synchronize()
    assert bool((t3 == -7.0).all()) and bool((u1 == -7.0).all())
    with pytest.raises(hpe_amd._lib.HpeError):
        e.debug_stream_chain(i2c, t2, x, rows=100)
    assert call(i2c, 64) == 0
    full = chained(engines, "res2b_branch2c", 1)
    t3, u1 = t3.cpu().reshape(-1, 256), u1.cpu().reshape(-1, 64)
    assert torch.equal(t3[:64], full[0].reshape(-1, 256)[:64]) and bool((t3[64:] == -7.0).all())
    assert torch.equal(u1[:64], full[1].reshape(-1, 64)[:64]) and bool((u1[64:] == -7.0).all())
