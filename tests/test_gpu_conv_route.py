"""hpe_debug_conv_route against what a context really holds and launches: the pack mask of the pure rule against the buffers hpe_finalize
allocated, and the kernel a route names against the output of the launch (a wrong route that still launched would compute with the other
kernel's rounding, a route whose packing is missing is refused by run_conv)."""
import pytest
import torch

import hpe_amd
from hpe_amd import _lib, synthetic
from hpe_amd.resnet_spec import CONV_INDEX, CONV_SPECS

pytestmark = pytest.mark.gpu
PACKINGS = _lib.ENCODER_PACKINGS
FORMS = ("w_split", "wino_u", "wino4_u", "stem_w", "w_dual", "w_dual_split")
PLANS = {"A": {}, "B": {"f32_split": 15, "wino_f4": 15}, "C": {"f32_split": 0, "wino_f4": 0, "dual_gemm": 0}}  # those of test_gpu_encoder_repack.py


@pytest.fixture(scope="module")
def enc():
    return synthetic.make_encoder_params()


def encoder_engine(enc, max_batch, **kw):
    e = hpe_amd.HpeEngine(device=0, max_batch=max_batch, **kw)
    e.load_encoder(enc)
    e.finalize()
    return e


@pytest.mark.parametrize("plan", sorted(PLANS))
def test_pack_mask_is_what_finalize_allocated(enc, plan):
    e = encoder_engine(enc, 2, **PLANS[plan])
    try:
        held = set()
        for i in range(len(CONV_SPECS)):
            mask = e.conv_route(i, 2).packs
            for name in FORMS:
                w = PACKINGS.index(name)
                n = e.lib.hpe_debug_encoder_packing_bytes(e._h, i, w)
                assert (n > 0) == bool(mask >> w & 1), (CONV_SPECS[i].name, name, n, mask)
                held |= {name} if n else set()
            assert not mask & ~sum(1 << PACKINGS.index(n) for n in FORMS)
        assert held == (set(FORMS) if plan != "C" else {"wino_u", "stem_w"}), held
    finally:
        e.close()


MAXB = 37
GEMM_ONLY = dict(wino_min_c=0, halo3=0)
LAYERS = ("res2b_branch2b", "res3b_branch2b", "res5b_branch2b", "res3a_branch2c", "res2b_branch2c")
# the kernel of the default plan, from the rules: bf16 3x3 layers take halo3 at every batch.  fp32 3x3 layers need wino_min_items = 128
# work items (F(4x4): min(128, wino4_min_items = 64) 32-tile x 32-cout workgroups): at B = 37 res2b (56x56, fused F(2x2), 2 tile rows a
# workgroup) has 37 * 28 / 2 = 518, res3b (28x28, F(4x4)) ceil(37 * 49 / 32) * 4 = 232, res5b (7x7, F(4x4)) ceil(37 * 4 / 32) * 16 = 80;
# at B = 3 they have 42, 20 and 16 and stay on the direct kernel.  The 1x1 layers are GEMMs under both plans.
DEFAULT_KERNEL = {
    ("fp32", "res2b_branch2b", 37): "wino_fused", ("fp32", "res3b_branch2b", 37): "wino4", ("fp32", "res5b_branch2b", 37): "wino4",
    ("bf16", "res2b_branch2b", 3): "halo3", ("bf16", "res3b_branch2b", 3): "halo3", ("bf16", "res5b_branch2b", 3): "halo3",
    ("bf16", "res2b_branch2b", 37): "halo3", ("bf16", "res3b_branch2b", 37): "halo3", ("bf16", "res5b_branch2b", 37): "halo3",
}
GEMMS = {"fp32": ("f32", "f32s"), "bf16": ("bf16",)}
# test_winograd4_conv_matches_oracle holds F(4x4) to 5e-5 of the layer's largest output (the direct kernel: 5e-6),
# test_bf16_halo3_layer_matches_oracle holds the two bf16 kernels to one bf16 ulp of each other
TOL = {"fp32": 5e-5, "bf16": 2.0 ** -8}


@pytest.fixture(scope="module")
def engines(enc):
    made = {(dt, gemm): encoder_engine(enc, MAXB, encoder_dtype=dt, **(GEMM_ONLY if gemm else {})) for dt in ("fp32", "bf16") for gemm in (False, True)}
    yield made
    for e in made.values():
        e.close()


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


@pytest.mark.parametrize("B", [3, 37])
@pytest.mark.parametrize("name", LAYERS)
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_route_names_the_kernel_that_ran(engines, dt, name, B):
    idx = CONV_INDEX[name]
    s = CONV_SPECS[idx]
    dflt, gemm = engines[(dt, False)], engines[(dt, True)]
    is2c = name.endswith("2c")
    g = torch.Generator().manual_seed(4100 + idx + B)
    x = torch.randn((B, s.hin, s.hin, s.cin), generator=g)
    x[torch.rand(x.shape, generator=g) < 0.3] = 0.0  # post-ReLU sparsity
    x[0, 0, 0, :] = 20.0  # a corner pixel: only 4 of the 9 taps see it
    x = x.cuda()
    res = torch.randn((B, s.hout, s.hout, s.cout), generator=g).cuda() if is2c else None
    routes = [e.conv_route(idx, B, residual=is2c) for e in (dflt, gemm)]
    kernels = [_lib.CONV_KERNELS[r.kernel] for r in routes]
    assert kernels[1] in GEMMS[dt] and routes[1].in_slab8 == 0, kernels
    assert kernels[0] == DEFAULT_KERNEL.get((dt, name, B), kernels[0] if kernels[0] in GEMMS[dt] else None), kernels
    assert routes[0].in_slab8 == (kernels[0] == "wino_fused")
    assert routes[0].join == routes[1].join and (is2c or routes[0].join == 0)
    if routes[0].join == 2:  # chained with the next block's branch2a in the network: that launch
        out = [torch.cat([t.reshape(B, -1) for t in e.debug_chain(idx, x, res)[:2]], 1) for e in (dflt, gemm)]
    else:
        out = [e.debug_conv(idx, x, residual=res, relu=True) for e in (dflt, gemm)]
    err = rel(out[0], out[1])
    print("%s %s B=%d: %s against %s, join %d: rel %.3g" % (dt, name, B, kernels[0], kernels[1], routes[0].join, err))
    assert err < TOL[dt], err
    if kernels[0] != kernels[1] and dt == "fp32":
        assert not torch.equal(out[0], out[1])  # Winograd arithmetic shows in fp32 (bf16 outputs may round to the same values: res2b does)
