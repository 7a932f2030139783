"""The conv dispatch (route_conv / route_block / layer_packs of csrc/hpe_plan.hip) through hpe_debug_conv_route against its restatement
tests/route_ref.py: every layer, both dtypes, every query flag, batches on both sides of every threshold, nine option sets.  No GPU, no
context."""
import ctypes as C
import itertools

import pytest

import route_ref as R
from hpe_amd import _lib, build as hbuild
from hpe_amd.resnet_spec import CONV_INDEX, CONV_SPECS

BATCHES = (1, 2, 4, 8, 16, 31, 32, 37, 64, 100, 128, 256)
OPTION_SETS = {
    "defaults": {}, "wino_min_c=0": dict(wino_min_c=0), "wino_f4=0": dict(wino_f4=0), "wino4_fused=12": dict(wino4_fused=12),
    "wino_fused=0": dict(wino_fused=0), "dual_gemm=0": dict(dual_gemm=0), "chain_fuse=0": dict(chain_fuse=0), "chain_fuse=23": dict(chain_fuse=23),
    "halo3=0,bf16_p8=31": dict(halo3=0, bf16_p8=31), "f32_split=0": dict(f32_split=0), "f32_split=15": dict(f32_split=15),
}
FIELDS = ("kernel", "mode", "tile", "in_slab8", "out_slab8")


@pytest.fixture(scope="module")
def lib():
    hbuild.build()
    return _lib.load()


@pytest.fixture(autouse=True)
def no_plan_environment(monkeypatch):
    import os

    for k in [k for k in os.environ if k.startswith("HPE_")]:
        monkeypatch.delenv(k)


def config(lib, bf16, opts):
    cfg = _lib.HpeConfig()
    lib.hpe_config_init(C.byref(cfg))
    cfg.encoder_dtype = int(bf16)
    for k, v in opts.items():
        setattr(cfg, k, v)
    return cfg


def asked(lib, cfg, idx, B, concurrent, residual, workspace):
    r = _lib.conv_route(lib, cfg, idx, B, concurrent, residual, workspace)
    assert r.reserved == 0
    return r


def as_dict(r):
    return dict(kernel=_lib.CONV_KERNELS[r.kernel], mode=r.mode, tile=r.tile, in_slab8=bool(r.in_slab8), out_slab8=bool(r.out_slab8))


def sweep(lib, bf16, opts):
    """the network's launches of every swept case: yields (case, {idx: HpeConvRoute}, {idx: restated launch}); residual as the network
    passes it (the branch2c layers)"""
    cfg, pl = config(lib, bf16, opts), R.resolve_plan(bf16, **opts)
    i2c = {blk[5] for blk in R.BLOCKS}
    for B, concurrent, workspace in itertools.product(BATCHES, (False, True), (False, True)):
        got = {i: asked(lib, cfg, i, B, concurrent, i in i2c, workspace) for i in range(len(CONV_SPECS))}
        yield (bf16, B, concurrent, workspace), got, R.chunk_launches(pl, bf16, B, concurrent, workspace)


@pytest.fixture(scope="module")
def swept(lib):
    """{(option set, bf16): [cases]}, computed once"""
    return {(name, bf16): list(sweep(lib, bf16, opts)) for name, opts in OPTION_SETS.items() for bf16 in (False, True)}


def test_network_routes_match_the_restatement(swept):
    bad = []
    for (name, _), cases in swept.items():
        for case, got, ref in cases:
            for idx, want in ref.items():
                g = got[idx]
                if "join" not in want or want["join"] == "separate":
                    have = as_dict(g)
                    if any(have[f] != want[f] for f in FIELDS):
                        bad.append((name, case, CONV_SPECS[idx].name, have, want))
                if "join" in want:
                    have = (_lib.BLOCK_JOINS[g.join], _lib.CONV_KERNELS[g.join_kernel] if g.join == 1 else None, g.join_tile, bool(g.next_slab8))
                    exp = (want["join"], want.get("kernel") if want["join"] == "dual" else None, want["tile"] if want["join"] == "dual" else -1,
                           bool(want.get("next_slab8")))
                    if have != exp:
                        bad.append((name, case, CONV_SPECS[idx].name, have, exp))
                elif (g.join, g.join_kernel, g.join_tile, g.next_slab8) != (0, -1, -1, 0):
                    bad.append((name, case, CONV_SPECS[idx].name, "join fields of a layer that is no branch2c"))
    assert not bad, (len(bad), bad[:5])


def test_single_layer_routes_match_the_restatement(lib):
    """what hpe_debug_conv and the training forward launch: the layer alone, NHWC input, with and without a residual"""
    bad = []
    for name, opts in OPTION_SETS.items():
        for bf16 in (False, True):
            cfg, pl = config(lib, bf16, opts), R.resolve_plan(bf16, **opts)
            for idx, B, res in itertools.product(range(len(CONV_SPECS)), BATCHES, (False, True)):
                have, want = as_dict(asked(lib, cfg, idx, B, False, res, True)), R.debug_conv(pl, bf16, idx, B, res)
                if any(have[f] != want[f] for f in FIELDS[:4]):
                    bad.append((name, bf16, CONV_SPECS[idx].name, B, res, have, want))
    assert not bad, (len(bad), bad[:5])


def reached(cases):
    out = set()
    for _, got, ref in cases:
        out |= {_lib.CONV_KERNELS[got[i].kernel] for i, w in ref.items() if w.get("join", "separate") == "separate"}
        out |= {_lib.CONV_KERNELS[got[i].join_kernel] for i, w in ref.items() if w.get("join") == "dual"}
    return out


def test_every_kernel_is_reached(swept):
    """the defaults reach every kernel but the opt-in ones, which are reached under their option.  F(2x2) through the workspace counts as
    opt-in here: by the rules F(4x4) (wino_f4 = 7, the 28 / 14 / 7 maps) takes every launch it would get, from smaller batches on (14x14: F(4x4)
    from B = 15, F(2x2) from B = 41), and the 56x56 layers have 64 < wino_min_c channels -- it runs where wino_f4 leaves a map to it"""
    dflt = reached(swept[("defaults", False)]) | reached(swept[("defaults", True)])
    assert dflt == set(R.KERNELS) - {"bf16_p8", "wino4_fused", "wino"}, dflt
    assert "wino" in reached(swept[("wino_f4=0", False)])
    assert "wino4_fused" in reached(swept[("wino4_fused=12", False)])
    assert "bf16_p8" in reached(swept[("halo3=0,bf16_p8=31", True)])
    assert len(_lib.CONV_KERNELS) == len(R.KERNELS)


def test_halo3_beats_bf16_p8(lib):
    """bf16_p8 bits 1-2 name the 3x3 layers of stages 4 and 5; while halo3 holds their map sizes they stay on the halo kernel"""
    for name in ("res4b_branch2b", "res5b_branch2b"):
        idx = CONV_INDEX[name]
        both = asked(lib, config(lib, True, dict(bf16_p8=31)), idx, 64, False, False, True)
        freed = asked(lib, config(lib, True, dict(bf16_p8=31, halo3=0)), idx, 64, False, False, True)
        assert _lib.CONV_KERNELS[both.kernel] == "halo3" and both.tile == -1
        assert _lib.CONV_KERNELS[freed.kernel] == "bf16_p8" and freed.tile == R.TP8


def test_slab_major_consumer_has_slab_major_producer(swept):
    """a 3x3 layer that reads channel-slab major is fed by a branch2a that writes it: its own block's, or -- behind a chained launch -- the
    u1 output of the previous block's launch; and nothing else is written slab major"""
    n = 0
    for cases in swept.values():
        for case, got, ref in cases:
            prev = None
            for (_, _, _, i2a, i2b, i2c, _) in R.BLOCKS:
                chained_in = prev is not None and got[prev].join == 2
                produced = bool(got[prev].next_slab8) if chained_in else bool(got[i2a].out_slab8)
                assert produced == bool(got[i2b].in_slab8), (case, CONV_SPECS[i2b].name)
                if chained_in:
                    assert bool(got[i2a].out_slab8) == produced, (case, CONV_SPECS[i2a].name)  # the layer asked alone says the same
                n += bool(got[i2b].in_slab8)
                prev = i2c
            assert not any(got[i].out_slab8 for i in range(len(CONV_SPECS)) if i not in {b[3] for b in R.BLOCKS})
    assert n > 0


NEEDS = {"f32s": "w_split", "wino": "wino_u", "wino_fused": "wino_u", "wino4": "wino4_u", "wino4_fused": "wino4_u"}


def test_pack_mask_covers_every_route(swept):
    """the mask equals the restated packing conditions and holds what every swept route reads"""
    for (name, bf16), cases in swept.items():
        pl = R.resolve_plan(bf16, **OPTION_SETS[name])
        for case, got, ref in cases:
            for idx, g in got.items():
                assert g.packs == R.pack_mask(R.packs(pl, bf16, idx)), (name, case, CONV_SPECS[idx].name)
                need = NEEDS.get(_lib.CONV_KERNELS[g.kernel])
                assert need is None or g.packs >> R.PACK_BITS[need] & 1, (name, case, CONV_SPECS[idx].name, need)
                if g.join:  # dual, or the chained conv_block form, reads the concatenated weights
                    first = CONV_SPECS[idx + 1].name.endswith("branch1")
                    assert not first or g.packs >> R.PACK_BITS["w_dual"] & 1
                    assert g.join != 1 or _lib.CONV_KERNELS[g.join_kernel] != "f32s" or g.packs >> R.PACK_BITS["w_dual_split"] & 1
            assert got[0].packs >> R.PACK_BITS["stem_w"] & 1


def test_refusals(lib):
    cfg = config(lib, False, {})
    r = _lib.HpeConvRoute(struct_size=C.sizeof(_lib.HpeConvRoute))
    call = lib.hpe_debug_conv_route
    assert call(C.byref(cfg), 5, 8, 0, 0, 1, C.byref(r)) == 0
    for idx, B in ((-1, 8), (len(CONV_SPECS), 8), (5, 0), (5, -3)):
        assert call(C.byref(cfg), idx, B, 0, 0, 1, C.byref(r)) == 1 and b"idx must be" in lib.hpe_last_error()
    r.struct_size -= 4
    assert call(C.byref(cfg), 5, 8, 0, 0, 1, C.byref(r)) == 1 and b"struct_size" in lib.hpe_last_error()
    r.struct_size += 4
    cfg.struct_size -= 4
    assert call(C.byref(cfg), 5, 8, 0, 0, 1, C.byref(r)) == 1 and b"struct_size" in lib.hpe_last_error()
    assert call(None, 5, 8, 0, 0, 1, C.byref(r)) == 1 and call(C.byref(cfg), 5, 8, 0, 0, 1, None) == 1
