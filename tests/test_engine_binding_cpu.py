"""The binding's tables, without a GPU: the (role, BatchNorm mode, precision) -> C symbol table of encoder training
(_lib.ENCODER_ENTRY through HpeEngine._entry_symbol) against the names as include/hpe.h spells them, written out here; the refusal of
precision="bf16" with batch statistics; and the *_mixed prototypes that _lib derives from their fp32 twins."""
import hashlib

import pytest

import hpe_amd
from hpe_amd import _lib, build as hbuild

# role -> the four families' symbols: (frozen fp32, frozen mixed, batch fp32, batch mixed); None: the role has no frozen-statistics form
SYMBOLS = {
    "reserve": ("hpe_encoder_train_reserve", "hpe_encoder_train_reserve_mixed",
                "hpe_encoder_train_reserve_batchnorm", "hpe_encoder_train_reserve_batchnorm_mixed"),
    "ws_floats": ("hpe_encoder_train_ws_floats", "hpe_encoder_train_ws_floats_mixed",
                  "hpe_encoder_train_ws_floats_batchnorm", "hpe_encoder_train_ws_floats_batchnorm_mixed"),
    "forward": ("hpe_encoder_forward_train", "hpe_encoder_forward_train_mixed",
                "hpe_encoder_forward_batchnorm", "hpe_encoder_forward_batchnorm_mixed"),
    "backward": ("hpe_encoder_backward", "hpe_encoder_backward_mixed",
                 "hpe_encoder_backward_batchnorm", "hpe_encoder_backward_batchnorm_mixed"),
    "stash": ("hpe_debug_encoder_stash", "hpe_debug_encoder_stash_mixed", "hpe_debug_encoder_stash", "hpe_debug_encoder_stash_mixed"),
    "stash_batch": ("hpe_debug_encoder_stash_batch", "hpe_debug_encoder_stash_batch_mixed",
                    "hpe_debug_encoder_stash_batch", "hpe_debug_encoder_stash_batch_mixed"),
    "stash_raw": (None, None, "hpe_debug_encoder_stash_raw", "hpe_debug_encoder_stash_raw_mixed"),
    "conv_batchnorm": (None, None, "hpe_debug_conv_batchnorm", "hpe_debug_conv_batchnorm_mixed"),
    "conv_backward": ("hpe_debug_conv_backward", "hpe_debug_conv_backward_mixed",
                      "hpe_debug_conv_backward_batchnorm", "hpe_debug_conv_backward_batchnorm_mixed"),
    "maxpool_backward": ("hpe_debug_maxpool_backward", "hpe_debug_maxpool_backward_mixed",
                         "hpe_debug_maxpool_backward", "hpe_debug_maxpool_backward_mixed"),
    "avgpool_backward": ("hpe_debug_avgpool_backward", "hpe_debug_avgpool_backward_mixed",
                         "hpe_debug_avgpool_backward", "hpe_debug_avgpool_backward_mixed"),
}
REFUSAL = "precision='bf16' runs with frozen BatchNorm statistics only: batch statistics in bf16 are the follow-up"
PAIRS = [(bn, precision) for bn in ("frozen", "batch") for precision in ("fp32", "bf16", "mixed")]

# sorted(_lib._PROTOS) of the parent commit, where the sixteen *_mixed prototypes were written out by hand
DECLARED_COUNT = 153
DECLARED_SHA256 = "c8e472ac628d1836300f647223114c015131ada429217ead76a17bb5976b41f6"


def test_table_covers_the_roles():
    assert set(_lib.ENCODER_ENTRY) == set(SYMBOLS)


@pytest.mark.parametrize("bn,precision", PAIRS)
def test_every_role_resolves_to_the_header_symbol(bn, precision):
    declared = _lib.declared_symbols()
    for role, names in SYMBOLS.items():
        if (bn, precision) == ("batch", "bf16"):
            with pytest.raises(ValueError) as e:
                hpe_amd.HpeEngine._entry_symbol(role, bn, precision)
            assert str(e.value) == REFUSAL
            continue
        want = names[2 * (bn == "batch") + (precision != "fp32")]
        if want is None:
            with pytest.raises(ValueError):
                hpe_amd.HpeEngine._entry_symbol(role, bn, precision)
            continue
        name, prec = hpe_amd.HpeEngine._entry_symbol(role, bn, precision)
        assert name == want and name in declared
        assert (prec.suffix, prec.dtype) == (("_mixed", "bfloat16") if precision != "fp32" else ("", "float32"))
        assert name.endswith("_mixed") == (precision != "fp32")


def test_every_listed_symbol_is_declared():
    declared = set(_lib.declared_symbols())
    listed = {n for names in SYMBOLS.values() for n in names if n}
    assert len(listed) == 32 and listed <= declared
    assert {n for n in declared if n.endswith("_mixed")} == {n for n in listed if n.endswith("_mixed")}


def test_refusal_text_and_bad_names():
    with pytest.raises(ValueError) as e:
        hpe_amd.HpeEngine._mixed("bf16", "batch")
    assert str(e.value) == REFUSAL
    with pytest.raises(ValueError, match="precision must be 'fp32', 'bf16' or 'mixed', got 'fp16'"):
        hpe_amd.HpeEngine._entry_symbol("forward", "frozen", "fp16")
    with pytest.raises(ValueError, match="bn must be 'frozen' or 'batch', got 'moving'"):
        hpe_amd.HpeEngine._entry_symbol("forward", "moving", "fp32")


def test_mixed_prototypes_equal_their_twins():
    derived = [n for n in _lib._PROTOS if n.endswith("_mixed")]
    assert len(derived) == 16
    for name in derived:
        twin = name[:-len("_mixed")]
        assert _lib._PROTOS[name][0] is _lib._PROTOS[twin][0], name
        assert list(_lib._PROTOS[name][1]) == list(_lib._PROTOS[twin][1]), name
    hbuild.build()
    lib = _lib.load()  # the bound functions carry them too
    for name in derived:
        fn, twin = getattr(lib, name), getattr(lib, name[:-len("_mixed")])
        assert fn.restype is twin.restype and tuple(fn.argtypes) == tuple(twin.argtypes), name


def test_declared_symbols_are_the_parents():
    d = _lib.declared_symbols()
    assert d == sorted(d) and len(d) == DECLARED_COUNT
    assert hashlib.sha256("\n".join(d).encode()).hexdigest() == DECLARED_SHA256
