"""hpe_encoder_set_params_dev and its read-back without a GPU: the three symbols are declared in include/hpe.h, mirrored in _lib.py and
exported, the packing names follow the header's enum, and the refusals that need no device."""
import os
import re

import pytest

from hpe_amd import _lib, build as hbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hpe_encoder_set_params_dev", "hpe_debug_encoder_packing_bytes", "hpe_debug_encoder_packing")


@pytest.fixture(scope="module")
def lib():
    hbuild.build()
    return _lib.load()


def test_symbols_declared_and_exported(lib):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hpe.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in _lib.declared_symbols() and hasattr(lib, name), name


def test_packing_names_follow_the_header():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hpe.h")).read(), flags=re.S)
    enum = re.findall(r"\bHPE_PACK_([A-Z0-9_]+)\b", txt[txt.index("HPE_PACK_W"):])
    assert enum[-1] == "COUNT" and tuple(n.lower() for n in enum[:-1]) == _lib.ENCODER_PACKINGS


def test_null_context(lib):
    assert lib.hpe_encoder_set_params_dev(None, None, None) == 1
    for which in range(len(_lib.ENCODER_PACKINGS)):
        assert lib.hpe_debug_encoder_packing_bytes(None, 0, which) == 0
    assert lib.hpe_debug_encoder_packing(None, 0, 0, None, None) == 1
