"""CPU-side checks of the guarded optimiser step (csrc/adam.hip, DESIGN.md "Guarded optimiser step"): the NumPy restatement
(tests/grad_guard_ref.py) against math.fsum inside its a-priori bound, the new entry points in header and binding, and every refusal of
the three calls.  NONE of the refusals needs a device: each call checks its arguments on the host (hpe_grad_stats from the host copy of
the offsets table) before it touches HIP, so the pointers below are plain numbers that are never dereferenced."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import hpe_amd
from hpe_amd import _lib

import adam_ref
import grad_guard_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hpe_grad_stats_chunk", "hpe_grad_stats_workspace_bytes", "hpe_grad_stats", "hpe_adam_guard", "hpe_adam_apply_guarded")
CH = G.CHUNK


@pytest.fixture(scope="module")
def lib():
    hpe_amd.build.build()
    return _lib.load()


def values(n, kind, seed=0):
    rng = np.random.RandomState(seed + n % 997)
    if kind == "normal":
        return rng.standard_normal(n).astype(np.float32)
    if kind == "tiny":
        return (rng.standard_normal(n) * 1e-30).astype(np.float32)
    return np.where(rng.rand(n) < 0.5, np.float32(3e38), np.float32(-3e38)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("kind", ("normal", "tiny", "huge"))
@pytest.mark.parametrize("n", (1, 3, 4, 5, 255, 256, 257, CH - 1, CH, CH + 1, 2 * CH + 1, 100003))
def test_restatement_is_inside_its_bound_against_fsum(n, kind):
    """every term is >= 0 and exact in float64, so (d + c) roundings of relative size 2^-53 bound the error of the kernel's order: the
    bound is computed from n (c = the number of chunk partials), not fixed"""
    x = values(n, kind)
    s, mx, bad = G.segment_record(x)
    exact = G.exact_sumsq(x)
    bound = 1.01 * (G.DEPTH + G.chunks_of(n)) * 2.0 ** -53
    assert bound == G.sumsq_bound(n)
    assert math.isfinite(s) and s > 0 and abs(s - exact) <= bound * exact, (n, kind, s, exact)
    assert mx == float(np.abs(x).max()) and bad == 0.0
    if kind == "tiny":  # the float32 squares are subnormal or zero: the float64 ones are not lost
        assert float(np.float32(x[0]) * np.float32(x[0])) < np.finfo(np.float32).tiny and s > 1e-62 * n / 2
    if kind == "huge":  # the float32 square overflows
        with np.errstate(over="ignore"):
            assert np.isinf(x[0] * x[0])
        assert s == pytest.approx(9e76 * n, rel=1e-6)


def test_restatement_tree_and_segments():
    """the tree is the documented one (checked on a chunk where the order shows), a segment's record does not know its neighbours, and
    non-finite elements are counted, kept out of the maximum and part of the sum"""
    x = np.zeros(CH, np.float32)
    x[:4] = (1.0, 2.0 ** -27, 2.0 ** -26, 2.0 ** -27)  # squares 1, 2^-54, 2^-52, 2^-54
    s, _, _ = G.chunk_partial(x)
    assert s == (1.0 + 2.0 ** -52) + (2.0 ** -54 + 2.0 ** -54) == 1.0 + 2.0 ** -51  # (x0^2 + x2^2) + (x1^2 + x3^2): a tie, to even
    assert s != (1.0 + 2.0 ** -54) + (2.0 ** -52 + 2.0 ** -54)  # what pairing neighbours would give
    g = values(3 * CH + 11, "normal", 5)
    offs = [0, 1, 6, CH - 1, CH + 5, 2 * CH + 4, 2 * CH + 4, 3 * CH + 11]
    rec = G.grad_stats(g, offs)
    assert rec.shape == (7, 3) and tuple(rec[5]) == (0.0, 0.0, 0.0)
    for i, (a, b) in enumerate(zip(offs[:-1], offs[1:])):
        assert tuple(rec[i]) == G.segment_record(g[a:b])
    g2 = g.copy()
    g2[0], g2[7], g2[CH + 5] = np.nan, np.inf, -np.inf
    rec2 = G.grad_stats(g2, offs)
    assert rec2[:, 2].tolist() == [1, 0, 1, 0, 1, 0, 0] and np.isnan(rec2[0, 0]) and np.isinf(rec2[2, 0]) and np.isinf(rec2[4, 0])
    assert rec2[0, 1] == 0.0 and rec2[2, 1] == float(np.abs(np.delete(g2[6:CH - 1], 1)).max())
    for i in (1, 3, 5, 6):
        assert rec2[i].tobytes() == rec[i].tobytes()


def test_restated_guard_decides_as_documented():
    st, gd = G.new_state(), G.new_guard()
    rec = [np.array([[9.0, 3.0, 0.0]]), np.array([[16.0, 4.0, 0.0], [0.0, 0.0, 0.0]])]
    s1, g1 = G.guard(st, gd, rec, 1e-4, 0.9, 0.999)  # no clipping
    assert g1[G.NORM] == 5.0 and g1[G.SCALE] == 1.0 and g1[G.APPLIED] == 1.0 and g1[G.CLIPPED] == 0.0 and g1[G.MAXABS] == 4.0
    assert s1[0] == 1.0 and s1[3] == adam_ref.alpha64(1e-4, 0.9, 0.999, 1)
    s2, g2 = G.guard(s1, g1, rec, 1e-4, 0.9, 0.999, clip_norm=5.0)  # norm == clip_norm: exactly 1, not counted
    assert g2[G.SCALE] == 1.0 and g2[G.CLIPPED] == 0.0 and s2[0] == 2.0
    s3, g3 = G.guard(s2, g2, rec, 1e-4, 0.9, 0.999, clip_norm=1.0)
    assert g3[G.SCALE] == float(np.float32(1.0 / 5.0)) and g3[G.CLIPPED] == 1.0 and s3[0] == 3.0
    bad = rec + [np.array([[np.nan, 1.0, 2.0]])]
    s4, g4 = G.guard(s3, g3, bad, 1e-4, 0.9, 0.999, clip_norm=1.0, skip_nonfinite=True)
    assert s4.tobytes() == s3.tobytes() and g4[G.APPLIED] == 0.0 and g4[G.SKIPPED] == 1.0 and g4[G.NONFINITE] == 2.0 and g4[G.CLIPPED] == 1.0
    s5, g5 = G.guard(s4, g4, bad, 1e-4, 0.9, 0.999, clip_norm=1.0, skip_nonfinite=False)  # propagates: a NaN norm scales by 1
    assert s5[0] == 4.0 and g5[G.APPLIED] == 1.0 and g5[G.SCALE] == 1.0 and g5[G.SKIPPED] == 1.0 and np.isnan(g5[G.NORM])
    p = np.ones(4, np.float32)
    z = np.zeros(4, np.float32)
    out = G.apply_guarded(p, z, z, p, s4, g4, adam_ref.one_minus(0.9), adam_ref.one_minus(0.999), 1e-7)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(out, (p, z, z)))


# ------------------------------------------------------------------------------------------------ header, binding, refusals
def test_header_and_binding_carry_the_entry_points(lib):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hpe.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in _lib.declared_symbols() and hasattr(lib, name), name
    assert lib.hpe_grad_stats_chunk() == G.CHUNK
    for n, S in ((0, 1), (1, 1), (CH, 1), (100003, 7)):
        assert lib.hpe_grad_stats_workspace_bytes(n, S) == 8 * (S + 1) + 8 * G.RECORD * (n // CH + S)
        assert n // CH + S >= G.chunks_of(n)  # room for every chunk however the S segments cut n
    assert len(hpe_amd.KerasAdam.GUARD_FIELDS) == G.GUARD_DOUBLES
    assert [hpe_amd.KerasAdam.GUARD_FIELDS.index(k) for k in ("norm", "scale", "applied", "skipped", "clipped", "nonfinite", "maxabs", "sumsq")] == \
        [G.NORM, G.SCALE, G.APPLIED, G.SKIPPED, G.CLIPPED, G.NONFINITE, G.MAXABS, G.SUMSQ]


def refused(lib, rc, *words):
    assert rc == 1, rc  # HPE_ERR_INVALID
    msg = lib.hpe_last_error().decode()
    assert msg and all(w in msg for w in words), msg


def test_grad_stats_refusals_need_no_device(lib):
    P = 0x1000  # a pointer that is never dereferenced: every check below comes before the first HIP call
    n, S = 100, 2
    off = (C.c_longlong * 3)(0, 40, 100)
    offp = C.addressof(off)
    ws = lib.hpe_grad_stats_workspace_bytes(n, S)
    call = lambda g=P, n=n, oh=offp, od=P, S=S, rec=P, w=P, wb=ws: lib.hpe_grad_stats(g, n, oh, od, S, rec, w, wb, None)  # noqa: E731
    for kw in ({"g": None}, {"oh": None}, {"od": None}, {"rec": None}, {"w": None}):
        refused(lib, call(**kw), "null")
    refused(lib, call(n=-1), "n must be >= 0")
    refused(lib, call(S=0), "S must be >= 1")
    desc = (C.c_longlong * 3)(0, 60, 40)
    refused(lib, call(oh=C.addressof(desc)), "ascend")
    neg = (C.c_longlong * 3)(-1, 40, 100)
    refused(lib, call(oh=C.addressof(neg)), "offsets[0]")
    refused(lib, call(n=99), "beyond n")
    refused(lib, call(wb=ws - 1), "workspace", str(ws))
    assert lib.hpe_grad_stats_workspace_bytes(-1, 1) == -1 and lib.hpe_last_error()
    assert lib.hpe_grad_stats_workspace_bytes(10, 0) == -1


def test_guard_and_guarded_apply_refusals_need_no_device(lib):
    P = 0x1000
    recs, counts = (C.c_void_p * 2)(P, P), (C.c_int * 2)(1, 3)
    rp, cp = C.addressof(recs), C.addressof(counts)
    call = lambda st=P, gd=P, r=rp, c=cp, k=2, lr=1e-4, b1=0.9, b2=0.999, clip=1.0: lib.hpe_adam_guard(st, gd, r, c, k, lr, b1, b2, clip, 1, None)  # noqa: E731
    for kw in ({"st": None}, {"gd": None}, {"r": None}, {"c": None}):
        refused(lib, call(**kw), "null")
    hole = (C.c_void_p * 2)(P, None)
    refused(lib, call(r=C.addressof(hole)), "null", "list 1")
    zero = (C.c_int * 2)(1, 0)
    refused(lib, call(c=C.addressof(zero)), "at least one record")
    refused(lib, call(k=0), "n_lists")
    refused(lib, call(k=17), "n_lists")
    refused(lib, call(clip=-1.0), "clip_norm")
    refused(lib, call(clip=float("nan")), "clip_norm")
    refused(lib, call(lr=float("inf")), "lr")
    refused(lib, call(b1=1.0), "beta")
    omb1, omb2 = float(adam_ref.one_minus(0.9)), float(adam_ref.one_minus(0.999))
    for i in range(6):
        a = [P] * 6
        a[i] = None
        refused(lib, lib.hpe_adam_apply_guarded(a[0], a[1], a[2], a[3], 8, a[4], a[5], omb1, omb2, 1e-7, None), "null")
    refused(lib, lib.hpe_adam_apply_guarded(P, P, P, P, -1, P, P, omb1, omb2, 1e-7, None), "n must be >= 0")
    assert lib.hpe_adam_apply_guarded(P, P, P, P, 0, P, P, omb1, omb2, 1e-7, None) == 0  # n == 0 launches nothing


def test_optimiser_and_trainers_refuse_bad_options():
    with pytest.raises(ValueError):
        hpe_amd.KerasAdam(1e-4, global_clipnorm=-1.0)
    with pytest.raises(ValueError):
        hpe_amd.KerasAdam(1e-4, global_clipnorm=float("nan"))
    opt = hpe_amd.KerasAdam(1e-4)
    assert not opt.guarded and opt.skipped_steps == 0 and opt.clipped_steps == 0
    assert hpe_amd.KerasAdam(1e-4, global_clipnorm=float("inf")).guarded and hpe_amd.KerasAdam(1e-4, skip_nonfinite=True).guarded
    from hpe_amd.optim import layer_segments
    from hpe_amd import critic_spec, regressor_spec, resnet_spec

    for kind, total, layers in (("regressor", regressor_spec.PARAM_FLOATS, 4), ("encoder", resnet_spec.ENCODER_PARAM_FLOATS, 53),
                                ("critic", critic_spec.PARAM_FLOATS, 9)):
        off, names = layer_segments(kind)
        assert off[0] == 0 and off[-1] == total and len(off) == len(names) + 1 and len(set(names)) == layers
        assert all(b > a for a, b in zip(off[:-1], off[1:]))
    assert [o for _k, o, _s in regressor_spec.flat_layout()] == layer_segments("regressor")[0][:-1]
    assert [o for _k, o, _s in critic_spec.flat_layout()] == layer_segments("critic")[0][:-1]
