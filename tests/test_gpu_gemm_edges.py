"""GPU tests of the fp32 implicit-GEMM kernel (conv_gemm.hip) through hpe_debug_gemm_ex: every tile instantiation, the dense, strided,
3x3 and dual A-operand modes, split-K with its fix-up kernel, both residual paths and the y_slab8 layout, at the smallest shapes where
the kernel can still go wrong -- one row, one tile less / exactly / one more than a tile, two tiles and a bit, widths that are not a
multiple of 4, pitches wider than the rows, maps whose rows and images end inside a tile -- against the float64 references of
tests/gemm_ref.py on the same float32 inputs (signed data, a different scale and shift in every column).

Every output buffer has one row more than M and a pitch wider than N, filled with a sentinel bit pattern; every check includes
"the sentinels are untouched".  Bar: the project's single-conv bar, max|got - ref| / max|ref| <= 5e-6, applied to the whole matrix
and, separately, to the rows of the last partial M-tile and the columns of the last partial N-tile (gemm_ref.edge_errors).  The float32
NumPy restatement of the same inputs sits under a quarter of it (tests/test_gemm_ref_cpu.py).

A test runs all its cases, then fails with the list of (tile, mode, shape, block) that missed.  Each prints its worst figures
(pytest -s); DESIGN.md section 2, "GEMM coverage", records them.
"""
import ctypes as C

import numpy as np
import pytest

import gemm_ref as R
import hpe_amd
from hpe_amd import _lib, synthetic

pytestmark = pytest.mark.gpu

SENTINEL = -559038737  # 0xDEADBEEF as int32: a float no kernel computes (-6.26e18)
MODE_NAMES = {R.DENSE: "dense", R.STRIDED: "strided", R.CONV3: "conv3", R.DUAL: "dual"}
GEMM_FIELDS = ("M", "N", "K", "lda", "ldw", "ldy", "ldres", "w_rows", "relu", "Hi", "Wi", "Cin", "Ho", "Wo", "stride", "k1_slabs", "y_slab8",
               "use_splitk")


@pytest.fixture(scope="module")
def eng():
    e = hpe_amd.HpeEngine(device=0, max_batch=1)
    e.load_regressor(synthetic.make_regressor_params())
    e.load_mean_theta(np.zeros(85, np.float32))
    e.finalize()
    yield e
    e.close()


def gpu(a):
    import torch

    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def upload(inp):
    return {k: gpu(inp[k]) for k in ("x", "x2", "wt", "res", "scale", "shift")}


def out_rows(c):
    """rows x pitch of the output buffer: one row (slab8: four 8-float rows) more than the kernel may write"""
    return (c["N"] // 8 * c["M"] + 4, 8) if c.get("y_slab8") else (c["M"] + 1, c["ldy"])


def new_output(c):
    import torch

    return torch.full(out_rows(c), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)


def launch(eng, c, dev):
    """-> (the whole output buffer as int32 bits, split_k)"""
    y = new_output(c)
    kw = {k: c[k] for k in GEMM_FIELDS if k in c}
    sk = eng.debug_gemm_ex(c["mode"], c["tile"], dev["x"], dev["wt"], y, x2=dev["x2"], residual=dev["res"], scale=dev["scale"], shift=dev["shift"], **kw)
    return y.cpu().numpy().view(np.int32), sk


def split_output(c, bits):
    """(the [M, N] result re-laid row-major, True if every word outside it still holds the sentinel)"""
    M, N = c["M"], c["N"]
    if c.get("y_slab8"):
        rows = N // 8 * M
        got = bits[:rows].view(np.float32).reshape(N // 8, M, 8).transpose(1, 0, 2).reshape(M, N)
        return got, bool((bits[rows:] == SENTINEL).all())
    return bits[:M, :N].view(np.float32), bool((bits[:M, N:] == SENTINEL).all() and (bits[M:] == SENTINEL).all())


def describe(c):
    s = "%s %s M=%d N=%d K=%d" % (R.TILE_NAMES[c["tile"]], MODE_NAMES[c["mode"]], c["M"], c["N"], c["K"])
    if c["mode"] != R.DENSE:
        s += " %dx%d->%dx%d/s%d Cin=%d" % (c["Hi"], c["Wi"], c["Ho"], c["Wo"], c["stride"], c["Cin"])
    s += " lda=%d ldy=%d" % (c["lda"], c["ldy"])
    for k in ("use_res", "relu", "y_slab8", "use_splitk", "k1_slabs"):
        if c.get(k):
            s += " %s=%d" % (k, c[k])
    return s


class Tally:
    """runs cases, remembers the worst figure per block and every miss; check() fails with all of them"""

    def __init__(self, eng):
        self.eng, self.worst, self.missed, self.n = eng, [0.0, 0.0, 0.0], [], 0

    def run(self, c, want_split=None, twice=False):
        inp = R.inputs(c)
        dev = upload(inp)
        bits, sk = launch(self.eng, c, dev)
        got, clean = split_output(c, bits)
        ref = R.reference(c, inp)
        if c.get("y_slab8"):  # the layout itself: the raw buffer against the reference re-laid by gemm_ref.to_slab8
            raw = bits[: c["N"] // 8 * c["M"]].view(np.float32)
            if R.rel(raw, R.to_slab8(ref)) > R.BAR:
                self.missed.append(describe(c) + ": slab8 layout")
        e = R.edge_errors(got, ref, *R.TILES[c["tile"]])
        self.n += 1
        for i, (name, v) in enumerate(zip(("whole matrix", "last partial M-tile", "last partial N-tile"), e)):
            self.worst[i] = max(self.worst[i], v) if np.isfinite(v) else float("inf")
            if not v <= R.BAR:
                self.missed.append("%s: %s %.3e" % (describe(c), name, v))
        if not clean:
            self.missed.append(describe(c) + ": sentinel overwritten")
        if want_split == "split" and not sk > 1:
            self.missed.append("%s: split_k = %d, expected a split" % (describe(c), sk))
        if want_split == "whole" and sk != 1:
            self.missed.append("%s: split_k = %d, expected 1" % (describe(c), sk))
        if twice:
            again, sk2 = launch(self.eng, c, dev)
            if sk2 != sk or not np.array_equal(again, bits):
                self.missed.append(describe(c) + ": two runs differ")
        return sk

    def check(self, what):
        print("%s: %d launches, worst whole %.2e, M edge %.2e, N edge %.2e (bar %.0e)" % ((what, self.n) + tuple(self.worst) + (R.BAR,)))
        assert not self.missed, "%d of %d launches missed:\n  " % (len(self.missed), self.n) + "\n  ".join(self.missed[:40])


@pytest.mark.parametrize("tile", range(7), ids=R.TILE_NAMES[:7])
def test_dense_every_edge(eng, tile):
    """M in {1, BM-1, BM, BM+1, 2BM+37} x N in {4, BN-4, BN, BN+4, 2BN+20, 85 at run_dense's pitch} x K in {32, 64, 96, 512}; residual,
    ReLU and the pitches (lda > K, ldy > N, ldres != ldy) cycle over the cases (gemm_ref.dense_cases)"""
    t = Tally(eng)
    for c in R.dense_cases(tile):
        t.run(c, want_split="whole")  # no workspace handed over: never split
    t.check("dense " + R.TILE_NAMES[tile])


def test_slab8_layout(eng):
    t = Tally(eng)
    for tile in R.SLAB8_TILES:
        for c in R.slab8_cases(tile):
            t.run(c)
    t.check("y_slab8")


@pytest.mark.parametrize("tile", R.SPLIT_TILES, ids=R.TILE_NAMES[:4])
def test_splitk_and_fixup(eng, tile):
    """the 4-wave tiles with the context's workspace: the launcher must report a split (K = 288 is 9 slabs: uneven slices), the fix-up
    kernel's result holds the bar and two runs are bit-identical"""
    t = Tally(eng)
    for c in R.splitk_cases(tile):
        sk = t.run(c, want_split="split", twice=True)
        assert sk == R.expected_split_k(c), (describe(c), sk)
    t.check("split-K " + R.TILE_NAMES[tile])


def test_eight_wave_tiles_never_split(eng):
    t = Tally(eng)
    for c in R.w8_splitk_cases():
        t.run(c, want_split="whole")
    t.check("8-wave tiles with the workspace")


@pytest.mark.parametrize("tile", range(7), ids=R.TILE_NAMES[:7])
def test_strided(eng, tile):
    """B = 3, (Hi, Ho, stride) in {(6, 3, 2), (14, 7, 2), (7, 7, 1)} x Cin in {32, 96} x N in {64, 132}, on every tile"""
    t = Tally(eng)
    for c in R.strided_cases(tile):
        t.run(c)
    t.check("strided " + R.TILE_NAMES[tile])


@pytest.mark.parametrize("tile", range(7), ids=R.TILE_NAMES[:7])
def test_conv3(eng, tile):
    """B = 3, maps 1x1, 3x3, 7x7, 14x14 and 5x7 x Cin in {32, 64} x N in {64, 192}, on every tile; every pixel is non-zero, so a tap that
    leaks across a row end or into the next image shows against the per-image zero padding of the reference.  5x7 (H != W) is inside the
    launcher's contract and the kernel handles it: it stays accepted."""
    t = Tally(eng)
    for c in R.conv3_cases(tile):
        t.run(c)
    t.check("conv3 " + R.TILE_NAMES[tile])


def test_conv3_splitk(eng):
    """the 3x3 mode cut along K (what the product runs at small batches): slices that start inside a tap (slab_seek)"""
    t = Tally(eng)
    for c in R.conv3_cases(2, use_splitk=1):
        t.run(c, want_split="split" if R.expected_split_k(c) > 1 else "whole", twice=True)
    t.check("conv3 split-K 64x64")


@pytest.mark.parametrize("tile", range(7), ids=R.TILE_NAMES[:7])
def test_dual(eng, tile):
    """k1_slabs in {1, 3} x Cin in {32, 64} x (stride 1 at 7x7, stride 2 from 14x14) x N in {128, 260}, B = 3, no residual"""
    t = Tally(eng)
    for c in R.dual_cases(tile):
        t.run(c)
    t.check("dual " + R.TILE_NAMES[tile])


def test_old_entry_point(eng):
    """hpe_debug_gemm (tools/gemm_bench.py) is the dense mode with scale 1, shift 0 and dense pitches"""
    g = R.rng(77)
    M, N, K = 70, 64, 96
    A, W = R.normal(g, (M, K)), R.weights(g, N, K)
    y = new_output(dict(M=M, N=N, ldy=N))
    x, wt = gpu(A), gpu(W)
    _lib.check(eng.lib.hpe_debug_gemm(eng._h, x.data_ptr(), wt.data_ptr(), M, N, K, 64, 2, None, 1, y.data_ptr(), None))
    bits = y.cpu().numpy().view(np.int32)
    assert R.rel(bits[:M].view(np.float32), np.maximum(R.acc_dense(A, W), 0)) <= R.BAR and (bits[M:] == SENTINEL).all()


def test_rejected_launches(eng):
    """each clause of the launcher's contract broken once (gemm_ref.ERROR_CASES): HPE_ERR_INVALID, a message that names the clause,
    split_k = 0 and an untouched output.  Nothing is launched, so nothing here can reach the device with a bad shape."""
    import torch

    lib = eng.lib
    missed = []
    for i in range(len(R.ERROR_CASES)):
        c, null, mis = R.error_case(i)
        base = R.error_bases()[R.ERROR_CASES[i][0]]
        want = R.contract_violations(c, null, mis)
        assert len(want) == 1
        inp = R.inputs(base)
        if inp["res"] is None:
            inp["res"] = np.zeros((base["M"], base["ldres"]), np.float32)
        dev = upload(inp)
        y = new_output(base)
        ptr = dict(x=dev["x"], x2=dev["x2"], wt=dev["wt"], residual=dev["res"] if c["use_res"] else None, y=y)
        g = _lib.HpeDebugGemm()
        g.struct_size = C.sizeof(_lib.HpeDebugGemm)
        g.mode, g.tile = c["mode"], c["tile"]
        for k in GEMM_FIELDS:
            setattr(g, k, c.get(k, 0))
        for k, t in ptr.items():
            a = None if t is None or k in null else t.data_ptr() + (4 if k in mis else 0)
            setattr(g, k, a)
        g.scale, g.shift = dev["scale"].data_ptr(), dev["shift"].data_ptr()
        sk = C.c_int(-1)
        g.split_k = C.pointer(sk)
        rc = lib.hpe_debug_gemm_ex(eng._h, C.byref(g), None)
        msg = lib.hpe_last_error().decode()
        torch.cuda.synchronize()
        ok = rc == 1 and sk.value == 0 and len(msg) > 20 and ("contract" in msg or "mode" in msg) and want[0] in msg and bool((y.view(torch.int32) == SENTINEL).all())
        if not ok:
            missed.append((i, R.ERROR_CASES[i], rc, sk.value, msg))
    assert not missed, missed
    # the struct's own guard
    g = _lib.HpeDebugGemm()
    assert lib.hpe_debug_gemm_ex(eng._h, C.byref(g), None) == 1 and b"struct_size" in lib.hpe_last_error()
    assert lib.hpe_debug_gemm_ex(eng._h, None, None) == 1
    # scale / shift NULL: the context's ones / zeros, N <= 1024 only
    base = dict(R.error_bases()["dense"], N=1028, w_rows=1088, ldy=1032, use_res=0)
    g.struct_size = C.sizeof(_lib.HpeDebugGemm)
    for k in GEMM_FIELDS:
        setattr(g, k, base.get(k, 0))
    g.mode, g.tile = base["mode"], base["tile"]
    z = torch.zeros(1088 * 64, device="cuda")
    g.x = g.wt = g.y = z.data_ptr()
    assert lib.hpe_debug_gemm_ex(eng._h, C.byref(g), None) == 1 and b"1024" in lib.hpe_last_error()
    assert not z.any()
