"""GPU tests of the other three implicit-GEMM kernels -- conv_gemm_f32s.hip (fp32 on the bf16 matrix cores, split weights), conv_gemm_bf16.hip
(7 tiles) and conv_gemm_bf16_p8.hip (256x256, its own split-K and fix-up) -- through hpe_debug_gemm_launch, at the edges of the one contract
they share with the fp32 kernel (tests/test_gpu_gemm_edges.py has that one): every tile and mode, one row, one less / exactly / one more
than a tile, two tiles and a bit, widths that are no multiple of the 16-byte vector (the scalar tail of the epilogues), the prefetched
residual with an M tail and an N tail in one workgroup, K of one, two and three slabs, weight rows clamped at w_rows < 256, w_piece > K,
pitches wider than the rows, maps with H != W and images that end inside a tile.  References: float64, tests/gemm_ref.py, on the very
operands the kernel reads (bf16 kernels: inputs are bf16 values; f32s: the weights are split on the test side by the rule of the kernel's
header comment).

Every output buffer has one row more than M and a pitch wider than N, filled with a sentinel bit pattern (int16 0xDEAD for bf16 outputs,
int32 0xDEADBEEF for fp32 ones); every case asserts that the words outside [M, N] are untouched.

Bars, none taken from the code under test.  f32s: gemm_ref.BAR = 5e-6 on max|got - ref| / max|ref|, on the whole matrix and on the last
partial M-tile and N-tile.  bf16 and bf16_p8, first check: max|got - ref| / max|ref| < 2^-8 and rel-L2 < 2.5e-3 on the same three blocks;
second check, per element: |got - ref| <= 2^-8 |ref| + 4 e32 A[m][n] (gemm_ref.bf16_figures has the terms).  tests/test_gemm_ref_cpu.py
shows on the CPU that a float32 restatement passes all of it on every case.

A test runs all its cases, then fails with the list of (kernel, tile, mode, shape, block) that missed.  Each prints its worst figures
(pytest -s); DESIGN.md section 2, "GEMM coverage", records them.
"""
import ctypes as C

import numpy as np
import pytest

import gemm_ref as R
import hpe_amd
from hpe_amd import _lib, synthetic
from test_gpu_gemm_edges import GEMM_FIELDS, SENTINEL, describe as describe_shape

pytestmark = pytest.mark.gpu

SENTINEL16 = -8531  # 0xDEAD as int16: the bf16 -6.2e18, which no kernel computes
F32S_TILES, BF16_TILES = tuple(R.KERNELS["f32s"]["tiles"]), tuple(range(8))  # tile 7 is the 256x256 kernel
BF16_IDS = tuple(R.TILE_NAMES[t] for t in BF16_TILES)


def kernel_of(tile):
    return "bf16_p8" if tile == 7 else "bf16"


@pytest.fixture(scope="module")
def eng():
    e = hpe_amd.HpeEngine(device=0, max_batch=1)
    e.load_regressor(synthetic.make_regressor_params())
    e.load_mean_theta(np.zeros(85, np.float32))
    e.finalize()
    yield e
    e.close()


def describe(c):
    return c["kernel"] + " " + describe_shape(c) + (" w_piece=%d" % c["w_piece"] if "w_piece" in c else "") + " w_rows=%d" % c["w_rows"]


def gpu(a, bf16=False):
    import torch

    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    return t.to(torch.bfloat16) if bf16 else t  # exact: every such input is a bf16 value


def upload(c, inp):
    bf = R.reads_bf16(c["kernel"])
    dev = {k: gpu(inp[k], bf) for k in ("x", "x2", "res")}
    dev["wt"] = gpu(inp["wt"], True)  # f32s: the three bf16 pieces
    dev["scale"], dev["shift"] = gpu(inp["scale"]), gpu(inp["shift"])
    return dev


def new_output(c):
    import torch

    if R.reads_bf16(c["kernel"]):
        return torch.full((c["M"] + 1, c["ldy"]), SENTINEL16, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    return torch.full((c["M"] + 1, c["ldy"]), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)


def launch(eng, c, dev):
    """-> (the whole output buffer as integer bits, split_k)"""
    import torch

    y = new_output(c)
    kw = {k: c[k] for k in GEMM_FIELDS if k in c}
    sk = eng.debug_gemm_launch(R.KERNELS[c["kernel"]]["id"], c["mode"], c["tile"], dev["x"], dev["wt"], y, x2=dev["x2"], residual=dev["res"],
                               scale=dev["scale"], shift=dev["shift"], w_piece=c.get("w_piece", 0), **kw)
    bits = y.view(torch.int16 if R.reads_bf16(c["kernel"]) else torch.int32).cpu().numpy()
    return bits, sk


def split_output(c, bits):
    """(the [M, N] result as float32, True if every word outside it still holds the sentinel)"""
    M, N = c["M"], c["N"]
    if bits.dtype == np.int16:
        got = (bits[:M, :N].astype(np.uint16).astype(np.uint32) << 16).view(np.float32)
        sentinel = SENTINEL16
    else:
        got, sentinel = np.ascontiguousarray(bits[:M, :N]).view(np.float32), SENTINEL
    return got, bool((bits[:M, N:] == sentinel).all() and (bits[M:] == sentinel).all())


class Tally:
    """runs cases, remembers the worst figure per block and every miss; check() fails with all of them"""

    def __init__(self, eng):
        self.eng, self.missed, self.n, self.e32 = eng, [], 0, []
        self.worst = [[0.0, 0.0, 0.0] for _ in R.BLOCK_NAMES]  # per block: f32s (error, -, -); bf16 (max-normalised, rel-L2, element / bound)

    def note(self, block, figures):
        self.worst[block] = [max(w, v) if np.isfinite(v) else float("inf") for w, v in zip(self.worst[block], figures)]

    def run(self, c, want_split=1, twice=False):
        """-> (got [M, N], reference [M, N])"""
        inp = R.inputs(c)
        dev = upload(c, inp)
        bits, sk = launch(self.eng, c, dev)
        got, clean = split_output(c, bits)
        self.n += 1
        if R.reads_bf16(c["kernel"]):
            e32, figs = R.bf16_figures(c, inp, got)
            self.e32.append(e32)
            for i, f in enumerate(figs):
                if f is not None:
                    self.note(i, f[:3])
            self.missed += ["%s: %s" % (describe(c), m) for m in R.bf16_misses(figs)]
        else:
            for i, v in enumerate(R.edge_errors(got, R.reference(c, inp), *R.TILES[c["tile"]])):
                self.note(i, (v, 0.0, 0.0))
                if not v <= R.BAR:
                    self.missed.append("%s: %s %.3e" % (describe(c), R.BLOCK_NAMES[i], v))
        if not clean:
            self.missed.append(describe(c) + ": sentinel overwritten")
        if sk != want_split:
            self.missed.append("%s: split_k = %d, expected %d" % (describe(c), sk, want_split))
        if twice:
            again, sk2 = launch(self.eng, c, dev)
            if sk2 != sk or not np.array_equal(again, bits):
                self.missed.append(describe(c) + ": two runs differ")
        return got, R.reference(c, inp)

    def check(self, what):
        if self.e32:
            print("%s: %d launches, e32 %.2e .. %.2e; (max-normalised, rel-L2, element / bound) whole %.2e %.2e %.2f, M edge %.2e %.2e %.2f, N edge %.2e %.2e %.2f"
                  % ((what, self.n, min(self.e32), max(self.e32)) + tuple(v for w in self.worst for v in w)))
        else:
            print("%s: %d launches, worst whole %.2e, M edge %.2e, N edge %.2e (bar %.0e)" % ((what, self.n) + tuple(w[0] for w in self.worst) + (R.BAR,)))
        assert not self.missed, "%d misses in %d launches:\n  " % (len(self.missed), self.n) + "\n  ".join(self.missed[:60])


# ------------------------------------------------------------------------------------------- f32s
@pytest.mark.parametrize("tile", F32S_TILES, ids=[R.TILE_NAMES[t] for t in F32S_TILES])
def test_f32s_dense_every_edge(eng, tile):
    """M in {1, BM-1, BM, BM+1, 2BM+37} x N in {4, BN-4, BN, BN+4, 2BN+20, 85 at pitch 96} x K in {32, 64, 96, 512}, w_piece in {K, K + 8};
    every case twice: the kernel's header promises bitwise repeatability"""
    t = Tally(eng)
    for c in R.dense_cases(tile, "f32s"):
        t.run(c, twice=True)
    t.check("f32s dense " + R.TILE_NAMES[tile])


@pytest.mark.parametrize("tile", F32S_TILES, ids=[R.TILE_NAMES[t] for t in F32S_TILES])
def test_f32s_strided_and_dual(eng, tile):
    """the fp32 file's geometries (B = 3) x Cin in {32, 96}; dual: k1_slabs in {1, 3}; every case twice"""
    t = Tally(eng)
    for c in R.strided_cases(tile, "f32s") + R.dual_cases(tile, "f32s"):
        t.run(c, twice=True)
    t.check("f32s strided + dual " + R.TILE_NAMES[tile])


# ------------------------------------------------------------------------------------------- bf16 and bf16_p8
@pytest.mark.parametrize("tile", BF16_TILES, ids=BF16_IDS)
def test_bf16_dense_every_edge(eng, tile):
    """M in {1, BM-1, BM, BM+1, 2BM+37} x N in {4, BN-4, BN, BN+4, 2BN+20, 85 at pitch 96} x K in {64, 128, 192, 512}: N = 4, BN +- 4 and 85
    take the scalar tail next to the 16-byte store; 256x256: w_rows = N.  The cases of the largest M and K run twice."""
    t = Tally(eng)
    cases = R.dense_cases(tile, kernel_of(tile))
    for c in cases:
        t.run(c, twice=c["K"] == 512 and c["M"] == max(c["M"] for c in cases))
    t.check("%s dense %s" % (kernel_of(tile), R.TILE_NAMES[tile]))


@pytest.mark.parametrize("tile", BF16_TILES, ids=BF16_IDS)
def test_bf16_strided_and_dual(eng, tile):
    """B = 3, (Hi, Ho, stride) in {(6, 3, 2), (14, 7, 2), (7, 7, 1)} x Cin in {64, 192} x N in {64, 132}; dual: k1_slabs in {1, 3} x N in {128, 260}"""
    t = Tally(eng)
    for c in R.strided_cases(tile, kernel_of(tile)) + R.dual_cases(tile, kernel_of(tile)):
        t.run(c)
    t.check("%s strided + dual %s" % (kernel_of(tile), R.TILE_NAMES[tile]))


@pytest.mark.parametrize("tile", BF16_TILES, ids=BF16_IDS)
def test_bf16_conv3(eng, tile):
    """B = 3, maps 1x1, 3x3, 7x7, 14x14 and 5x7 x Cin in {64, 192} (256x256: {64, 128}) x N in {64, 192}; every pixel non-zero"""
    t = Tally(eng)
    for c in R.conv3_cases(tile, kernel=kernel_of(tile)):
        t.run(c)
    t.check("%s conv3 %s" % (kernel_of(tile), R.TILE_NAMES[tile]))


def test_p8_splitk_and_fixup(eng):
    """the 256x256 kernel with the context's workspace: K in {512, 576} x (M, N) in {(257, 256), (549, 260), (100, 8)} -- the only M-tile or
    N-tile partial, nine k-tiles in two slices -- reports the split gemm_ref.expected_split_k restates, the fix-up's result holds the bars
    and two runs are bit-identical; K = 256 reports 1"""
    t = Tally(eng)
    for c in R.p8_splitk_cases():
        want = R.expected_split_k(c, kernel="bf16_p8")
        assert want == (1 if c["K"] == 256 else 2)
        t.run(c, want_split=want, twice=True)
    t.check("bf16_p8 split-K")


def test_p8_agrees_with_the_128x128_tile(eng):
    """the relation test_bf16_p8_layer_matches_oracle states: on the same dense and conv3 cases the two kernels differ by fp32 summation
    order only -- max|p8 - bf16| / max|bf16| < 2^-8, one bf16 ulp of the output"""
    t, worst, missed = Tally(eng), 0.0, []
    for c in R.dense_cases(7, "bf16_p8") + R.conv3_cases(7, kernel="bf16_p8"):
        new, _ = t.run(c)
        old, _ = t.run(dict(c, tile=0, kernel="bf16", w_rows=R.pad_to(c["N"], 128)))
        d = R.rel(new, old)
        worst = max(worst, d)
        if not d < R.BF16_ULP:
            missed.append("%s: %.3e" % (describe(c), d))
    print("bf16_p8 against bf16 128x128: worst %.3e of %d pairs (bar 2^-8 = %.3e)" % (worst, t.n // 2, R.BF16_ULP))
    assert not missed, missed
    t.check("bf16_p8 and bf16 128x128 on the same cases")


def test_kernel_0_is_the_fp32_hook(eng):
    """hpe_debug_gemm_launch with kernel 0 is hpe_debug_gemm_ex: the same bits and the same split_k, with and without the workspace"""
    import torch

    for c in (R.dense_cases(2)[-3], R.splitk_cases(2)[-1]):
        inp = R.inputs(c)
        dev = {k: gpu(inp[k]) for k in ("x", "x2", "wt", "res", "scale", "shift")}
        kw = {k: c[k] for k in GEMM_FIELDS if k in c}
        kw.update(x2=dev["x2"], residual=dev["res"], scale=dev["scale"], shift=dev["shift"])
        ys = [torch.full((c["M"] + 1, c["ldy"]), SENTINEL, dtype=torch.int32, device="cuda") for _ in range(2)]
        sk_ex = eng.debug_gemm_ex(c["mode"], c["tile"], dev["x"], dev["wt"], ys[0].view(torch.float32), **kw)
        sk = eng.debug_gemm_launch(0, c["mode"], c["tile"], dev["x"], dev["wt"], ys[1].view(torch.float32), **kw)
        assert sk == sk_ex == R.expected_split_k(c) and torch.equal(ys[0], ys[1]), (describe_shape(c), sk, sk_ex)
        got = ys[1].cpu().numpy()[: c["M"], : c["N"]].view(np.float32)
        assert R.rel(got, R.reference(c, inp)) <= R.BAR


# ------------------------------------------------------------------------------------------- refused launches
@pytest.mark.parametrize("kernel", ("f32s", "bf16", "bf16_p8"))
def test_rejected_launches(eng, kernel):
    """each clause of the kernel's contract broken once (gemm_ref.error_cases) with a live context and real buffers: HPE_ERR_INVALID, the
    clause named, split_k = 0 and an untouched output.  Nothing is launched, so nothing here can reach the device with a bad shape."""
    import torch

    lib, k = eng.lib, R.KERNELS[kernel]
    bases = {n: dict(b, kernel=kernel) for n, b in R.error_bases(kernel).items() if b["mode"] in k["modes"]}
    held = {}
    for n, b in bases.items():
        inp = R.inputs(b)
        if inp["res"] is None:
            inp["res"] = np.zeros((b["M"] + 1, b["ldres"]), np.float32)
        held[n] = upload(b, inp)
    missed = []
    cases = R.error_cases(kernel)
    for i in range(len(cases)):
        name = cases[i][0] if cases[i][0] in bases else "dense"  # a mode the kernel lacks: any buffers do
        c, null, mis = R.error_case(i, kernel)
        want = R.contract_violations(c, null, mis, kernel=kernel)
        dev, y = held[name], new_output(bases[name])
        ptr = dict(x=dev["x"], x2=dev["x2"], wt=dev["wt"], residual=dev["res"] if c["use_res"] else None, y=y)
        g = _lib.HpeDebugGemm()
        g.struct_size = C.sizeof(_lib.HpeDebugGemm)
        g.mode, g.tile = c["mode"], c["tile"]
        for f in GEMM_FIELDS:
            setattr(g, f, c.get(f, 0))
        for f, tns in ptr.items():
            setattr(g, f, None if tns is None or f in null else tns.data_ptr() + (4 if f in mis else 0))
        g.scale, g.shift = dev["scale"].data_ptr(), dev["shift"].data_ptr()
        sk = C.c_int(-1)
        g.split_k = C.pointer(sk)
        rc = lib.hpe_debug_gemm_launch(eng._h, C.byref(g), k["id"], c.get("w_piece", 0), None)
        msg = lib.hpe_last_error().decode()
        torch.cuda.synchronize()
        bits = y.view(torch.int16 if R.reads_bf16(kernel) else torch.int32)
        ok = len(want) == 1 and rc == 1 and sk.value == 0 and ("contract" in msg or "mode" in msg) and want[0] in msg
        ok = ok and bool((bits == (SENTINEL16 if R.reads_bf16(kernel) else SENTINEL)).all())
        if not ok:
            missed.append((i, cases[i], rc, sk.value, msg))
    assert not missed, missed
