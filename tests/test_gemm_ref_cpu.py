"""CPU checks of tests/gemm_ref.py, the float64 reference and the shape lists of tests/test_gpu_gemm_edges.py:
the references agree with a convolution written by someone else (oracle.hmr_oracle.conv2d_nhwc = torch's conv2d, float64), a float32
restatement on the test's own inputs sits under a quarter of the 5e-6 bar, every listed shape is inside the launcher's contract
and every error case breaks exactly one clause of it.  The same for the lists of tests/test_gpu_bf16_gemm_edges.py (f32s, bf16, bf16_p8):
what the lists hold, the float32 restatement of the bf16 kernels against their bars on every case, and the test-side three-way split of
the f32s weights."""
import numpy as np
import pytest

import gemm_ref as R
from oracle import hmr_oracle as O


def test_strided_reference_is_a_strided_1x1_convolution():
    g = R.rng(901)
    for Hi, Ho, s in R.STRIDED_GEO:
        x, W = R.normal(g, (2, Hi, Hi, 8)), R.normal(g, (5, 8))
        ref = O.conv2d_nhwc(x, W.T.reshape(1, 1, 8, 5), None, s, 0, dtype=np.float64)
        assert ref.shape == (2, Ho, Ho, 5)
        assert np.abs(R.acc_strided(x, W, Ho, Ho, s) - ref.reshape(-1, 5)).max() < 1e-13


def test_conv3_reference_and_packing_are_a_same_convolution():
    g = R.rng(902)
    for H, W in R.CONV3_MAPS:
        x, k = R.normal(g, (2, H, W, 4)), R.normal(g, (3, 3, 4, 6))
        ref = O.conv2d_nhwc(x, k, None, 1, 1, dtype=np.float64).reshape(-1, 6)
        assert np.abs(R.acc_conv3(x, k) - ref).max() < 1e-13
        # the packed rows against the taps gathered in the packing's own k order: k = (kh * 3 + kw) * Cin + ci
        xp = np.pad(x.astype(np.float64), ((0, 0), (1, 1), (1, 1), (0, 0)))
        A = np.concatenate([xp[:, kh : kh + H, kw : kw + W].reshape(-1, 4) for kh in range(3) for kw in range(3)], axis=1)
        Wt = R.pack_3x3(k, 8, 40)
        assert not Wt[6:].any() and not Wt[:, 36:].any()
        assert np.abs(A @ Wt[:6, :36].astype(np.float64).T - ref).max() < 1e-13


def test_dual_reference_is_the_sum_of_two_convolutions():
    g = R.rng(903)
    for Hi, Ho, s in R.DUAL_GEO:
        a, x2 = R.normal(g, (2 * Ho * Ho, 8)), R.normal(g, (2, Hi, Hi, 4))
        W1, W2 = R.normal(g, (5, 8)), R.normal(g, (5, 4))
        ref = O.conv2d_nhwc(a.reshape(2, Ho, Ho, 8), W1.T.reshape(1, 1, 8, 5), None, 1, 0, dtype=np.float64)
        ref = ref + O.conv2d_nhwc(x2, W2.T.reshape(1, 1, 4, 5), None, s, 0, dtype=np.float64)
        assert np.abs(R.acc_dual(a, W1, x2, W2, Ho, Ho, s) - ref.reshape(-1, 5)).max() < 1e-13
        Wt = R.pack_dual(W1, W2, 8, 12)
        assert np.array_equal(Wt[:5, :8], W1) and np.array_equal(Wt[:5, 8:], W2) and not Wt[5:].any()


def test_epilogue_and_slab8_layout():
    acc = np.array([[1.0, -2.0], [3.0, 4.0]])
    y = R.epilogue(acc, [2.0, -1.0], [0.5, 0.25], np.array([[1.0, 1.0], [-10.0, 0.0]]), True)
    assert np.array_equal(y, [[3.5, 3.25], [0.0, 0.0]])
    assert np.array_equal(R.epilogue(acc, [2.0, -1.0], [0.5, 0.25], None, False), [[2.5, 2.25], [6.5, -3.75]])
    M, N = 5, 24
    y = np.arange(M * N, dtype=np.float64).reshape(M, N)
    s = R.to_slab8(y)
    for m in range(M):
        for n in range(N):
            assert s[(n // 8) * M + m, n % 8] == y[m, n]


def test_float32_restatement_is_under_a_quarter_of_the_bar():
    """at the largest K of every block and in the metric of the GPU file (whole matrix, last partial M-tile, last partial N-tile), with
    and without residual and ReLU: the inputs leave an fp32 kernel three quarters of the bar for its own summation order"""
    picks = []
    for t in (2, 6):
        for cases in (R.dense_cases(t), R.strided_cases(t), R.conv3_cases(t), R.dual_cases(t)):
            kmax = max(c["K"] for c in cases)
            picks += [c for c in cases if c["K"] == kmax]
    picks += [c for c in R.splitk_cases(2) if c["K"] == 2048]
    worst = 0.0
    for c in picks:
        inp = R.inputs(c)
        e = R.edge_errors(R.float32_restatement(c, inp), R.reference(c, inp), *R.TILES[c["tile"]])
        worst = max(worst, *e)
        assert max(e) < R.BAR / 4, (c, e)
    assert max(c["K"] for c in picks) == 2048 and any(c["mode"] == R.CONV3 and c["K"] == 9 * 64 for c in picks)
    print("float32 restatement: worst %.2e of %d cases (bar / 4 = %.2e)" % (worst, len(picks), R.BAR / 4))


def test_every_listed_shape_is_inside_the_contract():
    cases = R.all_valid_cases()
    assert len(cases) > 1300
    for c in cases:
        assert R.contract_violations(c) == [], c
        assert c["ldy"] >= c["N"] and (not c["use_res"] or c["ldres"] >= c["N"]), c
        if c["mode"] != R.DENSE:
            assert c["M"] == R.BATCH * c["Ho"] * c["Wo"], c


def test_lists_hold_what_the_issue_asks_for():
    for t, (BM, BN) in R.KERNELS["f32"]["tiles"].items():
        d = R.dense_cases(t)
        assert {c["M"] for c in d} == {1, BM - 1, BM, BM + 1, 2 * BM + 37}
        assert {c["N"] for c in d} == {4, BN - 4, BN, BN + 4, 2 * BN + 20, 85}
        assert {c["K"] for c in d} == {32, 64, 96, 512}
        assert max(c["M"] for c in d) <= R.DENSE_M_MAX and max(c["N"] for c in d) <= R.DENSE_N_MAX
        assert any(c["lda"] > c["K"] and c["ldy"] > c["N"] and c["use_res"] and c["ldres"] != c["ldy"] for c in d)
        assert all((c["ldy"], c["ldres"], c["w_rows"]) == (R.THETA_LD, R.THETA_LD, 128) for c in d if c["N"] == 85)
        for cases in (d, R.strided_cases(t), R.conv3_cases(t)):
            assert {(c["use_res"], c["relu"]) for c in cases} == {(0, 0), (0, 1), (1, 0), (1, 1)}
            for N in {c["N"] for c in cases}:  # residual and ReLU both ways at every width
                assert {c["use_res"] for c in cases if c["N"] == N} == {0, 1} and {c["relu"] for c in cases if c["N"] == N} == {0, 1}
        assert {c["relu"] for c in R.dual_cases(t)} == {0, 1} and not any(c["use_res"] for c in R.dual_cases(t))
        assert len(R.strided_cases(t)) == 12 and len(R.conv3_cases(t)) == 20 and len(R.dual_cases(t)) == 16
    assert 147 in {c["M"] for c in R.strided_cases(0)}
    for t in R.SPLIT_TILES:
        s = R.splitk_cases(t)
        assert len(s) == 27 and all(R.expected_split_k(c) > 1 for c in s)
        assert R.expected_split_k(next(c for c in s if c["K"] == 288)) == 2  # 9 slabs in 2 slices: 4 + 5
    assert all(R.expected_split_k(c) > 1 for c in R.conv3_cases(2, use_splitk=1) if c["K"] >= 256)
    for t in R.SLAB8_TILES:
        assert {c["N"] for c in R.slab8_cases(t)} == {8, 72, R.TILES[t][1] + 8}


def test_error_case_breaks_exactly_one_clause():
    for base in R.error_bases().values():
        assert R.contract_violations(base) == [], base
    for i in range(len(R.ERROR_CASES)):
        c, null, mis = R.error_case(i)
        bad = R.contract_violations(c, null, mis)
        assert len(bad) == 1, (i, c, bad)


def test_error_cases_cover_the_contract():
    """every clause the restatement knows is broken by some case, but for the two that the other clauses imply"""
    import inspect
    import re

    every = set(re.findall(r'clause\("([^"]+)"', inspect.getsource(R.contract_violations)))
    every |= {n + " != NULL" for n in ("x", "wt", "y")}
    seen = set()
    for i in range(len(R.ERROR_CASES)):
        seen.update(R.contract_violations(*R.error_case(i)))
    assert len(every) > 35 and seen <= every
    assert every - seen == {"Cin % 4 == 0", "Cin % 32 == 0"}, every - seen


# ------------------------------------------------------------------------------------------- f32s, bf16, bf16_p8
OTHERS = ("f32s", "bf16", "bf16_p8")
PREFETCH_TILES = {"bf16": (1, 2, 3, 4, 5)}  # conv_gemm_bf16.hip: R_PRE = at most four row passes per thread in the epilogue


@pytest.mark.parametrize("kernel", OTHERS)
def test_other_kernels_lists_hold_what_the_issue_asks_for(kernel):
    k = R.KERNELS[kernel]
    S, G = k["slab"], k["gran"]
    for t, (BM, BN) in k["tiles"].items():
        d = R.dense_cases(t, kernel)
        assert {c["M"] for c in d} == {1, BM - 1, BM, BM + 1, 2 * BM + 37}
        assert {c["N"] for c in d} == {4, BN - 4, BN, BN + 4, 2 * BN + 20, 85}
        assert {c["K"] for c in d} == ({64, 128, 192, 512} if S == 64 else {32, 64, 96, 512})
        assert all(c["M"] <= c["master"][0] and c["N"] <= c["master"][1] for c in d)
        assert any(c["lda"] > c["K"] and c["ldy"] > c["N"] and c["use_res"] and c["ldres"] != c["ldy"] for c in d)
        assert all(c["ldy"] > c["N"] and c["ldy"] == c["ldres"] == R.THETA_LD for c in d if c["N"] == 85)
        assert all(c["ldy"] > c["N"] and c["ldy"] % G == 0 and c["ldres"] % G == 0 and c["lda"] % G == 0 for c in d)
        for K in {c["K"] for c in d}:  # every K with an M tail and an N tail in one workgroup
            assert any(c["K"] == K and c["M"] % BM and c["N"] % BN for c in d)
        if t in PREFETCH_TILES.get(kernel, ()):  # the prefetched residual with both tails in the same workgroup, a partial 8-group among its columns
            assert any(c["use_res"] and c["M"] % BM and c["N"] % BN and c["N"] % 8 and c["N"] > 8 for c in d), t
        lists = [d, R.strided_cases(t, kernel)] + ([R.conv3_cases(t, kernel=kernel)] if R.CONV3 in k["modes"] else [])
        for cases in lists:
            assert {(c["use_res"], c["relu"]) for c in cases} == {(0, 0), (0, 1), (1, 0), (1, 1)}
            for N in {c["N"] for c in cases}:
                assert {c["use_res"] for c in cases if c["N"] == N} == {0, 1} and {c["relu"] for c in cases if c["N"] == N} == {0, 1}
        s, du = R.strided_cases(t, kernel), R.dual_cases(t, kernel)
        assert len(s) == 12 and {c["Cin"] for c in s} == {S, 3 * S} and {(c["Hi"], c["Ho"], c["stride"]) for c in s} == set(R.STRIDED_GEO)
        assert len(du) == 16 and {c["k1_slabs"] for c in du} == {1, 3} and {c["Cin"] for c in du} == {S, 3 * S} and {c["relu"] for c in du} == {0, 1}
        assert all(c["K"] == c["k1_slabs"] * S + c["Cin"] for c in du) and any(c["lda"] > c["k1_slabs"] * S for c in du)
        if R.CONV3 in k["modes"]:
            c3 = R.conv3_cases(t, kernel=kernel)
            assert len(c3) == 20 and {(c["Hi"], c["Wi"]) for c in c3} == set(R.CONV3_MAPS) and {c["N"] for c in c3} == {64, 192}
            assert {c["Cin"] for c in c3} == ({64, 192} if kernel == "bf16" else {64, 128})
        for c in d + s + du:
            if kernel == "bf16_p8":
                assert c["w_rows"] == c["N"] and (c["N"] >= 256 or c["w_rows"] < 256), c
            if kernel == "f32s":
                assert c["w_piece"] in (c["K"], c["K"] + 8) and c["ldw"] == c["K"] + 2 * c["w_piece"], c
        if kernel == "f32s":
            for cases in (d, s, du):
                assert {c["w_piece"] - c["K"] for c in cases} == {0, 8}
            assert any(c["k1_slabs"] == 1 and c["w_piece"] > c["K"] for c in du)
    assert len(R.all_valid_cases(kernel)) == {"f32s": 3 * 148, "bf16": 7 * 168, "bf16_p8": 168 + 7}[kernel]


def test_p8_splitk_table():
    """K in {512, 576} x (M, N) in {(257, 256), (549, 260), (100, 8)}: every case splits, 576 = nine k-tiles in two slices; K = 256 does not"""
    cases = R.p8_splitk_cases()
    assert [(c["K"], c["M"], c["N"]) for c in cases] == [(K, M, N) for K in (512, 576) for M, N in ((257, 256), (549, 260), (100, 8))] + [(256, 257, 256)]
    assert [R.expected_split_k(c, kernel="bf16_p8") for c in cases] == [2, 2, 2, 2, 2, 2, 1]
    assert all(c["use_splitk"] and (c["M"] % 256 or c["N"] % 256) and c["w_rows"] == c["N"] for c in cases)
    assert {c["use_res"] for c in cases} == {0, 1} and {c["relu"] for c in cases} == {0, 1} and any(c["lda"] > c["K"] for c in cases)
    assert R.expected_split_k(dict(cases[0], use_splitk=0), kernel="bf16_p8") == 1
    assert R.expected_split_k(dict(cases[0], K=4096), kernel="bf16_p8") == 8 and R.expected_split_k(dict(cases[0], K=4096), 2 * 3 * 65536, "bf16_p8") == 3
    assert all(R.expected_split_k(c, kernel=k) == 1 for k in ("f32s", "bf16") for c in R.all_valid_cases(k)[::7])


def test_three_way_split_reproduces_every_weight():
    """w0 + w1 + w2 == w in float64 for every weight of every f32s case, each piece a bf16 value, and the packed rows hold piece j of
    Wt[n][k] at n * ldw + j * w_piece + k with nothing of a weight between or after the pieces"""
    n = 0
    for c in R.all_valid_cases("f32s"):
        inp = R.inputs(c)
        W, wt, K, N, wp = inp["W"], inp["wt"], c["K"], c["N"], c["w_piece"]
        assert wt.shape == (c["w_rows"], c["ldw"]) and np.array_equal(R.bf16_round(wt), wt)
        pieces = [wt[:N, j * wp : j * wp + K].astype(np.float64) for j in range(3)]
        assert np.array_equal(pieces[0] + pieces[1] + pieces[2], W.astype(np.float64)), c
        assert np.array_equal(pieces[0], R.bf16_round(W)) and np.abs(pieces[1]).max() <= np.abs(pieces[0]).max() * 2.0 ** -8
        assert not wt[N:].any()
        if wp > K:
            assert (wt[:N, K:wp] == R.SPLIT_GAP).all() and (wt[:N, wp + K : 2 * wp] == R.SPLIT_GAP).all()
        n += W.size
    assert n > 1e6


def test_f32s_restatement_is_under_a_quarter_of_the_bar():
    """the f32s lists share the fp32 kernel's bar; at the largest K of every block the float32 restatement leaves three quarters of it"""
    worst, n = 0.0, 0
    for t in R.KERNELS["f32s"]["tiles"]:
        for cases in (R.dense_cases(t, "f32s"), R.strided_cases(t, "f32s"), R.dual_cases(t, "f32s")):
            kmax = max(c["K"] for c in cases)
            for c in cases:
                if c["K"] == kmax:
                    inp = R.inputs(c)
                    e = R.edge_errors(R.float32_restatement(c, inp), R.reference(c, inp), *R.TILES[t])
                    worst, n = max(worst, *e), n + 1
                    assert max(e) < R.BAR / 4, (c, e)
    print("f32s float32 restatement: worst %.2e of %d cases (bar / 4 = %.2e)" % (worst, n, R.BAR / 4))


@pytest.mark.parametrize("kernel", ("bf16", "bf16_p8"))
def test_bf16_restatement_is_within_its_bars(kernel):
    """bf16 operands, float32 accumulation in NumPy, fp32 epilogue, one final rounding to bf16: on EVERY case of the kernel this stays
    inside both checks of the GPU file (gemm_ref.bf16_figures / bf16_misses) -- the reference alone passes its own bars.  Every input is a
    bf16 value.  Prints the range of e32 and counts the blocks whose rel-L2 bar is the format's 2^-8: all of them hold four elements."""
    cases = R.all_valid_cases(kernel)
    e32s, worst, small, missed = [], [0.0, 0.0, 0.0], [], []
    for c in cases:
        inp = R.inputs(c)
        for k in ("x", "x2", "wt", "res"):
            assert inp[k] is None or np.array_equal(R.bf16_round(inp[k]), inp[k]), (k, c)
        pre = R.float32_restatement(c, inp)
        e32, figs = R.bf16_figures(c, inp, R.bf16_round(pre))
        e32s.append(e32)
        missed += ["%s: %s" % (c, m) for m in R.bf16_misses(figs)]
        for b, f in zip(R.edge_blocks(c["M"], c["N"], *R.TILES[c["tile"]]), figs):
            if f is not None:
                worst = [max(w, v) for w, v in zip(worst, f[:3])]
                if f[3] != R.BF16_L2:
                    small.append((b[0].stop - b[0].start) * (b[1].stop - b[1].start))
    assert not missed, missed[:10]
    assert all(n <= 4 for n in small) and len(small) <= len(cases) // 100, small
    assert all(e > 0 for c, e in zip(cases, e32s) if not c["relu"]) and max(e32s) < 2.0 ** -20  # fp32 accumulation: a few 2^-24, never a bf16 step
    print("%s restatement: %d cases, e32 %.2e .. %.2e, worst max-normalised %.2e, rel-L2 %.2e, element/bound %.2f; %d blocks of <= 4 elements at the 2^-8 rel-L2 bar"
          % (kernel, len(cases), min(e for e in e32s if e > 0), max(e32s), worst[0], worst[1], worst[2], len(small)))
