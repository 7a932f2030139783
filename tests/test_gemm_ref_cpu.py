"""CPU checks of tests/gemm_ref.py, the float64 reference and the shape lists of tests/test_gpu_gemm_edges.py:
the references agree with a convolution written by someone else (oracle.hmr_oracle.conv2d_nhwc = torch's conv2d, float64), a float32
restatement on the test's own inputs sits under a quarter of the 5e-6 bar, every listed shape is inside the launcher's contract
and every error case breaks exactly one clause of it."""
import numpy as np

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
    for t, (BM, BN) in enumerate(R.TILES):
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
