"""float64 references of the four implicit-GEMM kernels (conv_gemm.hip, conv_gemm_f32s.hip, conv_gemm_bf16.hip, conv_gemm_bf16_p8.hip),
written from the definition

    y[m][n] = act((sum_k A[m][k] * Wt[n][k]) * scale[n] + shift[n] (+ res[m][n]))

for its four product modes, the weight packing the kernels read, seeded inputs, the shape lists of tests/test_gpu_gemm_edges.py (fp32)
and tests/test_gpu_bf16_gemm_edges.py (the other three: every generator takes the kernel's name) and a restatement of the host-side contract of the four GEMM launchers (csrc/gemm_contract.h).  Plain NumPy, no GPU, nothing taken from the library:
tests/test_gemm_ref_cpu.py pins the references to oracle.hmr_oracle.conv2d_nhwc, the inputs to the bar and the lists to the contract.

Packed weights Wt[n][k], w_rows x ldw, zero padded:  1x1 layers k = ci;  3x3 layers k = (kh * 3 + kw) * Cin + ci;  dual: the k
range of the dense source followed by the k range of the strided source.

The bf16 kernels (bf16, bf16_p8) get float32 inputs that are exactly representable in bf16 (rounded with torch.bfloat16), so the float64
reference is of the very operands the kernel reads; scale and shift stay fp32.  f32s reads fp32 activations and weights split into three
bf16 pieces (split3_rows).
"""
import functools

import numpy as np

DENSE, STRIDED, CONV3, STEM, DUAL = 0, 1, 2, 3, 4
TILES = ((128, 128), (128, 64), (64, 64), (64, 128), (128, 128), (128, 64), (256, 128), (256, 256))  # (BM, BN) of tile 0..7; 7: bf16_p8 only
TILE_NAMES = ("128x128", "128x64", "64x64", "64x128", "128x128_W8", "128x64_W8", "256x128_W8", "256x256_P8")
SPLIT_TILES = (0, 1, 2, 3)  # the 4-wave tiles: the only ones the launcher cuts along K
W8_TILES = (4, 5, 6)
BK = 32
SPLITK_MIN_SLABS = 4  # the plan's default (HPE_SPLITK_SLABS)
BAR = 5e-6  # the project's single-conv bar (test_conv_layer_matches_oracle): max|got - ref| / max|ref|
THETA_LD = 96  # pitch of the regressor's theta rows: run_dense writes its N = 85 layer at this pitch


def pad_to(n, b):
    return (n + b - 1) // b * b


# ------------------------------------------------------------------------------------------- references
def epilogue(acc, scale, shift, res, relu):
    """acc [M,N] float64 -> act(acc * scale + shift (+ res))"""
    N = acc.shape[1]
    y = acc * np.asarray(scale, np.float64)[:N] + np.asarray(shift, np.float64)[:N]
    if res is not None:
        y = y + np.asarray(res, np.float64)[: acc.shape[0], :N]
    return np.maximum(y, 0.0) if relu else y


def acc_dense(A, W):
    """A [M,K], W [N,K] -> [M,N] in float64"""
    return np.asarray(A, np.float64) @ np.asarray(W, np.float64).T


def gather_strided(x, Ho, Wo, stride):
    """x [B,Hi,Wi,C] -> rows [B*Ho*Wo, C]: pixel (ho * stride, wo * stride) of every image, (b, ho, wo) flattened"""
    B, _, _, C = x.shape
    rows = np.empty((B, Ho, Wo, C), x.dtype)
    for ho in range(Ho):
        for wo in range(Wo):
            rows[:, ho, wo, :] = x[:, ho * stride, wo * stride, :]
    return rows.reshape(B * Ho * Wo, C)


def acc_strided(x, W, Ho, Wo, stride):
    """1x1 convolution with a stride, no padding: x [B,Hi,Wi,Cin], W [N,Cin] -> [B*Ho*Wo, N]"""
    return acc_dense(gather_strided(x, Ho, Wo, stride), W)


def acc_conv3(x, hwio):
    """3x3 / stride 1 / SAME with zero padding around EACH image: x [B,H,W,Cin], hwio [3,3,Cin,N] -> [B*H*W, N]"""
    B, H, W, C = x.shape
    xp = np.zeros((B, H + 2, W + 2, C), np.float64)
    xp[:, 1 : H + 1, 1 : W + 1, :] = x
    k = np.asarray(hwio, np.float64)
    acc = np.zeros((B, H, W, k.shape[3]), np.float64)
    for kh in range(3):
        for kw in range(3):
            acc += xp[:, kh : kh + H, kw : kw + W, :] @ k[kh, kw]
    return acc.reshape(B * H * W, -1)


def acc_dual(a, W1, x2, W2, Ho, Wo, stride):
    """dense source a [M,K1] . W1 [N,K1] plus strided source x2 [B,Hi,Wi,Cin] . W2 [N,Cin], M = B*Ho*Wo"""
    return acc_dense(a, W1) + acc_strided(x2, W2, Ho, Wo, stride)


def to_slab8(y):
    """row-major [M,N] (N % 8 == 0) -> channel-slab major [(n / 8) * M + m][n % 8], as GemmArgs::y_slab8 writes it"""
    M, N = y.shape
    return np.ascontiguousarray(y.reshape(M, N // 8, 8).transpose(1, 0, 2)).reshape(N // 8 * M, 8)


# ------------------------------------------------------------------------------------------- packing
def pack_rows(W, w_rows, ldw):
    """W [N,K] -> float32 [w_rows, ldw], zero padded"""
    N, K = W.shape
    out = np.zeros((w_rows, ldw), np.float32)
    out[:N, :K] = W
    return out


def pack_3x3(hwio, w_rows, ldw):
    """hwio [3,3,Cin,N] -> Wt[n][(kh * 3 + kw) * Cin + ci]"""
    _, _, C, N = hwio.shape
    W = np.empty((N, 9 * C), np.float32)
    for kh in range(3):
        for kw in range(3):
            for ci in range(C):
                W[:, (kh * 3 + kw) * C + ci] = hwio[kh, kw, ci, :]
    return pack_rows(W, w_rows, ldw)


def pack_dual(W1, W2, w_rows, ldw):
    return pack_rows(np.concatenate([W1, W2], axis=1), w_rows, ldw)


# ------------------------------------------------------------------------------------------- inputs
def rng(*key):
    return np.random.Generator(np.random.Philox(key=[int(sum((k + 1) * 1000003 ** i for i, k in enumerate(key))) % (1 << 63), 17]))


def normal(g, shape, sigma=1.0):
    """signed normal data: ReLU cuts about half of the outputs and a leaked halo tap is never hidden by a zero"""
    return (g.normal(0, 1, shape) * sigma).astype(np.float32)


def weights(g, N, K):
    """N(0, 1/K): the accumulators come out N(0, 1), the size of shift and of the residual, so no term of the epilogue is hidden"""
    return normal(g, (N, K), 1.0 / np.sqrt(K))


def scale_shift(g, N):
    """scale in +-[0.5, 2], shift normal: a different pair in every column"""
    sc = (g.uniform(0.5, 2.0, N) * np.where(g.integers(0, 2, N) == 0, -1.0, 1.0)).astype(np.float32)
    return sc, normal(g, (N,))


# ------------------------------------------------------------------------------------------- metric
def rel(got, ref):
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max() / (np.abs(ref).max() + 1e-30))


def edge_errors(got, ref, BM, BN):
    """(whole matrix, rows of the last partial M-tile, columns of the last partial N-tile): each block over its OWN largest
    reference entry, so that an edge error is not diluted by the rest of the matrix.  A block that does not exist gives 0."""
    M, N = ref.shape
    e = [rel(got, ref), 0.0, 0.0]
    if M % BM:
        e[1] = rel(got[M // BM * BM :], ref[M // BM * BM :])
    if N % BN:
        e[2] = rel(got[:, N // BN * BN :], ref[:, N // BN * BN :])
    return tuple(e)


# ------------------------------------------------------------------------------------------- the shape lists of the GPU files
# Every generator takes the kernel's name (KERNELS below).  What changes with it: the k-slab S (32: f32, f32s; 64: bf16, bf16_p8), the
# elements per 16-byte vector G of the activations, residual and output (4 / 8), the tile set, for f32s the three-piece weight rows
# (w_piece, ldw = K + 2 * w_piece) and for bf16_p8 w_rows = N (the kernel clamps the weight rows it reads, none is padded for it).
# kernel="f32" gives the lists test_gpu_gemm_edges.py has always run.
DENSE_K = (32, 64, 96, 512)  # one slab, two, an odd count, many -- in slabs of 32
DENSE_K64 = (64, 128, 192, 512)  # the same in slabs of 64: one (the ring primes min(NS - 1, S) buffers), two, three (odd: leaves the unrolled body), eight


def slab(kernel):
    return KERNELS[kernel]["slab"]


def dense_k(kernel="f32"):
    return DENSE_K if slab(kernel) == 32 else DENSE_K64


def _mix(i, n_widths):
    """case number -> a counter whose bits change along the width loop (the innermost, n_widths long) AND along the loops around it,
    so that residual, ReLU and the pitches are not tied to one width"""
    return i // n_widths + i % n_widths


def dense_m(BM):
    return (1, BM - 1, BM, BM + 1, 2 * BM + 37)


def dense_n(BN):
    return (4, BN - 4, BN, BN + 4, 2 * BN + 20, 85)


DENSE_M_MAX = 2 * 256 + 37
DENSE_N_MAX = 2 * 128 + 20
DENSE_N_MAX_P8 = 2 * 256 + 20
DENSE_W_ROWS = pad_to(DENSE_N_MAX, 128)


def dense_master(kernel):
    """(Mmax, Nmax) of the draw the dense cases of a kernel are corners of"""
    return (DENSE_M_MAX, DENSE_N_MAX_P8 if slab(kernel) == 64 else DENSE_N_MAX)


def _weights_of(c, kernel, BN, j):
    """the weight fields of a case: w_rows, ldw and, for f32s, w_piece in {K, K + 8} by the bit j"""
    K, N = c["K"], c["N"]
    c["w_rows"] = N if kernel == "bf16_p8" else pad_to(N, BN)
    c["ldw"] = K
    if kernel != "f32":
        c["kernel"] = kernel
    if kernel == "f32s":
        c["w_piece"] = K + 8 * (j & 1)
        c["ldw"] = K + 2 * c["w_piece"]
    return c


def dense_cases(tile, kernel="f32"):
    """every (M, N, K) of the dense block on one tile; the pitches, residual and ReLU cycle with the case number so that each tile
    sees lda > K with ldy > N and ldres != ldy, and all four (residual, ReLU) pairs, many times over.  N = 85 always runs at
    run_dense's pitch: ldy = ldres = THETA_LD, w_rows = 128 (bf16_p8: 85)."""
    BM, BN = TILES[tile]
    G = KERNELS[kernel]["gran"]
    out = []
    i = 0
    for K in dense_k(kernel):
        for M in dense_m(BM):
            for N in dense_n(BN):
                m = _mix(i, 6)
                c = dict(mode=DENSE, tile=tile, M=M, N=N, K=K, relu=(m >> 1) & 1, use_res=m & 1,
                         lda=K + 2 * G * ((m >> 2) % 3 == 1), ldy=pad_to(N, G) + G + G * ((m >> 3) & 1), ldres=pad_to(N, G) + 3 * G)
                _weights_of(c, kernel, BN, m >> 2)
                if N == 85:
                    c.update(ldy=THETA_LD, ldres=THETA_LD)
                    if kernel != "bf16_p8":
                        c.update(w_rows=128)
                if kernel != "f32":
                    c["master"] = dense_master(kernel)
                out.append(c)
                i += 1
    return out


SLAB8_TILES = (1, 4)


def slab8_cases(tile):
    BM, BN = TILES[tile]
    return [dict(mode=DENSE, tile=tile, M=M, N=N, K=64, lda=64, ldw=64, ldy=N, ldres=N + 4, w_rows=pad_to(N, BN), relu=_mix(i, 3) & 1, use_res=(_mix(i, 3) >> 1) & 1,
                 y_slab8=1, master=(257, 136))
            for i, (M, N) in enumerate((M, N) for M in (BM + 1, 37) for N in (8, 72, BN + 8))]


SPLITK_M, SPLITK_N, SPLITK_K = (1, 5, 65), (64, 85, 200), (256, 288, 2048)


def splitk_cases(tile):
    BN = TILES[tile][1]
    out = []
    for i, (K, M, N) in enumerate((K, M, N) for K in SPLITK_K for M in SPLITK_M for N in SPLITK_N):
        out.append(dict(mode=DENSE, tile=tile, M=M, N=N, K=K, lda=K, ldw=K, ldy=pad_to(N, 4) + 4, ldres=pad_to(N, 4) + 8, w_rows=pad_to(N, BN),
                        relu=(_mix(i, 3) >> 1) & 1, use_res=_mix(i, 3) & 1, use_splitk=1, master=(65, 200)))
    return out


def w8_splitk_cases():
    """an 8-wave tile handed the workspace must not split: one shape per tile that a 4-wave tile would cut in 16"""
    return [dict(mode=DENSE, tile=t, M=65, N=200, K=2048, lda=2048, ldw=2048, ldy=204, ldres=208, w_rows=256, relu=1, use_res=1, use_splitk=1,
                 master=(65, 200)) for t in W8_TILES]


P8_SPLITK_K, P8_SPLITK_MN = (512, 576), ((257, 256), (549, 260), (100, 8))  # 576: nine k-tiles in two slices (5 + 4); every (M, N) ends in a partial tile


def p8_splitk_cases():
    """the 256x256 kernel with the workspace: the only M-tile or N-tile partial, K the slices do and do not divide; last, K = 256
    (four k-tiles, below the launcher's eight), which must report split_k == 1"""
    out = []
    for i, (K, (M, N)) in enumerate([(K, mn) for K in P8_SPLITK_K for mn in P8_SPLITK_MN] + [(256, (257, 256))]):
        out.append(dict(mode=DENSE, tile=7, M=M, N=N, K=K, lda=K + 16 * (i & 1), ldw=K, ldy=pad_to(N, 8) + 8, ldres=pad_to(N, 8) + 24, w_rows=N,
                        relu=(i >> 1) & 1, use_res=1 - (i & 1) if i < 6 else 1, use_splitk=1, kernel="bf16_p8", master=dense_master("bf16_p8")))
    return out


def expected_split_k(c, partial_floats=512 * 128 * 128, kernel="f32"):
    """the launcher's choice as written in launch_cfg (conv_gemm.hip) or, for bf16_p8, in launch_p8 (conv_gemm_bf16_p8.hip): the CPU
    check that every split-K case really splits, and what the GPU tests ask the launcher to report.  f32s and bf16 never split."""
    BM, BN = TILES[c["tile"]]
    grid = pad_to(c["M"], BM) // BM * (pad_to(c["N"], BN) // BN)
    if kernel == "bf16_p8":
        S = c["K"] // 64
        if not c.get("use_splitk") or grid > 160 or S < 8:  # about one workgroup per CU, at least four k-tiles per slice
            return 1
        sk = min((256 + grid - 1) // grid, S // 4, 8)
        while sk > 1 and grid * sk * BM * BN > partial_floats:
            sk -= 1
        while sk > 1 and (S + sk - 1) // sk * (sk - 1) >= S:  # every slice owns at least one k-tile
            sk -= 1
        return max(sk, 1)
    if kernel != "f32" or c["tile"] not in SPLIT_TILES or not c.get("use_splitk"):
        return 1
    S = c["K"] // BK
    if grid >= 128 or S < 2 * SPLITK_MIN_SLABS:
        return 1
    sk = min(256 // grid, S // SPLITK_MIN_SLABS, 16)
    while sk > 1 and grid * sk * BM * BN > partial_floats:
        sk -= 1
    return max(sk, 1)


BATCH = 3
STRIDED_GEO = ((6, 3, 2), (14, 7, 2), (7, 7, 1))  # (Hi, Ho, stride); (14, 7, 2): M = 147 crosses a 128-row tile inside an image


def strided_cin(kernel="f32"):
    return (slab(kernel), 3 * slab(kernel))  # one slab and an odd count


def strided_cases(tile, kernel="f32"):
    BN = TILES[tile][1]
    G = KERNELS[kernel]["gran"]
    out = []
    for i, (geo, Cin, N) in enumerate((g, c, n) for g in STRIDED_GEO for c in strided_cin(kernel) for n in (64, 132)):
        Hi, Ho, s = geo
        c = dict(mode=STRIDED, tile=tile, M=BATCH * Ho * Ho, N=N, K=Cin, Cin=Cin, Hi=Hi, Wi=Hi, Ho=Ho, Wo=Ho, stride=s, lda=Cin,
                 ldy=pad_to(N, G) + G, ldres=pad_to(N, G) + 2 * G, relu=(_mix(i, 2) >> 1) & 1, use_res=_mix(i, 2) & 1)
        out.append(_weights_of(c, kernel, BN, i >> 2))
    return out


CONV3_MAPS = ((1, 1), (3, 3), (7, 7), (14, 14), (5, 7))  # (H, W); (5, 7): inside the launcher's contract, outside the product's use


def conv3_cin(kernel="f32"):
    """f32: one and two slabs per tap; bf16: one and three (not a power of two: legal there); bf16_p8: one and two (three is refused)"""
    return {"f32": (32, 64), "bf16": (64, 192), "bf16_p8": (64, 128)}[kernel]


def conv3_cases(tile, use_splitk=0, kernel="f32"):
    BN = TILES[tile][1]
    G = KERNELS[kernel]["gran"]
    out = []
    for i, (hw, Cin, N) in enumerate((m, c, n) for m in CONV3_MAPS for c in conv3_cin(kernel) for n in (64, 192)):
        H, W = hw
        c = dict(mode=CONV3, tile=tile, M=BATCH * H * W, N=N, K=9 * Cin, Cin=Cin, Hi=H, Wi=W, Ho=H, Wo=W, stride=1, lda=Cin,
                 ldy=N + G, ldres=N + 2 * G, relu=(_mix(i, 2) >> 1) & 1, use_res=_mix(i, 2) & 1, use_splitk=use_splitk)
        out.append(_weights_of(c, kernel, BN, 0))
    return out


DUAL_GEO = ((7, 7, 1), (14, 7, 2))


def dual_cin(kernel="f32"):
    return {"f32": (32, 64), "f32s": (32, 96), "bf16": (64, 192), "bf16_p8": (64, 192)}[kernel]


def dual_cases(tile, kernel="f32"):
    BN = TILES[tile][1]
    G, S = KERNELS[kernel]["gran"], slab(kernel)
    out = []
    for i, (geo, k1, Cin, N) in enumerate((g, k, c, n) for g in DUAL_GEO for k in (1, 3) for c in dual_cin(kernel) for n in (128, 260)):
        Hi, Ho, s = geo
        K = k1 * S + Cin
        c = dict(mode=DUAL, tile=tile, M=BATCH * Ho * Ho, N=N, K=K, Cin=Cin, Hi=Hi, Wi=Hi, Ho=Ho, Wo=Ho, stride=s, k1_slabs=k1,
                 lda=k1 * S + 8 * (_mix(i, 2) & 1), ldy=pad_to(N, G) + G, ldres=pad_to(N, G) + G, relu=(_mix(i, 2) >> 1) & 1, use_res=0)
        out.append(_weights_of(c, kernel, BN, i >> 1))
    return out


def all_valid_cases(kernel="f32"):
    k = KERNELS[kernel]
    out = []
    for t in k["tiles"]:
        out += dense_cases(t, kernel) + strided_cases(t, kernel) + dual_cases(t, kernel)
        if CONV3 in k["modes"]:
            out += conv3_cases(t, kernel=kernel)
    if kernel == "bf16_p8":
        out += p8_splitk_cases()
    if kernel != "f32":
        return out
    for t in SLAB8_TILES:
        out += slab8_cases(t)
    for t in SPLIT_TILES:
        out += splitk_cases(t)
    out += conv3_cases(2, use_splitk=1)
    out += w8_splitk_cases()
    return out


# ------------------------------------------------------------------------------------------- the launchers' contract
POINTERS = ("x", "x2", "wt", "residual", "y")
# The four launchers (csrc/gemm_contract.h), by the number hpe_debug_gemm_check takes: elements per 16-byte vector of the activations
# (gran) and of the weights (wgran), elements per k-slab, the modes the debug hooks can ask of the kernel and its tiles {id: (BM, BN)}.
KERNELS = {
    "f32": dict(id=0, gran=4, wgran=4, slab=32, modes=(DENSE, STRIDED, CONV3, DUAL), tiles={t: TILES[t] for t in range(7)}),
    "f32s": dict(id=1, gran=4, wgran=8, slab=32, modes=(DENSE, STRIDED, DUAL), tiles={t: TILES[t] for t in (0, 4, 6)}),
    "bf16": dict(id=2, gran=8, wgran=8, slab=64, modes=(DENSE, STRIDED, CONV3, DUAL), tiles={t: TILES[t] for t in range(7)}),
    "bf16_p8": dict(id=3, gran=8, wgran=8, slab=64, modes=(DENSE, STRIDED, CONV3, DUAL), tiles={7: TILES[7]}),
}
TILE_CLAUSE = {"f32": "tile in 0..6", "f32s": "tile in {0, 4, 6}", "bf16": "tile in 0..6", "bf16_p8": "tile == 7"}
# contract_violations writes every clause under the fp32 launcher's name; these tables give the names of the clauses whose number is
# the kernel's slab (64), its activation vector (8) or its weight vector (8) instead
SLAB64_NAMES = {"K % 32 == 0": "K % 64 == 0", "Cin % 32 == 0": "Cin % 64 == 0", "k1_slabs * 32 < K": "k1_slabs * 64 < K",
                "lda >= k1_slabs * 32": "lda >= k1_slabs * 64", "Cin == K - k1_slabs * 32": "Cin == K - k1_slabs * 64"}
VEC8_NAMES = {"ldy % 4 == 0": "ldy % 8 == 0", "ldres % 4 == 0": "ldres % 8 == 0", "lda % 4 == 0": "lda % 8 == 0", "Cin % 4 == 0": "Cin % 8 == 0"}
WVEC8_NAMES = {"ldw % 4 == 0": "ldw % 8 == 0"}
CLAUSE_NAMES = {"f32": {}, "f32s": dict(WVEC8_NAMES), "bf16": {**SLAB64_NAMES, **VEC8_NAMES, **WVEC8_NAMES}}
CLAUSE_NAMES["bf16_p8"] = CLAUSE_NAMES["bf16"]


def clause_name(name, kernel):
    """the fp32 launcher's name of a clause -> the name of the same clause of `kernel`"""
    return TILE_CLAUSE[kernel] if name == "tile in 0..6" else CLAUSE_NAMES[kernel].get(name, name)


def contract_violations(c, null=(), misaligned=(), kernel="f32"):
    """The clauses of a launcher's host-side contract (gemm_contract.h; default: hpe_launch_gemm, the fp32 kernel) that the launch c
    breaks, by name.  Pointers are described, not held: a case has x, wt and y, residual with use_res and x2 in dual mode, minus `null`;
    the ones in `misaligned` are not multiples of 16 bytes.  scale, shift and the zero page come from the hook and are never NULL.
    The clauses are written with the fp32 kernel's numbers in their names; clause_name() turns them into the other kernels'."""
    k = KERNELS[kernel]
    G, WG, SLAB = k["gran"], k["wgran"], k["slab"]
    g = dict(lda=0, ldw=0, ldy=0, ldres=0, w_rows=0, Hi=0, Wi=0, Cin=0, Ho=0, Wo=0, stride=0, k1_slabs=0, y_slab8=0, w_piece=0)
    g.update(c)
    has = {"x": True, "wt": True, "y": True, "residual": bool(g.get("use_res")), "x2": g["mode"] == DUAL}
    for n in null:
        has[n] = False
    bad = []

    def clause(name, broken):
        if broken:
            bad.append(clause_name(name, kernel))

    def only(which, name, broken):  # a clause that only the kernel `which` has
        if kernel == which and broken:
            bad.append(name)

    M, N, K = g["M"], g["N"], g["K"]
    clause("M > 0", M <= 0)
    clause("N > 0", N <= 0)
    clause("K > 0", K <= 0)
    clause("K % 32 == 0", K > 0 and K % SLAB != 0)
    clause("ldw % 4 == 0", g["ldw"] % WG != 0)
    if kernel == "f32s":  # three bf16 pieces per weight row
        only("f32s", "w_piece % 8 == 0", g["w_piece"] % 8 != 0)
        only("f32s", "w_piece >= K", g["w_piece"] < K)
        only("f32s", "ldw >= K + 2 * w_piece", g["ldw"] < K + 2 * g["w_piece"])
    else:
        clause("ldw >= K", g["ldw"] < K)
    for n in ("x", "wt", "y"):
        clause(n + " != NULL", not has[n])
    clause("ldy % 4 == 0", g["ldy"] % G != 0)
    clause("y aligned", "y" in misaligned)
    if G == 4:  # the bf16 kernels have no slab-major output
        clause("y_slab8 needs N % 8 == 0", bool(g["y_slab8"]) and N % 8 != 0)
    if has["residual"]:
        clause("ldres % 4 == 0", g["ldres"] % G != 0)
        clause("residual aligned", "residual" in misaligned)
    clause("x aligned", "x" in misaligned)
    clause("wt aligned", "wt" in misaligned)
    tile = g["tile"]
    clause("tile in 0..6", tile not in k["tiles"])
    if kernel == "bf16_p8":  # it clamps the weight rows it reads instead
        only("bf16_p8", "w_rows >= 1", g["w_rows"] < 1)
    elif tile in k["tiles"] and N > 0:
        clause("w_rows covers the padded N", pad_to(N, k["tiles"][tile][1]) > g["w_rows"])
    mode = g["mode"]
    clause("mode", mode not in k["modes"])  # the hooks refuse the stem mode, the launchers the modes their kernel lacks
    stride_ok = g["Ho"] >= 1 and g["Wo"] >= 1 and g["stride"] >= 1
    if mode not in k["modes"]:
        pass
    elif mode == DENSE:
        clause("lda >= K", g["lda"] < K)
        clause("lda % 4 == 0", g["lda"] % G != 0)
    elif mode == STRIDED:
        clause("Cin == K", g["Cin"] != K)
        clause("Cin % 4 == 0", g["Cin"] % G != 0)
        clause("Ho, Wo, stride >= 1", not stride_ok)
        clause("(Ho - 1) * stride < Hi", stride_ok and (g["Ho"] - 1) * g["stride"] >= g["Hi"])
        clause("(Wo - 1) * stride < Wi", stride_ok and (g["Wo"] - 1) * g["stride"] >= g["Wi"])
    elif mode == CONV3:
        clause("Cin % 32 == 0", g["Cin"] % SLAB != 0)
        clause("K == 9 * Cin", K != 9 * g["Cin"])
        cs = g["Cin"] // SLAB  # the hooks derive cin_slabs from Cin
        only("bf16_p8", "cin_slabs a power of two", g["Cin"] % SLAB == 0 and cs & (cs - 1) != 0)
        clause("Ho == Hi", g["Ho"] != g["Hi"])
        clause("Wo == Wi", g["Wo"] != g["Wi"])
        clause("Hi, Wi >= 1", g["Hi"] < 1 or g["Wi"] < 1)
    elif mode == DUAL:
        k1 = g["k1_slabs"]
        clause("x2 != NULL", not has["x2"])
        clause("x2 aligned", "x2" in misaligned)
        clause("k1_slabs >= 1", k1 < 1)
        clause("k1_slabs * 32 < K", k1 * SLAB >= K)
        clause("lda >= k1_slabs * 32", g["lda"] < k1 * SLAB)
        clause("lda % 4 == 0", g["lda"] % G != 0)
        clause("Cin == K - k1_slabs * 32", g["Cin"] != K - k1 * SLAB)
        clause("Cin % 4 == 0", g["Cin"] % G != 0)
        clause("Ho, Wo, stride >= 1", not stride_ok)
        clause("M % (Ho * Wo) == 0", stride_ok and M % (g["Ho"] * g["Wo"]) != 0)
        clause("(Ho - 1) * stride < Hi", stride_ok and (g["Ho"] - 1) * g["stride"] >= g["Hi"])
        clause("(Wo - 1) * stride < Wi", stride_ok and (g["Wo"] - 1) * g["stride"] >= g["Wi"])
    return bad


def error_bases(kernel="f32"):
    """one valid launch per mode of the kernel (no residual unless the case needs one): the error cases are these with ONE change.
    fp32: the 64x64 tile.  The others: the kernel's first tile, K and Cin in its slabs, pitches in its vectors, w_rows one tile wide;
    f32s: the three weight pieces w_piece = K apart, ldw = 3 K."""
    if kernel == "f32":
        return {
            "dense": dict(mode=DENSE, tile=2, M=5, N=64, K=64, lda=64, ldw=64, ldy=68, ldres=72, w_rows=64, relu=0, use_res=1),
            "strided": dict(mode=STRIDED, tile=2, M=27, N=64, K=32, Cin=32, Hi=6, Wi=6, Ho=3, Wo=3, stride=2, lda=32, ldw=32, ldy=68, ldres=72, w_rows=64,
                            relu=0, use_res=0),
            "conv3": dict(mode=CONV3, tile=2, M=27, N=64, K=288, Cin=32, Hi=3, Wi=3, Ho=3, Wo=3, stride=1, lda=32, ldw=288, ldy=68, ldres=72, w_rows=64,
                          relu=0, use_res=0),
            "dual": dict(mode=DUAL, tile=2, M=27, N=64, K=64, Cin=32, Hi=6, Wi=6, Ho=3, Wo=3, stride=2, k1_slabs=1, lda=32, ldw=64, ldy=68, ldres=72,
                         w_rows=64, relu=0, use_res=0),
        }
    k = KERNELS[kernel]
    S, tile = k["slab"], min(k["tiles"])
    common = dict(tile=tile, N=64, ldy=72, ldres=80, w_rows=k["tiles"][tile][1], relu=0, use_res=0)
    geo = dict(M=27, Hi=6, Wi=6, Ho=3, Wo=3, stride=2)
    out = {
        "dense": dict(common, mode=DENSE, M=5, K=2 * S, lda=2 * S, use_res=1),
        "strided": dict(common, mode=STRIDED, K=S, Cin=S, lda=S, **geo),
        "conv3": dict(common, mode=CONV3, M=27, K=9 * S, Cin=S, Hi=3, Wi=3, Ho=3, Wo=3, stride=1, lda=S),
        "dual": dict(common, mode=DUAL, K=2 * S, Cin=S, k1_slabs=1, lda=S, **geo),
    }
    for c in out.values():
        c.update(ldw=3 * c["K"], w_piece=c["K"]) if kernel == "f32s" else c.update(ldw=c["K"])
    return out


def error_cases(kernel):
    """(base, the one change, null pointers, misaligned pointers) for a kernel other than fp32: every clause of its contract that a
    debug hook can reach, broken once and alone.  Out of reach, for every kernel: the clauses of the stem mode (both geometries: the
    hooks refuse the mode), cin_slabs == Cin / slab (the hooks derive it) and, as in ERROR_CASES, Cin % vector and Cin % slab (other
    clauses imply them); for the 256x256 kernel also the alignment of the zero page and of the split-K workspace, which the library owns.  A conv3 case handed to f32s
    breaks "mode": the kernel has no such mode."""
    k = KERNELS[kernel]
    G, WG, S = k["gran"], k["wgran"], k["slab"]
    b = error_bases(kernel)
    d, K = b["dense"], b["dense"]["K"]
    out = [("dense", dict(M=0), (), ()), ("dense", dict(N=0), (), ()), ("dense", dict(K=0, lda=0, ldw=0, w_piece=0), (), ()),
           ("dense", dict(K=S // 2), (), ()), ("dense", dict(ldw=d["ldw"] + WG // 2), (), ())]
    if kernel == "f32s":
        out += [("dense", dict(w_piece=K + 4, ldw=3 * K + 16), (), ()), ("dense", dict(w_piece=K - 8), (), ()), ("dense", dict(ldw=3 * K - 8), (), ())]
    else:
        out += [("dense", dict(ldw=K - WG), (), ())]
    out += [("dense", {}, (n,), ()) for n in ("x", "wt", "y")]
    out += [("dense", dict(ldy=d["ldy"] + G // 2), (), ()), ("dense", dict(ldres=d["ldres"] + G // 2), (), ())]
    out += [("dense", {}, (), (n,)) for n in ("y", "residual", "x", "wt")]
    if G == 4:
        out += [("dense", dict(y_slab8=1, N=60), (), ())]
    out += [("dense", dict(tile=t), (), ()) for t in (-1, 8) + tuple(t for t in range(8) if t not in k["tiles"])]
    out += [("dense", dict(w_rows=0), (), ())]  # one tile short: the coverage clause, or w_rows >= 1 of the 256x256 kernel
    if kernel != "bf16_p8":
        out += [("dense", dict(w_rows=d["w_rows"] - 4), (), ()), ("dense", dict(N=d["w_rows"] + 4, ldy=d["w_rows"] + 8, ldres=d["w_rows"] + 8), (), ())]
    out += [("dense", dict(mode=STEM), (), ()), ("dense", dict(lda=K - G), (), ()), ("dense", dict(lda=K + G // 2), (), ())]
    out += [("strided", ch, (), ()) for ch in (dict(Cin=2 * S), dict(Ho=0), dict(Wo=0), dict(stride=0), dict(stride=-2), dict(Hi=4), dict(Wi=4))]
    if CONV3 in k["modes"]:
        out += [("conv3", ch, (), ()) for ch in (dict(K=8 * S), dict(Ho=2), dict(Wo=4), dict(Hi=0, Ho=0), dict(Wi=0, Wo=0))]
        if kernel == "bf16_p8":
            out += [("conv3", dict(Cin=3 * S, K=27 * S, ldw=27 * S), (), ())]
    else:
        out += [("conv3", {}, (), ())]
    out += [("dual", {}, ("x2",), ()), ("dual", {}, (), ("x2",))]
    out += [("dual", ch, (), ()) for ch in (dict(k1_slabs=0, Cin=2 * S), dict(k1_slabs=2, Cin=0, lda=2 * S), dict(lda=S - G), dict(lda=S + G // 2),
                                            dict(Cin=2 * S), dict(Ho=0), dict(Wo=0), dict(stride=0), dict(M=26), dict(Hi=4), dict(Wi=4))]
    return out


# (base, the one change, null pointers, misaligned pointers): each breaks exactly one clause of the contract.  Not reachable alone and
# so not listed: Cin % 4 (strided: Cin == K and K % 32 == 0 imply it; dual: K and k1_slabs * 32 are multiples of 32), Cin % 32 of
# conv3 (K == 9 * Cin and K % 32 == 0 imply it) and cin_slabs (the hook derives it from Cin).
ERROR_CASES = [
    ("dense", dict(M=0), (), ()),
    ("dense", dict(N=0), (), ()),
    ("dense", dict(K=0, lda=0, ldw=0), (), ()),
    ("dense", dict(K=48), (), ()),
    ("dense", dict(ldw=66), (), ()),
    ("dense", dict(ldw=60), (), ()),
    ("dense", {}, ("x",), ()),
    ("dense", {}, ("wt",), ()),
    ("dense", {}, ("y",), ()),
    ("dense", dict(ldy=70), (), ()),
    ("dense", {}, (), ("y",)),
    ("dense", dict(y_slab8=1, N=60), (), ()),
    ("dense", dict(ldres=70), (), ()),
    ("dense", {}, (), ("residual",)),
    ("dense", {}, (), ("x",)),
    ("dense", {}, (), ("wt",)),
    ("dense", dict(w_rows=60), (), ()),
    ("dense", dict(N=68), (), ()),  # 68 columns need two 64-wide tiles = 128 weight rows
    ("dense", dict(tile=7), (), ()),
    ("dense", dict(tile=-1), (), ()),
    ("dense", dict(mode=STEM), (), ()),
    ("dense", dict(lda=60), (), ()),
    ("dense", dict(lda=66), (), ()),
    ("strided", dict(Cin=64), (), ()),
    ("strided", dict(Ho=0), (), ()),
    ("strided", dict(stride=0), (), ()),
    ("strided", dict(stride=-2), (), ()),
    ("strided", dict(Hi=4), (), ()),  # (Ho - 1) * stride = 4 >= Hi
    ("strided", dict(Wi=4), (), ()),
    ("conv3", dict(K=256, ldw=288), (), ()),
    ("conv3", dict(Ho=2), (), ()),
    ("conv3", dict(Wo=4), (), ()),
    ("conv3", dict(Hi=0, Ho=0), (), ()),
    ("dual", {}, ("x2",), ()),
    ("dual", {}, (), ("x2",)),
    ("dual", dict(k1_slabs=0, Cin=64), (), ()),
    ("dual", dict(k1_slabs=2, Cin=0, lda=64), (), ()),  # k1_slabs * 32 == K: nothing left for the strided source
    ("dual", dict(lda=28), (), ()),
    ("dual", dict(lda=34), (), ()),
    ("dual", dict(Cin=64), (), ()),
    ("dual", dict(Wo=0), (), ()),
    ("dual", dict(M=26), (), ()),
    ("dual", dict(Hi=4), (), ()),
    ("dual", dict(Wi=4), (), ()),
]


def error_case(i, kernel="f32"):
    base, change, null, mis = (ERROR_CASES if kernel == "f32" else error_cases(kernel))[i]
    return dict(error_bases(kernel)[base], **change), null, mis


# ------------------------------------------------------------------------------------------- the inputs and references of a case
def bf16_round(a):
    """float32 -> the nearest bf16 value (ties to even), held in float32: torch.bfloat16's rounding, as _bf16_round of test_gpu_parity.py"""
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def reads_bf16(kernel):
    """True for the kernels whose activations, weights, residual and output are bf16"""
    return KERNELS[kernel]["gran"] == 8


def split3(W):
    """The three-step rule of csrc/bf16_split.h's header comment (conv_gemm_f32s.hip): w0 = bf16(w), w1 = bf16(w - w0), w2 = bf16(w - w0 - w1); both
    subtractions are exact in float32.  Three float32 arrays holding bf16 values.  Written from the comment, not from the host packer."""
    w = np.asarray(W, np.float32)
    w0 = bf16_round(w)
    r1 = w - w0
    w1 = bf16_round(r1)
    return w0, w1, bf16_round(r1 - w1)


SPLIT_GAP = 1e3  # between the pieces of a weight row when w_piece > K: never read, and far from any weight if it is


def pack_split3(W, w_rows, ldw, w_piece):
    """W [N,K] -> [w_rows, ldw] of bf16 values: piece j of Wt[n][k] at n * ldw + j * w_piece + k; rows past N zero"""
    N, K = W.shape
    out = np.zeros((w_rows, ldw), np.float32)
    out[:N] = SPLIT_GAP
    for j, piece in enumerate(split3(W)):
        out[:N, j * w_piece : j * w_piece + K] = piece
    return out


def a_matrix(mode, x, x2, Ho, Wo, stride, k1_cols):
    """the A operand [M, K] of a non-dense mode, gathered in the k order of the packing, in the dtype of x"""
    if mode == STRIDED:
        return gather_strided(x, Ho, Wo, stride)
    if mode == CONV3:
        B, H, W, C = x.shape
        xp = np.zeros((B, H + 2, W + 2, C), x.dtype)
        xp[:, 1 : H + 1, 1 : W + 1] = x
        return np.concatenate([xp[:, kh : kh + H, kw : kw + W].reshape(B * H * W, C) for kh in range(3) for kw in range(3)], axis=1)
    return np.concatenate([x[:, :k1_cols], gather_strided(x2, Ho, Wo, stride)], axis=1)


def abs_product(A, W):
    """sum_k |a| |w| in float64: the size every rounding of the accumulation is relative to"""
    return np.abs(np.asarray(A, np.float64)) @ np.abs(np.asarray(W, np.float64)).T


@functools.lru_cache(maxsize=None)
def _dense_master(K, Mmax, Nmax, bf=False):
    """one draw per (K, block): every dense case of the block is its top-left corner, the float64 product is formed once.  bf: the
    activations, weights and residual are rounded to bf16 before anything is formed from them"""
    g = rng(DENSE, K, Mmax, Nmax)
    A, W = normal(g, (Mmax, K)), weights(g, Nmax, K)
    sc, sh = scale_shift(g, Nmax)
    R, pad = normal(g, (Mmax, Nmax)), normal(g, (Mmax, 16 if bf else 8))
    if bf:
        A, W, R, pad = bf16_round(A), bf16_round(W), bf16_round(R), bf16_round(pad)
    return dict(A=A, W=W, R=R, pad=pad, scale=sc, shift=sh, acc=acc_dense(A, W), absacc=abs_product(A, W) if bf else None)


@functools.lru_cache(maxsize=None)
def _conv_master(mode, Hi, Wi, Ho, Wo, stride, Cin, N, k1, S=BK, bf=False):
    g = rng(mode, Hi, Wi, Ho, stride, Cin, N, k1)
    rnd = bf16_round if bf else (lambda a: a)
    M = BATCH * Ho * Wo
    d = dict(x2=None, x=rnd(normal(g, (BATCH, Hi, Wi, Cin))), R=rnd(normal(g, (M, N))), a=None)
    d["scale"], d["shift"] = scale_shift(g, N)
    if mode == STRIDED:
        d["W"] = rnd(weights(g, N, Cin))
        d["acc"] = acc_strided(d["x"], d["W"], Ho, Wo, stride)
    elif mode == CONV3:
        d["hwio"] = rnd(normal(g, (3, 3, Cin, N), 1.0 / np.sqrt(9 * Cin)))
        d["W"] = pack_3x3(d["hwio"], N, 9 * Cin)
        d["acc"] = acc_conv3(d["x"], d["hwio"])
    else:  # DUAL: x is the strided source here, a the dense one
        K = k1 * S + Cin
        d["a"], d["pad"] = rnd(normal(g, (M, k1 * S))), rnd(normal(g, (M, 8)))
        d["W1"], d["W2"] = rnd(weights(g, N, K)[:, : k1 * S].copy()), rnd(weights(g, N, K)[:, :Cin].copy())
        d["W"] = np.concatenate([d["W1"], d["W2"]], axis=1)
        d["acc"] = acc_dual(d["a"], d["W1"], d["x"], d["W2"], Ho, Wo, stride)
    if bf:
        d["absacc"] = abs_product(a_matrix(mode, d["x"] if mode != DUAL else d["a"], d["x"], Ho, Wo, stride, k1 * S), d["W"])
    return d


def inputs(c):
    """host arrays of case c in the layouts the kernel reads -- x [M, lda] (dense; the columns past K hold noise, not zeros) or NHWC,
    x2, wt [w_rows, ldw], res [M + 1, ldres], scale, shift -- and acc, the float64 accumulators A . Wt^T.  All float32; for the bf16
    kernels every activation, weight and residual is a bf16 value (upload as bf16) and absacc holds sum_k |a| |w|.  f32s: wt holds the
    three bf16 pieces of every weight (upload as bf16).  W: the logical weights [N, K] in the packing's k order."""
    M, N, K = c["M"], c["N"], c["K"]
    kernel = c.get("kernel", "f32")
    bf = reads_bf16(kernel)
    if c["mode"] == DENSE:
        m = _dense_master(K, *c.get("master", (DENSE_M_MAX, DENSE_N_MAX)), bf=bf)
        x = np.concatenate([m["A"][:M], m["pad"][:M]], axis=1)[:, : c["lda"]]
        x2, W, R, acc = None, m["W"][:N], m["R"][:M, :N], m["acc"][:M, :N]
    else:
        m = _conv_master(c["mode"], c["Hi"], c["Wi"], c["Ho"], c["Wo"], c["stride"], c["Cin"], N, c.get("k1_slabs", 0), S=slab(kernel), bf=bf)
        x, x2, W, R, acc = m["x"], None, m["W"], m["R"], m["acc"]
        if c["mode"] == DUAL:
            x, x2 = np.concatenate([m["a"], m["pad"]], axis=1)[:, : c["lda"]], m["x"]
    res = None
    if c.get("use_res"):
        res = np.full((M + 1, c["ldres"]), 1e3, np.float32)  # a residual read at the wrong pitch, column or row lands on 1000 (a bf16 value)
        res[:M, :N] = R
    wt = pack_split3(W, c["w_rows"], c["ldw"], c["w_piece"]) if kernel == "f32s" else pack_rows(W, c["w_rows"], c["ldw"])
    out = dict(x=np.ascontiguousarray(x), x2=x2, wt=wt, res=res, scale=m["scale"][:N], shift=m["shift"][:N], acc=acc, W=W)
    if bf:
        out["absacc"] = m["absacc"][:M, :N]
    return out


def reference(c, inp):
    """row-major float64 [M, N]"""
    return epilogue(inp["acc"], inp["scale"], inp["shift"], None if inp["res"] is None else inp["res"][: c["M"], : c["N"]], c["relu"])


def float32_restatement(c, inp):
    """the same computation carried out in float32 NumPy on the operands of the case: what a kernel that accumulates in fp32 can be
    asked to reach.  For the bf16 kernels this is the value BEFORE the one final rounding to bf16 (bf16_round gives the output)."""
    M, N, K = c["M"], c["N"], c["K"]
    A = inp["x"][:, :K] if c["mode"] == DENSE else a_matrix(c["mode"], inp["x"], inp["x2"], c["Ho"], c["Wo"], c["stride"], K - c.get("Cin", 0))
    y = (A.astype(np.float32) @ inp["W"].T.astype(np.float32)) * inp["scale"] + inp["shift"]
    if inp["res"] is not None:
        y = y + inp["res"][:M, :N]
    assert y.dtype == np.float32 and y.shape == (M, N)
    return np.maximum(y, 0) if c["relu"] else y


# ------------------------------------------------------------------------------------------- the bars of the bf16 kernels
# First check: the project's two bf16 layer bars (test_gpu_parity.py), on the whole matrix and on each edge block.  Second check, per
# element: |got - ref| <= 2^-8 |ref| + 4 e32 A[m][n].  2^-8 |ref| is the one final rounding to bf16 (half an ulp of an 8-bit significand
# is at most 2^-8 of the value); A = sum_k |a| |w| * |scale| + |shift| + |res| is what every fp32 rounding before it is relative to;
# e32 is the largest |restatement before the final rounding - ref| / A the float32 NumPy restatement reaches on the same case, and 4 the
# margin test_gpu_encoder_train.py grants a different but equally valid summation order.
BF16_ULP = 2.0 ** -8
BF16_L2 = 2.5e-3
ORDER_MARGIN = 4.0
BLOCK_NAMES = ("whole matrix", "last partial M-tile", "last partial N-tile")


def rel_l2(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.sqrt(((got - ref) ** 2).sum() / ((ref ** 2).sum() + 1e-300)))


def edge_blocks(M, N, BM, BN):
    """the (row slice, column slice) of the three blocks of edge_errors; None for a block that does not exist"""
    return ((slice(0, M), slice(0, N)), (slice(M // BM * BM, M), slice(0, N)) if M % BM else None, (slice(0, M), slice(N // BN * BN, N)) if N % BN else None)


def magnitude(c, inp):
    """A[m][n] of the second check, float64"""
    a = inp["absacc"] * np.abs(np.asarray(inp["scale"], np.float64)) + np.abs(np.asarray(inp["shift"], np.float64))
    return a if inp["res"] is None else a + np.abs(np.asarray(inp["res"][: c["M"], : c["N"]], np.float64))


def bf16_figures(c, inp, got):
    """got [M, N] (bf16 values) against the float64 reference -> (e32, per block (max-normalised error, rel-L2, worst ratio of an
    element's error to its bound, the block's rel-L2 bar) or None where the block does not exist).  Every element of [M, N] enters
    every figure.  The rel-L2 bar is 2.5e-3 except on a block where the float64 reference rounded once to bf16 -- the best any kernel
    can do -- itself misses it: 2.5e-3 is the rms of many roundings, and four of them (the 1 x 4 block of M = BM + 1, N = 4) can all
    fall badly.  Such a block gets the format's own bound 2^-8, which no correctly rounded output exceeds; the per-element check
    binds every one of its elements all the same (tests/test_gemm_ref_cpu.py counts these blocks and pins their size)."""
    ref, A = reference(c, inp), magnitude(c, inp)
    e32 = float((np.abs(float32_restatement(c, inp).astype(np.float64) - ref) / A).max())
    err = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):  # a bound of 0 (everything cut by the ReLU, exactly): only an error of 0 meets it
        ratio = np.where(err == 0, 0.0, err / (BF16_ULP * np.abs(ref) + ORDER_MARGIN * e32 * A))
    ideal = bf16_round(ref.astype(np.float32))  # float32 holds 24 bits of the reference: its rounding to bf16 is the reference's
    out = []
    for b in edge_blocks(c["M"], c["N"], *TILES[c["tile"]]):
        if b is None:
            out.append(None)
            continue
        l2_bar = BF16_L2 if rel_l2(ideal[b], ref[b]) < BF16_L2 else BF16_ULP
        out.append((rel(got[b], ref[b]), rel_l2(got[b], ref[b]), float(ratio[b].max()), l2_bar))
    return e32, out


def bf16_misses(figures):
    """the checks that the per-block figures of bf16_figures miss, as text"""
    bad = []
    for name, f in zip(BLOCK_NAMES, figures):
        if f is None:
            continue
        if not f[0] < BF16_ULP:
            bad.append("%s max-normalised %.3e >= 2^-8" % (name, f[0]))
        if not f[1] < f[3]:
            bad.append("%s rel-L2 %.3e >= %.3e" % (name, f[1], f[3]))
        if not f[2] <= 1.0:
            bad.append("%s an element is at %.2f of 2^-8 |ref| + 4 e32 A" % (name, f[2]))
    return bad
