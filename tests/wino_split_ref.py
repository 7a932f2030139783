"""NumPy restatement of the arithmetic of wino_fused_split_kernel (csrc/conv_wino.hip): the fused F(2x2,3x3) layer on the bf16
matrix cores through the exact three-piece split.

What is restated, in the kernel's own order:
  * U = G g G^T from double, rounded once to fp32 (the host packer);
  * the input transform B^T d B in fp32: rows first (d0 - d2, d1 + d2, d2 - d1, d1 - d3), then the same on the columns;
  * the split x0 = bf16(x), x1 = bf16(x - x0), x2 = bf16(x - x0 - x1), every piece rounded to nearest even, of V and of U;
  * per slab of 8 channels three 16-deep matrix steps into ONE fp32 accumulator, smallest terms first, each step carrying two
    (A piece, W piece) pairs over the same 8 channels:   {a0 w2, a2 w0}   {a1 w0, a1 w1}   {a0 w0, a0 w1};
    a step is modelled as one rounding: acc = fp32(acc + exact sum of its 16 products);
  * the output transform A^T M A in fp32, left to right.
fp32_mfma_layer is the same layer on the fp32 matrix instruction (2 k per step, one rounding per step), the arithmetic of
wino_fused_kernel; direct_fp64 is the reference.
"""
import numpy as np

SLAB = 8
# (A piece, W piece) of lanes 0-31 and of lanes 32-63, in the order of the three steps
STEPS = (((0, 2), (2, 0)), ((1, 0), (1, 1)), ((0, 0), (0, 1)))

G = np.array([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], np.float64)


def bf16_rne(x):
    """fp32 -> nearest bf16 (ties to even), returned as fp32 (finite inputs)"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    u = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return u.view(np.float32)


def split3(x):
    x = np.asarray(x, np.float32)
    h0 = bf16_rne(x)
    r1 = (x - h0).astype(np.float32)
    h1 = bf16_rne(r1)
    r2 = (r1 - h1).astype(np.float32)
    return h0, h1, bf16_rne(r2)


def winograd_u(w):
    """w [3][3][C][N] -> U [16][N][C] fp32, computed in double"""
    u = np.einsum("ai,ijcn,bj->abnc", G, w.astype(np.float64), G)
    return u.reshape(16, w.shape[3], w.shape[2]).astype(np.float32)


def input_transform(x):
    """x [H][W][C] fp32 (H, W even) -> V [16][tiles][C] fp32, the kernel's fp32 operation order"""
    H, W, C = x.shape
    xp = np.zeros((H + 2, W + 2, C), np.float32)
    xp[1:-1, 1:-1] = x
    d = [[xp[a:a + H:2, e:e + W:2] for e in range(4)] for a in range(4)]  # d[a][e]: [TH][TW][C]
    rows = lambda a, e: (d[0][e] - d[2][e], d[1][e] + d[2][e], d[2][e] - d[1][e], d[1][e] - d[3][e])[a]  # noqa: E731
    V = []
    for a in range(4):
        r = [rows(a, e) for e in range(4)]
        V += [r[0] - r[2], r[1] + r[2], r[2] - r[1], r[1] - r[3]]
    return np.stack(V).reshape(16, -1, C).astype(np.float32)


def output_transform(M, H, W):
    """M [16][tiles][N] fp32 -> y [H][W][N] fp32"""
    u0 = [M[v] + M[4 + v] + M[8 + v] for v in range(4)]
    u1 = [M[4 + v] - M[8 + v] - M[12 + v] for v in range(4)]
    o = [[u0[0] + u0[1] + u0[2], u0[1] - u0[2] - u0[3]], [u1[0] + u1[1] + u1[2], u1[1] - u1[2] - u1[3]]]
    N = M.shape[2]
    y = np.empty((H, W, N), np.float32)
    for dy in range(2):
        for dx in range(2):
            y[dy::2, dx::2] = o[dy][dx].reshape(H // 2, W // 2, N)
    return y


def _step(acc, terms):
    """one matrix step: a single rounding of the accumulator plus the exact sum of the step's products"""
    s = acc.astype(np.float64)
    for a, w in terms:
        s = s + np.einsum("ctk,cnk->ctn", a.astype(np.float64), w.astype(np.float64))
    return s.astype(np.float32)


def split_gemm(V, U, accumulators=1):
    """M [16][tiles][N]: the kernel's split products.  accumulators=2 keeps a0 w0 apart from the five cross terms (the 1x1
    kernel's arrangement), for comparison only."""
    C = V.shape[2]
    acc = np.zeros((16, V.shape[1], U.shape[1]), np.float32)
    accx = np.zeros_like(acc)
    for k in range(0, C, SLAB):
        a = split3(V[:, :, k:k + SLAB])
        w = split3(U[:, :, k:k + SLAB])
        if accumulators == 1:
            for lo, hi in STEPS:
                acc = _step(acc, [(a[lo[0]], w[lo[1]]), (a[hi[0]], w[hi[1]])])
        else:
            accx = _step(accx, [(a[0], w[2]), (a[2], w[0])])
            accx = _step(accx, [(a[1], w[0]), (a[1], w[1])])
            accx = _step(accx, [(a[0], w[1])])
            acc = _step(acc, [(a[0], w[0])])
    return acc if accumulators == 1 else acc + accx


def fp32_gemm(V, U):
    """the fp32 matrix instruction: 2 k per step"""
    acc = np.zeros((16, V.shape[1], U.shape[1]), np.float32)
    for k in range(0, V.shape[2], 2):
        acc = _step(acc, [(V[:, :, k:k + 2], U[:, :, k:k + 2])])
    return acc


def split_layer(x, w, accumulators=1):
    H, W, _ = x.shape
    return output_transform(split_gemm(input_transform(x), winograd_u(w), accumulators), H, W)


def fp32_mfma_layer(x, w):
    H, W, _ = x.shape
    return output_transform(fp32_gemm(input_transform(x), winograd_u(w)), H, W)


def direct_fp64(x, w):
    """3x3 / stride 1 / SAME, x [H][W][C], w [3][3][C][N]"""
    H, W, C = x.shape
    xp = np.zeros((H + 2, W + 2, C), np.float64)
    xp[1:-1, 1:-1] = x
    y = np.zeros((H, W, w.shape[3]), np.float64)
    for i in range(3):
        for j in range(3):
            y += xp[i:i + H, j:j + W] @ w[i, j].astype(np.float64)
    return y


def dynamic_range_input(g, H, C, binades=12):
    """N(0,1) scaled by 2^+-binades per pixel, a third exact zeros"""
    x = g.normal(0, 1, (H, H, C)) * np.exp2(g.integers(-binades, binades + 1, (H, H, 1)))
    x[g.random(x.shape) < 1 / 3] = 0.0
    return x.astype(np.float32)


def max_rel(a, ref):
    return float(np.abs(np.asarray(a, np.float64) - ref).max() / np.abs(ref).max())
