"""NumPy restatement of the chained forms of the streaming 1x1 kernel (csrc/conv_stream_chain_f32s.hip) and the float64 chain they are
measured against.  Written from the kernel's header comment, nothing taken from the library; the split is tests/gemm_ref.py's.

    t3 = relu(scaleA * (WA . a) + shiftA (+ res))      K = 64 (identity chain) or 64 + 64 (conv_block chain, folded weights, no residual)
    u1 = relu(scaleB * (WB . t3) + shiftB)             K = 256, N = 64

Both GEMMs: the operands split into three bf16 pieces (round to nearest even), per 16-k step the six products with i + j <= 2, the five cross
terms smallest first into one fp32 accumulator and a0 w0 into another, the two added at the end.  One MFMA is modelled as its 16 exact
products per output summed in float64 and added to the fp32 accumulator with one rounding.  The reduce is cut into eight k-slices of 32
channels, one per wave, each walked in the register order of a transposed 32x32 accumulator (chain_perm), and the eight partial sums are
added in wave order in fp32.  The epilogues are fp32: one fused multiply-add, then the residual, then the ReLU."""
import numpy as np

from gemm_ref import split3

WAVES, SLICE = 8, 32
PRODUCTS = ((2, 0), (1, 1), (0, 2), (1, 0), (0, 1))  # (activation piece, weight piece) of the cross terms, smallest first


def chain_k(s, hi, t):
    """channel (of a wave's 32) behind slot t of k-step s of the reduce on lane half hi"""
    return 16 * s + 8 * (t >> 2) + 4 * hi + (t & 3)


def chain_perm():
    """k order of a wave's slice of the reduce: the matrix core's k index 16 s + 8 hi + t reads channel chain_k(s, hi, t)"""
    return np.array([chain_k(s, hi, t) for s in range(2) for hi in range(2) for t in range(8)])


def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32)


def split_gemm(A, W, order=None):
    """A [M,K] . W [N,K]^T in fp32 by the six-product rule, k walked in `order` (default 0 .. K-1), 16 at a time"""
    A, W = np.array(A, np.float32), np.array(W, np.float32)  # (copies: the shared inputs are read-only)
    K = A.shape[1]
    order = np.arange(K) if order is None else np.asarray(order)
    assert K % 16 == 0 and sorted(order.tolist()) == list(range(K))
    a = [p.astype(np.float64) for p in split3(A)]
    w = [p.astype(np.float64) for p in split3(W)]
    acc = np.zeros((A.shape[0], W.shape[0]), np.float32)
    acx = np.zeros_like(acc)
    for q in range(K // 16):
        ks = order[16 * q:16 * q + 16]
        for i, j in PRODUCTS:
            acx = _f32(acx.astype(np.float64) + a[i][:, ks] @ w[j][:, ks].T)
        acc = _f32(acc.astype(np.float64) + a[0][:, ks] @ w[0][:, ks].T)
    return _f32(acc.astype(np.float64) + acx)


def _fma(acc, scale, shift):
    return _f32(acc.astype(np.float64) * np.asarray(scale, np.float32).astype(np.float64) + np.asarray(shift, np.float32).astype(np.float64))


def chain_model(a, WA, scaleA, shiftA, res, WB, scaleB, shiftB):
    """the kernel's arithmetic: a [M, K] (t2, or [t2 | x] in the conv_block form), res [M, 256] or None -> (t3 [M,256], u1 [M,64]), fp32"""
    t3 = _fma(split_gemm(a, WA), scaleA, shiftA)
    if res is not None:
        t3 = _f32(t3.astype(np.float64) + np.asarray(res, np.float32))
    t3 = np.maximum(t3, np.float32(0))
    perm = chain_perm()
    u = None
    for wv in range(WAVES):  # wave order
        sl = SLICE * wv + perm
        part = split_gemm(t3[:, sl], np.asarray(WB, np.float32)[:, sl])
        u = part if u is None else _f32(u.astype(np.float64) + part)
    return t3, np.maximum(_fma(u, scaleB, shiftB), np.float32(0))


def chain_fp64(a, WA, scaleA, shiftA, res, WB, scaleB, shiftB):
    """the same chain in float64 on the same fp32 operands (scale / shift as the fp32 values the kernels read)"""
    f = lambda v: np.asarray(v, np.float32).astype(np.float64)
    t3 = (f(a) @ f(WA).T) * f(scaleA) + f(shiftA)
    if res is not None:
        t3 = t3 + f(res)
    t3 = np.maximum(t3, 0)
    return t3, np.maximum((t3 @ f(WB).T) * f(scaleB) + f(shiftB), 0)


def to_slab8(u1):
    """u1 [M, 64] -> channel-slab major [8, M, 8]: element (n, m) at [(n // 8), m, n % 8]"""
    M, N = u1.shape
    return np.ascontiguousarray(u1.reshape(M, N // 8, 8).transpose(1, 0, 2))
