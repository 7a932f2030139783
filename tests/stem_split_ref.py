"""NumPy model of the fp32 fused stem on the bf16 matrix cores (csrc/stem_fused.hip, stem_fused_f32s_kernel): the exact 3-piece bf16
split, the packing of the split weights, and the kernel's arithmetic in its own order -- per conv row, kernel rows 0..6, each one
32-deep MFMA step (8 px x 4 ch); the five cross terms a2 w0, a0 w2, a1 w1, a1 w0, a0 w1 into one fp32 accumulator and a0 w0 into a
second one, the two added once, then BN (one fused multiply-add), ReLU and the 3x3 / 2 max-pool.

What the model assumes of an MFMA: the products of two bf16 values are exact, the 32 of a step are summed exactly and the accumulator
takes one fp32 rounding per instruction.  The sums run in float64 here (24 + 5 bits: exact for these magnitudes up to the last bits)."""
import numpy as np

from hpe_amd import resnet_spec, synthetic

S = resnet_spec.CONV_SPECS[0]
# (activation piece, weight piece) in the kernel's order; the last one goes to the leading accumulator
CROSS = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1))
BAR = 5e-6  # the project's per-kernel bar against fp64: max|d| / max|ref|


def bf16_round(x):
    """round-to-nearest-even fp32 -> bf16 (finite inputs), returned as uint16 bit patterns: f2bf of csrc/bf16_split.h"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_value(h):
    return (h.astype(np.uint32) << 16).view(np.float32)


def split3(x):
    """x -> uint16 [3, ...]: x = h0 + h1 + h2 exactly, each piece the bf16 nearest to what the pieces before it left (bf16_split3)"""
    x = np.ascontiguousarray(x, np.float32)
    h0 = bf16_round(x)
    r1 = x - bf16_value(h0)
    h1 = bf16_round(r1)
    r2 = r1 - bf16_value(h1)
    return np.stack([h0, h1, bf16_round(r2)])


def pack_weights(kernel):
    """HWIO [7,7,3,64] fp32 -> (Wt [64][7][32] fp32 in the k enumeration kh, then 8 px x 4 ch; its split uint16 [3][64][7][32])"""
    wt = np.zeros((64, 7, 8, 4), np.float32)
    wt[:, :, :7, :3] = np.transpose(kernel, (3, 0, 1, 2))
    wt = wt.reshape(64, 7, 32)
    return wt, split3(wt)


def bn_fold(p, eps=1e-3):
    """scale / shift as the library folds them: in double, rounded once to fp32 (bn_fold of csrc/hpe_ctx.h)"""
    g, b = p[S.bn_name + "/gamma"].astype(np.float64), p[S.bn_name + "/beta"].astype(np.float64)
    m, v = p[S.bn_name + "/moving_mean"].astype(np.float64), p[S.bn_name + "/moving_variance"].astype(np.float64)
    scale = g / np.sqrt(v + np.float64(np.float32(eps)))
    shift = (p[S.name + "/bias"].astype(np.float64) - m) * scale + b
    return scale.astype(np.float32), shift.astype(np.float32)


def dynamic_range_images(B=3, seed=411):
    """the seeded synthetic images times 2^e, e per pixel from [-12, 12]; a third of the pixels exactly zero; image 0 carries constant
    +1 rows at the top, image 1 constant -1 columns at the left (the padding rows and columns matter)"""
    img = synthetic.make_images(B, seed=seed)
    g = np.random.Generator(np.random.Philox(seed + 1))
    e = g.integers(-12, 13, size=img.shape[:3])
    img = img * np.exp2(e).astype(np.float32)[..., None]
    img[g.random(img.shape[:3]) < 1.0 / 3] = 0.0
    img[0, :5, :, :] = 1.0
    img[1, :, :4, :] = -1.0
    return np.ascontiguousarray(img, np.float32)


def max_pool(act):
    """pool1_pad + MaxPooling2D(3, strides 2) of a non-negative [B,112,112,C] map"""
    B, H, W, C = act.shape
    p = np.zeros((B, H + 2, W + 2, C), act.dtype)
    p[:, 1:-1, 1:-1] = act
    out = None
    for dy in range(3):
        for dx in range(3):
            v = p[:, dy:dy + H:2, dx:dx + W:2]
            out = v if out is None else np.maximum(out, v)
    return out


def windows(x):
    """[B,224,224,3] -> [B,112,112,7,32]: the 8 px x 4 ch of every kernel row of every conv pixel (zero pad channel, eighth pixel
    real data or conv1_pad's zeros -- its weights are zero)"""
    B = x.shape[0]
    p = np.zeros((B, 230, 232, 4), x.dtype)
    p[:, 3:227, 3:227, :3] = x
    out = np.empty((B, 112, 112, 7, 8, 4), x.dtype)
    for kh in range(7):
        for kw in range(8):
            out[:, :, :, kh, kw] = p[:, kh:kh + 223:2, kw:kw + 223:2]
    return out.reshape(B, 112, 112, 7, 32)


def reference_fp64(img, p):
    """the layer in float64 from the unsplit fp32 values"""
    wt = pack_weights(p[S.name + "/kernel"])[0].astype(np.float64)
    lin = np.einsum("bhwrk,nrk->bhwn", windows(img.astype(np.float64)), wt, optimize=True) + p[S.name + "/bias"].astype(np.float64)
    g, b = p[S.bn_name + "/gamma"].astype(np.float64), p[S.bn_name + "/beta"].astype(np.float64)
    m, v = p[S.bn_name + "/moving_mean"].astype(np.float64), p[S.bn_name + "/moving_variance"].astype(np.float64)
    sc = g / np.sqrt(v + 1e-3)
    return max_pool(np.maximum(lin * sc + (b - m * sc), 0))


def model_fp32(img, p):
    """the kernel's arithmetic: [B,56,56,64] fp32"""
    a = [windows(bf16_value(h)).astype(np.float64) for h in split3(img)]
    w = [bf16_value(h).astype(np.float64) for h in pack_weights(p[S.name + "/kernel"])[1]]
    B = img.shape[0]
    acc = np.zeros((B, 112, 112, 64), np.float32)
    acx = np.zeros((B, 112, 112, 64), np.float32)
    for kh in range(7):
        for i, j in CROSS:
            acx = (acx + a[i][:, :, :, kh] @ w[j][:, kh].T).astype(np.float32)
        acc = (acc + a[0][:, :, :, kh] @ w[0][:, kh].T).astype(np.float32)
    conv = acc + acx
    scale, shift = bn_fold(p)
    act = np.maximum((conv.astype(np.float64) * scale + shift).astype(np.float32), np.float32(0))
    return max_pool(act)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))
