"""NumPy float32 restatement of the reference's training-batch augmentation, DataLoader.image_preprocessing
(src/data_loader.py:160-213) with jitter_center, jitter_scale, pad_image_edge, random_flip and flip_image
(src/util/data_utils.py:144-238), the random draws as inputs.

``augment_sample`` follows the reference step by step and MATERIALISES each stage: the resized image, the copy padded by
112 + trans_max + 50, the slice, the reversed copy, then the keypoint lines.  ``fused_sample`` is the rule the kernel implements: no
intermediate, output pixel (oy, ox) reads resized pixel (clamp(cy - 112 + oy), clamp(cx - 112 + ox)), keypoints as
x' = (kx - cx) + 112.  Every operation is float32 in the reference's order; casts to int truncate toward zero as tf.cast does.  The
source coordinate of the resize, (o + 0.5) * scale - 0.5, is one fused multiply-add (one rounding), the form torch's kernels evaluate:
with the product rounded first the result is up to 1.4e-5 away from torch.nn.functional.interpolate at these sizes, with it 1.8e-7.

tf.image.resize is restated from its published rule (TF2 defaults: bilinear, half-pixel centres, no antialiasing); TensorFlow is not
installed here, so tests/test_augment_cpu.py pins the rule against torch.nn.functional.interpolate instead."""
import numpy as np

F = np.float32
S = 224
SWAP_INDS = np.array([5, 4, 3, 2, 1, 0, 11, 10, 9, 8, 7, 6, 12, 13, 14, 16, 15, 18, 17])


def axis_taps(o, src, dst):
    """destination coordinates o (int array) of an axis resized src -> dst: (lower tap, upper tap, weight of the upper tap)"""
    scale = F(src) / F(dst)
    # ONE rounding: the float32 product is exact in float64, and so is the difference for every scale above 2^-7
    x = ((o.astype(np.float64) + 0.5) * np.float64(scale) - 0.5).astype(F)
    fl = np.floor(x)
    lo = np.maximum(fl, 0).astype(np.int64)
    hi = np.minimum(np.ceil(x), src - 1).astype(np.int64)
    return lo, hi, (x - fl).astype(F)


def _lerp(a, b, w):
    return a + (b - a) * w


def gather_bilinear(img, ylo, yhi, wy, xlo, xhi, wx):
    """img float32 [H,W,C]; row taps [n], column taps [m] -> [n,m,C]: the x lerp of the top and bottom rows first, then the y lerp"""
    wx = wx[None, :, None]
    top = _lerp(img[ylo][:, xlo], img[ylo][:, xhi], wx)
    bot = _lerp(img[yhi][:, xlo], img[yhi][:, xhi], wx)
    return _lerp(top, bot, wy[:, None, None])


def resize_bilinear(img, newH, newW):
    """tf.image.resize(img, [newH, newW]) for a float32 [H,W,C] image"""
    assert img.dtype == F and img.ndim == 3
    H, W = img.shape[:2]
    return gather_bilinear(img, *axis_taps(np.arange(newH), H, newH), *axis_taps(np.arange(newW), W, newW))


def geometry(H, W, center, trans, scale, trans_max=20):
    """the integers and factors of jitter_center + jitter_scale, and whether tf.slice would succeed"""
    cx0, cy0 = int(center[0]) + int(trans[0]), int(center[1]) + int(trans[1])
    scale = F(scale)
    newH, newW = int(F(H) * scale), int(F(W) * scale)
    fy, fx = F(newH) / F(H), F(newW) / F(W)
    cx, cy = int(F(cx0) * fx), int(F(cy0) * fy)
    ms = S // 2 + trans_max + 50
    sx, sy = cx + ms - S // 2, cy + ms - S // 2
    inside = sx >= 0 and sy >= 0 and sx + S <= newW + 2 * ms and sy + S <= newH + 2 * ms
    return {"newH": newH, "newW": newW, "fx": fx, "fy": fy, "cx": cx, "cy": cy, "margin_safe": ms, "start": (sx, sy), "inside": inside,
            "rx": F(W) / F(newW), "ry": F(H) / F(newH)}


def _unit(image, seg):
    assert image.dtype == np.uint8 and seg.dtype == np.uint8 and image.shape[:2] == seg.shape and image.shape[2] == 3
    k = F(1.0 / 255.0)
    return image.astype(F) * k, seg.astype(F)[:, :, None] * k


def _final_label(x, y, vis):
    v = (vis > 0).astype(F)
    return (v * np.stack([F(2.0) * (x / F(S)) - F(1.0), F(2.0) * (y / F(S)) - F(1.0), v])).T.astype(F)


def flip_keypoints(x, y, vis):
    """flip_image's keypoint lines: new_x = 224 - x - 1, then the left / right swap of all three rows"""
    x = F(S) - x - F(1.0)
    return x[SWAP_INDS], y[SWAP_INDS], vis[SWAP_INDS]


def augment_sample(image, seg, kp, center, trans, scale, flip, trans_max=20):
    """the reference, stage by stage -> (image [224,224,3], seg [224,224], kp_gt [19,3]); raises ValueError where tf.slice would"""
    H, W = seg.shape
    g = geometry(H, W, center, trans, scale, trans_max)
    img, sg = _unit(image, seg)
    kp = np.asarray(kp, F)
    ms = g["margin_safe"]
    new_image = resize_bilinear(img, g["newH"], g["newW"])  # jitter_scale
    new_seg = resize_bilinear(sg, g["newH"], g["newW"])
    x, y = kp[:, 0] * g["fx"], kp[:, 1] * g["fy"]
    image_pad = np.pad(new_image, ((ms, ms), (ms, ms), (0, 0)), mode="edge")  # pad_image_edge
    seg_pad = np.pad(new_seg, ((ms, ms), (ms, ms), (0, 0)), mode="edge")
    x_pad, y_pad = x + F(ms), y + F(ms)
    sx, sy = g["start"]
    if not g["inside"]:
        raise ValueError("tf.slice: the window leaves the padded image")
    crop = image_pad[sy:sy + S, sx:sx + S]
    crop_gt = seg_pad[sy:sy + S, sx:sx + S]
    x_crop, y_crop, vis = x_pad - F(sx), y_pad - F(sy), kp[:, 2]
    if flip:  # flip_image
        crop, crop_gt = crop[:, ::-1], crop_gt[:, ::-1]
        x_crop, y_crop, vis = flip_keypoints(x_crop, y_crop, vis)
    return (F(2.0) * (crop - F(0.5))).astype(F), np.ascontiguousarray(crop_gt[:, :, 0]), _final_label(x_crop, y_crop, vis)


def fused_sample(image, seg, kp, center, trans, scale, flip, trans_max=20):
    """the kernel's rule: clamped reads of the resized image that never exists; the window may leave the pad (it clamps on)"""
    H, W = seg.shape
    g = geometry(H, W, center, trans, scale, trans_max)
    img, sg = _unit(image, seg)
    kp = np.asarray(kp, F)
    o = np.arange(S)
    ry = np.clip(g["cy"] - S // 2 + o, 0, g["newH"] - 1)
    rx = np.clip(g["cx"] - S // 2 + (S - 1 - o if flip else o), 0, g["newW"] - 1)
    ty, tx = axis_taps(ry, H, g["newH"]), axis_taps(rx, W, g["newW"])
    crop = gather_bilinear(img, *ty, *tx)
    crop_gt = gather_bilinear(sg, *ty, *tx)
    x = (kp[:, 0] * g["fx"] - F(g["cx"])) + F(S // 2)
    y = (kp[:, 1] * g["fy"] - F(g["cy"])) + F(S // 2)
    vis = kp[:, 2]
    if flip:
        x, y, vis = flip_keypoints(x, y, vis)
    return (F(2.0) * (crop - F(0.5))).astype(F), np.ascontiguousarray(crop_gt[:, :, 0]), _final_label(x, y, vis)


def augment_batch(frames, segs, kp, centers, draws, trans_max=20, fn=augment_sample):
    """a batch through ``fn`` -> (images [B,224,224,3], seg [B,224,224], kp_gt [B,19,3])"""
    outs = [fn(frames[b], segs[b], kp[b], centers[b], np.asarray(draws["trans"])[b], np.asarray(draws["scale"])[b],
               bool(np.asarray(draws["flip"])[b]), trans_max) for b in range(len(frames))]
    return tuple(np.stack([o[i] for o in outs]) for i in range(3))


# ---- the fixture shared by the CPU and the GPU tests: five ragged random-noise frames, mixed flips, jitters at -20 and +19
SIZES = [(37, 53), (301, 211), (224, 224), (150, 333), (97, 101)]
CENTERS = np.array([[26, 18], [100, 160], [112, 112], [0, 0], [50, 48]], np.int32)
DRAWS = {"trans": np.array([[-20, 19], [19, -20], [0, 0], [-20, -20], [19, 19]], np.int32),
         "scale": np.array([0.9, 1.17, 1.0, 0.8, 1.2299999], np.float32), "flip": np.array([True, False, True, False, True])}
_CACHE = {}


def fixture():
    """(frames, segs, kp, centers, draws) of the B = 5 case.  37 x 53 is smaller than the crop, so all four edges clamp; 224 x 224 has
    scale exactly 1.0 (the resize is the identity); 150 x 333 has its centre at a corner, so the jittered centre is negative; 97 x 101
    has odd row pitches and an odd byte count.  The masks are noise with half of the pixels 0, so ``> 0`` has edges everywhere;
    keypoints lie in and a little outside the frame, a third of them invisible (visibility 0 or negative)."""
    if "fx" not in _CACHE:
        g = np.random.RandomState(20240)
        frames = [g.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in SIZES]
        segs = [(g.randint(1, 256, (h, w)) * (g.rand(h, w) < 0.5)).astype(np.uint8) for h, w in SIZES]
        kp = np.zeros((len(SIZES), 19, 3), np.float32)
        for b, (h, w) in enumerate(SIZES):
            kp[b, :, 0] = g.uniform(-0.1 * w, 1.1 * w, 19)
            kp[b, :, 1] = g.uniform(-0.1 * h, 1.1 * h, 19)
            kp[b, :, 2] = g.choice([1.0, 1.0, 1.0, 2.0, 0.0, -1.0], 19)
        _CACHE["fx"] = (frames, segs, kp, CENTERS, DRAWS)
    return _CACHE["fx"]


def reference():
    """augment_sample on the fixture, computed once and never modified"""
    if "ref" not in _CACHE:
        out = augment_batch(*fixture())
        for a in out:
            a.setflags(write=False)
        _CACHE["ref"] = out
    return _CACHE["ref"]
