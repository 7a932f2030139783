"""NumPy restatement of the skeleton drawing and the panel (DESIGN.md "Training summaries"): the raster rules in exact integers and the
reference's paint order (src/util/renderer.py:411-438), painted FORWARDS over the image -- the last paint wins --, where csrc/draw.hip
gathers backwards.  It shares no code with csrc/draw.hip or hpe_amd/draw.py; the tables below are typed from the reference's first
(19-joint) tables on their own."""
import numpy as np

WHITE = (255, 255, 255)
PINK, LPINK, LGREEN, GREEN, RED, PURPLE, LBLUE, BLUE = ((197, 27, 125), (233, 163, 201), (161, 215, 106), (77, 146, 33), (215, 48, 39),
                                                        (118, 42, 131), (145, 191, 219), (69, 117, 180))
JCOLORS = [LPINK] * 3 + [PINK] * 3 + [LBLUE] * 3 + [BLUE] * 3 + [PURPLE, PURPLE, RED, GREEN, GREEN, WHITE, WHITE]
PARENTS = [1, 2, 8, 9, 3, 4, 7, 8, 12, 12, 9, 10, 14, -1, 13, -1, -1, 15, 16]
ECOLORS = {0: LPINK, 1: LPINK, 2: LPINK, 3: PINK, 4: PINK, 5: PINK, 6: LBLUE, 7: LBLUE, 8: LBLUE, 9: BLUE, 10: BLUE, 11: BLUE, 12: PURPLE,
           14: PURPLE, 17: LGREEN, 18: LGREEN}


def grid(H, W):
    y, x = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    return x, y


def disc_mask(H, W, cx, cy, r):
    x, y = grid(H, W)
    return (x - cx) ** 2 + (y - cy) ** 2 <= r * r


def ring_mask(H, W, cx, cy, r):
    x, y = grid(H, W)
    d4 = 4 * ((x - cx) ** 2 + (y - cy) ** 2)
    return ((2 * r - 1) ** 2 <= d4) & (d4 < (2 * r + 1) ** 2)


def edge_mask(H, W, x0, y0, x1, y1, th):
    """4 * dist2 <= th * th with dist2 the squared distance to the segment p0-p1.  The middle branch, 4 * (|a|^2 * (b.b) - (a.b)^2) <=
    th * th * (b.b), is evaluated in Python integers (joints reach +-32768, where |a|^2 * (b.b) leaves 64 bits), and only for the pixels
    of the segment's bounding box grown by th: no other pixel is within th / 2 of it."""
    x, y = grid(H, W)
    ax, ay, bx, by = x - x0, y - y0, int(x1) - int(x0), int(y1) - int(y0)
    ab, bb, a2 = ax * bx + ay * by, bx * bx + by * by, ax * ax + ay * ay
    first = ab <= 0  # bb == 0 lands here: ab is 0
    last = ~first & (ab >= bb)
    hit = (first & (4 * a2 <= th * th)) | (last & (4 * ((x - x1) ** 2 + (y - y1) ** 2) <= th * th))
    near = ~first & ~last & (x >= min(x0, x1) - th) & (x <= max(x0, x1) + th) & (y >= min(y0, y1) - th) & (y <= max(y0, y1) + th)
    for yy, xx in np.argwhere(near).tolist():
        A, D = int(a2[yy, xx]), int(ab[yy, xx])
        if 4 * (A * int(bb) - D * D) <= th * th * int(bb):
            hit[yy, xx] = True
    return hit


def joint_pixels(v):
    """float pixel coordinates -> integers: np.round (half to even), clamped to +-32768, a NaN to -32768"""
    v = np.asarray(v, np.float32)
    r = np.where(np.isnan(v), np.float32(-32768), np.clip(np.round(v), -32768, 32768))
    return r.astype(np.int64)


def draw_skeleton(image, joints, draw_edges=True, vis=None, radius=None):
    """uint8 [H,W,3], joints float [19,2] in pixels -> a new uint8 [H,W,3]"""
    img = image.copy()
    H, W = img.shape[:2]
    r = max(4, int(np.mean([H, W]) * 0.01)) if radius is None else int(radius)
    j = joint_pixels(joints)

    def fill(mask, color):
        img[mask] = color

    for child in range(19):
        cx, cy = int(j[child, 0]), int(j[child, 1])
        if vis is not None and not vis[child]:
            continue
        if not draw_edges:
            fill(ring_mask(H, W, cx, cy, r - 1), JCOLORS[child])
            continue
        fill(disc_mask(H, W, cx, cy, r), WHITE)
        fill(disc_mask(H, W, cx, cy, r - 1), JCOLORS[child])
        pa = PARENTS[child]
        if pa < 0 or (vis is not None and not vis[pa]):
            continue
        px, py = int(j[pa, 0]), int(j[pa, 1])
        fill(disc_mask(H, W, px, py, r - 1), JCOLORS[pa])
        fill(edge_mask(H, W, cx, cy, px, py, max(1, r - 2)), ECOLORS[child])
    return img


def crop_u8(images):
    """fp32 in [-1, 1] -> trunc(((img + 1) * 0.5) * 255) in float32, in that order, clamped to [0, 255]; a NaN reads 0"""
    f = ((np.asarray(images, np.float32) + np.float32(1)) * np.float32(0.5)) * np.float32(255)
    f = np.where(np.isnan(f), np.float32(0), np.clip(f, 0, 255))
    return np.trunc(f).astype(np.uint8)


def panels(images, kp_gt, kp_pred, rend_img, rend_seg):
    """images fp32 [n,S,S,3], kp_gt [n,19,3], kp_pred [n,T,19,2], rend_* uint8 [n*T,S,S,3] -> uint8 [n, T*S, 3*S, 3]"""
    n, S = images.shape[0], images.shape[1]
    T = kp_pred.shape[1]
    crops = crop_u8(images)
    to_px = lambda k: ((np.asarray(k, np.float32) + np.float32(1)) * np.float32(0.5)) * np.float32(S)  # noqa: E731
    out = np.zeros((n, T * S, 3 * S, 3), np.uint8)
    for i in range(n):
        with_gt = draw_skeleton(crops[i], to_px(kp_gt[i, :, :2]), draw_edges=False, vis=kp_gt[i, :, 2].astype(bool))
        for t in range(T):
            skel = draw_skeleton(with_gt, to_px(kp_pred[i, t]))
            out[i, t * S:(t + 1) * S] = np.hstack([skel, rend_img[i * T + t], rend_seg[i * T + t]])
    return out


def joint_cases(S=224, seed=0):
    """(kp_gt [2,19,3], kp_pred [2,2,19,2]) in normalised coordinates covering: joints at pixel (0,0) and (S-1,S-1); joints outside the
    panel on each side; coincident child and parent; an invisible child and an invisible parent (ground truth); an exact .5 pixel
    coordinate (round half to even, both parities: at S = 224 the pixel coordinates 7k + 3.5 are dyadic in normalised form, so float32
    carries them exactly); NaN"""
    rng = np.random.RandomState(seed)
    px = lambda p: np.float32(2.0 * p / S - 1.0)  # noqa: E731  the normalised coordinate of pixel coordinate p
    gt = np.zeros((2, 19, 3), np.float32)
    gt[:, :, :2] = rng.uniform(-0.9, 0.9, (2, 19, 2))
    gt[:, :, 2] = 1
    pred = rng.uniform(-0.9, 0.9, (2, 2, 19, 2)).astype(np.float32)
    # image 0, stage 0
    pred[0, 0, 0] = (px(0), px(0))
    pred[0, 0, 5] = (px(S - 1), px(S - 1))
    pred[0, 0, 6] = (px(-7), px(40))          # left of the panel
    pred[0, 0, 11] = (px(S + 9), px(60))      # right
    pred[0, 0, 13] = (px(100), px(-30))       # above
    pred[0, 0, 3] = (px(50), px(S + 2))       # below: within the radius, its disc clips
    pred[0, 0, 2] = pred[0, 0, 1]             # coincident child (1) and parent (2)
    # image 0, stage 1: half-pixel coordinates, both parities, and NaN
    pred[0, 1, 7] = (px(10.5), px(17.5))      # -> 10, 18
    pred[0, 1, 8] = (px(24.5), px(101.5))     # -> 24, 102
    pred[0, 1, 15] = (np.nan, px(30))
    pred[0, 1, 10] = (px(80), np.nan)
    pred[0, 1, 12] = (np.float32(1e9), np.float32(-1e9))  # far outside: clamped
    # ground truth: invisible child, invisible parent, NaN visibility (visible), joints at the corners and outside
    gt[0, 4, 2] = 0
    gt[0, 8, 2] = 0
    gt[0, 9, 2] = np.nan
    gt[0, 0, :2] = (px(0), px(0))
    gt[0, 1, :2] = (px(S - 1), px(S - 1))
    gt[0, 2, :2] = (px(-2), px(50))
    gt[1, 3, :2] = (px(31.5), px(38.5))       # -> 32, 38
    gt[1, 5, :2] = (np.nan, np.nan)
    gt[1, 6, 2] = 0
    return gt, pred
