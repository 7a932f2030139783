"""NumPy CPU reference of the checkpoint scores (DESIGN.md "Checkpoint scores"; the kernel is csrc/eval_scores.hip).

The silhouette contract restated in integers: vertices snapped to 1/256 px, int64 edge functions and the renderer's top-left tie rule at
the sample (x, y) = (column, row).  Fed with the vertices the GPU saw, the covered pixels agree bit for bit.  The keypoint part is float64.
"""
import numpy as np

GUARD = 16384.0
TORSO = (9, 2)   # left shoulder, right hip (LSP order)
HEAD = (13, 12)  # head top, neck


def _edge(ax, ay, bx, by, px, py):
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


def _owns(ax, ay, bx, by):
    return (by > ay) | ((by == ay) & (bx < ax))


def snap(verts2d):
    """[P,2] float -> X, Y int64 (1/256 px) and which vertices are finite and inside the guard band"""
    v = np.asarray(verts2d, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(v).all(1) & (np.abs(v) <= GUARD).all(1)
    s = np.rint(256.0 * np.where(ok[:, None], v, 0.0)).astype(np.int64)  # exact: a power-of-two scale, then round half to even
    return s[:, 0], s[:, 1], ok


def silhouette(verts2d, faces, H, W):
    """-> bool [H,W]: pixel (row i, column j) is covered when the point (j, i) is inside some face"""
    X, Y, ok = snap(verts2d)
    f = np.asarray(faces, np.int64).reshape(-1, 3).copy()
    P = len(X)
    keep = ((f >= 0) & (f < P)).all(1)
    f = f[keep]
    keep = ok[f].all(1)
    f = f[keep]
    A = _edge(X[f[:, 0]], Y[f[:, 0]], X[f[:, 1]], Y[f[:, 1]], X[f[:, 2]], Y[f[:, 2]])
    f, A = f[A != 0], A[A != 0]
    neg = A < 0  # both windings are drawn: swap to a positive orientation
    f[neg, 1], f[neg, 2] = f[neg, 2].copy(), f[neg, 1].copy()
    out = np.zeros(H * W, bool)
    fx, fy = X[f], Y[f]
    # first / last pixel whose sample 256 j lies in the snapped box: ceil(min / 256), floor(max / 256), clipped to the image
    x0, x1 = np.maximum(-((-fx.min(1)) // 256), 0), np.minimum(fx.max(1) // 256, W - 1)
    y0, y1 = np.maximum(-((-fy.min(1)) // 256), 0), np.minimum(fy.max(1) // 256, H - 1)
    idx = np.flatnonzero((x0 <= x1) & (y0 <= y1))
    w = (x1 - x0 + 1)[idx]
    cnt = w * (y1 - y0 + 1)[idx]
    if cnt.sum() == 0:
        return out.reshape(H, W)
    fi = np.repeat(idx, cnt)  # one entry per (face, pixel of its box)
    off = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    wr = np.repeat(w, cnt)
    j, i = x0[fi] + off % wr, y0[fi] + off // wr
    px, py = 256 * j, 256 * i
    inside = np.ones(len(fi), bool)
    for p, q in ((1, 2), (2, 0), (0, 1)):  # the edge opposite vertex 0, 1, 2
        ax, ay, bx, by = fx[fi, p], fy[fi, p], fx[fi, q], fy[fi, q]
        E = _edge(ax, ay, bx, by, px, py)
        inside &= (E > 0) | ((E == 0) & _owns(ax, ay, bx, by))
    out[(i * W + j)[inside]] = True
    return out.reshape(H, W)


def counts(verts2d, faces, seg):
    """one image -> int64 [4] = tp, fp, fn, tn of the silhouette against seg > 0"""
    seg = np.asarray(seg)
    g = seg > 0
    p = silhouette(verts2d, faces, *g.shape)
    return np.array([(p & g).sum(), (p & ~g).sum(), (~p & g).sum(), (~p & ~g).sum()], np.int64)


def batch_counts(verts2d_stages, faces, segs):
    """verts2d_stages: n_stage arrays [B,P,2]; segs [B,H,W] -> int64 [n_stage,B,4]"""
    return np.stack([np.stack([counts(v[b], faces, segs[b]) for b in range(len(segs))]) for v in verts2d_stages])


def keypoints(kp_gt, kp2d_stages, H, W):
    """float64: kp_err [n_stage,B,K] pixels (-1 where not visible), norm [B,2] torso and head length (-1 where an end is not visible)"""
    g = np.asarray(kp_gt, np.float32).astype(np.float64)
    vis = g[:, :, 2] > 0
    scale = np.array([0.5 * W, 0.5 * H])
    err = []
    for p in kp2d_stages:
        d = (np.asarray(p, np.float32).astype(np.float64) - g[:, :, :2]) * scale
        err.append(np.where(vis, np.sqrt((d * d).sum(2)), -1.0))
    norm = np.full((g.shape[0], 2), -1.0)
    for c, (j0, j1) in enumerate((TORSO, HEAD)):
        if j0 < g.shape[1] and j1 < g.shape[1]:
            d = (g[:, j0, :2] - g[:, j1, :2]) * scale
            norm[:, c] = np.where(vis[:, j0] & vis[:, j1], np.sqrt((d * d).sum(1)), -1.0)
    return np.stack(err), norm
