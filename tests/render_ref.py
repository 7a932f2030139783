"""NumPy CPU reference of the mesh renderer (DESIGN.md "Renderer"; the kernels are csrc/render.hip).

Vertex stage in float64; coverage and visibility with the same int64 edge functions and top-left tie rule as the GPU, so that fed with
the GPU's own snapped vertex records the covered pixels agree bit for bit.  Vectorised over (face, pixel) candidates from each face's
bounding box: one 224 x 224 SMPL-sized image takes well under a second.
"""
import math

import numpy as np

BLUE = np.array([0.65098039, 0.74117647, 0.85882353])
PINK = np.array([0.9, 0.7, 0.7])
LIGHT_COLOR = np.array([1.0, 1.0, 0.7])
GUARD = 16384.0


def _rot_y(points, angle):
    ry = np.array([[np.cos(angle), 0.0, np.sin(angle)], [0.0, 1.0, 0.0], [-np.sin(angle), 0.0, np.cos(angle)]])
    return np.dot(points, ry)


LIGHTS = _rot_y(np.array([[-200.0, -100.0, -100.0], [800.0, 10.0, 300.0], [-500.0, 500.0, 1000.0]]), np.radians(120))


def rodrigues(axis, deg):
    """cv2.Rodrigues of radians(deg) about axis 1 = x, 2 = y, 3 = z"""
    t = math.radians(deg)
    c, s = math.cos(t), math.sin(t)
    return {1: np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), 2: np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]),
            3: np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])}[axis]


def vertex_records(verts, faces, H, W, cam=None, rot_axis=0, rot_deg=0.0, near=None, far=None, color_id=0):
    """-> dict U, V (int64, 1/256 px), valid (bool), iz, rgb [P,3], u, v (float64 pixel coordinates), verts (the posed vertices)"""
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64)
    if rot_axis:
        c = v.mean(0)
        v = np.dot(v - c, rodrigues(rot_axis, rot_deg)) + c
    fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    n = np.zeros_like(v)
    for k in range(3):
        np.add.at(n, f[:, k], fn)
    nl = np.linalg.norm(n, axis=1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        n = np.where(nl > 0, n / np.where(nl > 0, nl, 1), 0.0)
        shade = np.zeros(len(v))
        for k in range(3):
            d = LIGHTS[k] - v
            shade += LIGHT_COLOR[k] * np.maximum((n * d).sum(1) / np.linalg.norm(d, axis=1), 0.0)
    rgb = (PINK if (int(color_id or 0) % 2) else BLUE)[None, :] * shade[:, None]
    fl, px, py = (500.0, W / 2.0, H / 2.0) if cam is None else [float(x) for x in cam]
    znear = 0.1 if near is None or near < 0 else near
    zfar = np.inf if far is None or far < 0 else far
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        u = fl * v[:, 0] / v[:, 2] + px
        vv = fl * v[:, 1] / v[:, 2] + py
        valid = np.isfinite(v).all(1) & (v[:, 2] >= znear) & (v[:, 2] <= zfar) & (np.abs(u) <= GUARD) & (np.abs(vv) <= GUARD)
        U = np.where(valid, np.rint(256.0 * np.where(valid, u, 0)), 0).astype(np.int64)
        V = np.where(valid, np.rint(256.0 * np.where(valid, vv, 0)), 0).astype(np.int64)
        iz = np.where(valid, 1.0 / v[:, 2], 0.0)
    return {"U": U, "V": V, "valid": valid, "iz": iz, "rgb": rgb, "u": u, "v": vv, "verts": v}


def normal_condition(verts, faces):
    """per vertex: sum_k |n_k| / |sum_k n_k| over its faces' cross products -- how much float32 rounding of the sum is amplified in the
    normalised normal (inf for a vertex of no face or a cancelling sum)"""
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64)
    fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    n = np.zeros_like(v)
    mag = np.zeros(len(v))
    for k in range(3):
        np.add.at(n, f[:, k], fn)
        np.add.at(mag, f[:, k], np.linalg.norm(fn, axis=1))
    with np.errstate(invalid="ignore", divide="ignore"):
        return mag / np.linalg.norm(n, axis=1)


def records_from_gpu(rec):
    """[P,8] int32 view of hpe_debug_render_vertices -> the dict vertex_records returns (U, V, valid, iz, rgb)"""
    rec = np.asarray(rec)
    fl = rec.view(np.float32)
    return {"U": rec[:, 0].astype(np.int64), "V": rec[:, 1].astype(np.int64), "valid": rec[:, 2] != 0, "iz": fl[:, 4].astype(np.float64),
            "rgb": fl[:, 5:8].astype(np.float64)}


def _edge(ax, ay, bx, by, px, py):
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


def _owns(ax, ay, bx, by):
    return (by > ay) | ((by == ay) & (bx < ax))


def _oriented(rec, faces):
    """faces with positive snapped area (v1 / v2 swapped where negative), their area, and which faces survive rejection"""
    f = np.asarray(faces, np.int64).copy()
    U, V = rec["U"], rec["V"]
    A = _edge(U[f[:, 0]], V[f[:, 0]], U[f[:, 1]], V[f[:, 1]], U[f[:, 2]], V[f[:, 2]])
    neg = A < 0
    f[neg, 1], f[neg, 2] = f[neg, 2].copy(), f[neg, 1].copy()
    ok = rec["valid"][f].all(1) & (A != 0)
    return f, np.abs(A), ok


def _terms(rec, f, A, px, py):
    """edge functions E [n,3] of oriented faces f [n,3] at the samples of pixels (px, py), and the inside mask"""
    U, V = rec["U"], rec["V"]
    x, y = U[f], V[f]
    sx, sy = 256 * px + 128, 256 * py + 128
    E = np.stack([_edge(x[:, 1], y[:, 1], x[:, 2], y[:, 2], sx, sy), _edge(x[:, 2], y[:, 2], x[:, 0], y[:, 0], sx, sy),
                  _edge(x[:, 0], y[:, 0], x[:, 1], y[:, 1], sx, sy)], 1)
    own = np.stack([_owns(x[:, 1], y[:, 1], x[:, 2], y[:, 2]), _owns(x[:, 2], y[:, 2], x[:, 0], y[:, 0]),
                    _owns(x[:, 0], y[:, 0], x[:, 1], y[:, 1])], 1)
    inside = ((E > 0) | ((E == 0) & own)).all(1)
    return E, inside


def candidates(rec, faces, H, W):
    """every covered (face, pixel) pair: (face index, pixel index py * W + px, float64 depth z_pix)"""
    f, A, ok = _oriented(rec, faces)
    U, V = rec["U"], rec["V"]
    x0 = np.maximum(-((128 - U[f].min(1)) // 256), 0)
    x1 = np.minimum((U[f].max(1) - 128) // 256, W - 1)
    y0 = np.maximum(-((128 - V[f].min(1)) // 256), 0)
    y1 = np.minimum((V[f].max(1) - 128) // 256, H - 1)
    ok &= (x0 <= x1) & (y0 <= y1)
    idx = np.flatnonzero(ok)
    w = (x1 - x0 + 1)[idx]
    cnt = w * (y1 - y0 + 1)[idx]
    if cnt.sum() == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0)
    fi = np.repeat(idx, cnt)
    off = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    wr = np.repeat(w, cnt)
    px = x0[fi] + off % wr
    py = y0[fi] + off // wr
    E, inside = _terms(rec, f[fi], A[fi], px, py)
    fi, px, py, E = fi[inside], px[inside], py[inside], E[inside]
    lam = E / A[fi][:, None].astype(np.float64)
    z = 1.0 / (lam * rec["iz"][f[fi]]).sum(1)
    return fi, py * W + px, z


def coverage_count(rec, faces, H, W):
    """[H,W] number of faces covering each pixel sample (no depth test)"""
    fi, pix, _ = candidates(rec, faces, H, W)
    return np.bincount(pix, minlength=H * W).reshape(H, W)


def raster_ids(rec, faces, H, W):
    """-> face [H,W] (-1 uncovered), z [H,W] float64 (0 uncovered): nearest depth wins, ties to the lower face index"""
    fi, pix, z = candidates(rec, faces, H, W)
    face = np.full(H * W, -1, np.int64)
    zz = np.zeros(H * W)
    if len(fi):
        order = np.lexsort((fi, z, pix))
        pix_s = pix[order]
        first = np.ones(len(order), bool)
        first[1:] = pix_s[1:] != pix_s[:-1]
        sel = order[first]
        face[pix[sel]] = fi[sel]
        zz[pix[sel]] = z[sel]
    return face.reshape(H, W), zz.reshape(H, W)


def depth_of(rec, faces, face_idx, py, px):
    """float64 depth of the given faces at the given pixels (NaN where the face does not cover the sample)"""
    f, A, ok = _oriented(rec, faces)
    face_idx = np.asarray(face_idx, np.int64)
    E, inside = _terms(rec, f[face_idx], A[face_idx], np.asarray(px, np.int64), np.asarray(py, np.int64))
    lam = E / A[face_idx][:, None].astype(np.float64)
    z = 1.0 / (lam * rec["iz"][f[face_idx]]).sum(1)
    return np.where(inside & ok[face_idx], z, np.nan)


def shade(rec, faces, face, bg=None, do_alpha=False):
    """resolve + composite of one image: face [H,W] -> uint8 [H,W,3|4]"""
    H, W = face.shape
    out = np.empty((H, W, 4 if do_alpha else 3), np.uint8)
    cov = face >= 0
    out[..., :3] = 255 if bg is None else bg
    if do_alpha:
        out[..., 3] = 255 if bg is not None else np.where(cov, 255, 0)
    py, px = np.nonzero(cov)
    if len(py):
        f, A, _ = _oriented(rec, faces)
        fi = face[py, px]
        E, _ = _terms(rec, f[fi], A[fi], px, py)
        lam = E / A[fi][:, None].astype(np.float64)
        wk = lam * rec["iz"][f[fi]]
        z = 1.0 / wk.sum(1)
        c = z[:, None] * (wk[:, :, None] * rec["rgb"][f[fi]]).sum(1)
        out[py, px, :3] = np.floor(255.0 * np.clip(c, 0.0, 1.0) + 0.5).astype(np.uint8)
    return out


def render(verts, faces, H, W, cam=None, bg=None, do_alpha=False, color_id=0, rot_axis=0, rot_deg=0.0, near=None, far=None, rec=None):
    """one image end to end (rec: use these vertex records, e.g. the GPU's, instead of computing them)"""
    if rec is None:
        rec = vertex_records(verts, faces, H, W, cam, rot_axis, rot_deg, near, far, color_id)
    face, _ = raster_ids(rec, faces, H, W)
    return shade(rec, faces, face, bg, do_alpha)
