"""The 3-D pose scores in float64 NumPy, built on np.linalg.svd: the reference of hpe_pose3d_scores, hpe_debug_procrustes3 and
metrics.Scores3D (DESIGN.md "3-D pose scores").  This is the usual HMR evaluation (compute_similarity_transform + root alignment), restated.

A point is scored when its weight is > 0.  Means are taken of the points relative to the first scored one, which changes nothing
mathematically and makes "var1 == 0" exact for a cloud of identical points."""
import numpy as np

FLAG_ROOT, FLAG_PA_JOINTS, FLAG_PA_VERTS, FLAG_NO_VERTS = 1, 2, 4, 8
PCK3D_THRESHOLDS_MM = tuple(range(0, 151, 5))


def solve_rotation(K):
    """K [3,3] = sum x1 x2^T -> (R, trace(R K)): R = V Z U^T, Z = diag(1, 1, sign det(U V^T)); NaN for a K that is not finite"""
    K = np.asarray(K, np.float64)
    if not np.isfinite(K).all():
        return np.full((3, 3), np.nan), np.nan
    U, s, Vt = np.linalg.svd(K)
    V = Vt.T
    d = np.sign(np.linalg.det(U @ V.T))
    if d == 0:
        d = 1.0
    Z = np.diag([1.0, 1.0, d])
    R = V @ Z @ U.T
    return R, float(s[0] + s[1] + d * s[2])


def gap_ratio(K):
    """(sigma_2 + sigma_3 sign det(U V^T)) / sigma_1: how well R is determined (0 for K == 0)"""
    U, s, Vt = np.linalg.svd(np.asarray(K, np.float64))
    d = np.sign(np.linalg.det(U @ Vt))
    return 0.0 if s[0] == 0 else float((s[1] + d * s[2]) / s[0])


def similarity(X, Y, w=None):
    """-> (scale, R, t, mu1, mu2) of the fit of X [N,3] to Y [N,3] over the scored points, or None where it is undefined"""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    sel = np.ones(len(X), bool) if w is None else np.asarray(w) > 0
    if sel.sum() < 3:
        return None
    Xs, Ys = X[sel], Y[sel]
    px, py = Xs[0], Ys[0]
    mu1, mu2 = px + (Xs - px).mean(0), py + (Ys - py).mean(0)
    X1, X2 = Xs - mu1, Ys - mu2
    var1 = (X1 ** 2).sum()
    if var1 == 0:
        return None
    K = X1.T @ X2
    R, tr = solve_rotation(K)
    scale = tr / var1
    return scale, R, mu2 - scale * R @ mu1, mu1, mu2


def pa_errors(X, Y, fit):
    """|scale R (x - mu1) - (y - mu2)| per point; NaN where the fit is undefined"""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    if fit is None:
        return np.full(len(X), np.nan)
    scale, R, _t, mu1, mu2 = fit
    return np.linalg.norm(scale * (X - mu1) @ R.T - (Y - mu2), axis=1)


def xform13(fit):
    if fit is None:
        return np.full(13, np.nan)
    return np.concatenate([[fit[0]], fit[1].reshape(-1), fit[2]])


def pose3d_scores(joints, joints_gt, weights=None, verts=None, verts_gt=None, roots=(2, 3)):
    """joints [n,B,K,3], joints_gt [B,K,3], weights [B,K] or None, verts [n,B,P,3] and verts_gt [B,P,3] or None ->
    (joint_err [n,B,2,K], summary [n,B,6], xform [n,B,2,13]) in float64"""
    joints, joints_gt = np.asarray(joints, np.float64), np.asarray(joints_gt, np.float64)
    n, B, K, _ = joints.shape
    a, b = roots
    err, summ, xf = np.full((n, B, 2, K), -1.0), np.zeros((n, B, 6)), np.full((n, B, 2, 13), np.nan)
    for s in range(n):
        for i in range(B):
            X, Y = joints[s, i], joints_gt[i]
            sel = np.ones(K, bool) if weights is None else np.asarray(weights[i]) > 0
            flags = 0
            if sel[a] and sel[b]:
                rx, ry = (X[a] + X[b]) / 2, (Y[a] + Y[b]) / 2
            else:
                rx = ry = np.full(3, np.nan)
                flags |= FLAG_ROOT
            fit = similarity(X, Y, sel)
            if fit is None:
                flags |= FLAG_PA_JOINTS
            e0, e1 = np.linalg.norm((X - rx) - (Y - ry), axis=1), pa_errors(X, Y, fit)
            err[s, i, 0, sel], err[s, i, 1, sel] = e0[sel], e1[sel]
            xf[s, i, 0] = xform13(fit)
            cnt = int(sel.sum())
            summ[s, i, 0] = e0[sel].mean() if cnt else np.nan
            summ[s, i, 1] = e1[sel].mean() if cnt else np.nan
            summ[s, i, 2] = summ[s, i, 3] = np.nan
            if verts is None:
                flags |= FLAG_NO_VERTS
            else:
                V, VG = np.asarray(verts[s][i], np.float64), np.asarray(verts_gt[i], np.float64)
                vfit = similarity(V, VG)
                if vfit is None:
                    flags |= FLAG_PA_VERTS
                summ[s, i, 2] = np.linalg.norm((V - rx) - (VG - ry), axis=1).mean()
                summ[s, i, 3] = pa_errors(V, VG, vfit).mean()
                xf[s, i, 1] = xform13(vfit)
            summ[s, i, 4], summ[s, i, 5] = cnt, flags
    return err, summ, xf


def scores3d(batches, num_joints=14, to_mm=1000.0):
    """the results of metrics.Scores3D from a list of (joint_err, summary) batches, by loops; one dict per stage"""
    n = batches[0][0].shape[0]
    out = []
    for s in range(n):
        images = root_bad = pa_bad = 0
        root_sum, root_cnt = np.zeros(num_joints), np.zeros(num_joints)
        pa_sum, pa_cnt = np.zeros(num_joints), np.zeros(num_joints)
        hits = np.zeros(len(PCK3D_THRESHOLDS_MM))
        pve, pve_n, pa_pve, pa_pve_n = 0.0, 0, 0.0, 0
        for err, summ in batches:
            err, summ = np.asarray(err, np.float64), np.asarray(summ, np.float64)
            for i in range(err.shape[1]):
                flags = int(summ[s, i, 5])
                images += 1
                root_bad += bool(flags & FLAG_ROOT)
                pa_bad += bool(flags & FLAG_PA_JOINTS)
                for j in range(num_joints):
                    if err[s, i, 0, j] < 0 and err[s, i, 1, j] < 0:
                        continue
                    if not flags & FLAG_ROOT:
                        e = err[s, i, 0, j] * to_mm
                        root_sum[j] += e
                        root_cnt[j] += 1
                        for k, thr in enumerate(PCK3D_THRESHOLDS_MM):
                            hits[k] += e <= thr
                    if not flags & FLAG_PA_JOINTS:
                        pa_sum[j] += err[s, i, 1, j] * to_mm
                        pa_cnt[j] += 1
                if not flags & (FLAG_ROOT | FLAG_NO_VERTS):
                    pve, pve_n = pve + summ[s, i, 2] * to_mm, pve_n + 1
                if not flags & (FLAG_PA_VERTS | FLAG_NO_VERTS):
                    pa_pve, pa_pve_n = pa_pve + summ[s, i, 3] * to_mm, pa_pve_n + 1

        def ratio(x, y):
            with np.errstate(invalid="ignore", divide="ignore"):
                return np.where(np.asarray(y) > 0, np.asarray(x) / np.where(np.asarray(y) > 0, y, 1), np.nan)

        share = ratio(hits, root_cnt.sum())
        out.append({"mpjpe_mm": float(ratio(root_sum.sum(), root_cnt.sum())), "pa_mpjpe_mm": float(ratio(pa_sum.sum(), pa_cnt.sum())),
                    "pve_mm": float(ratio(pve, pve_n)), "pa_pve_mm": float(ratio(pa_pve, pa_pve_n)),
                    "mpjpe_per_joint_mm": ratio(root_sum, root_cnt).tolist(), "pa_mpjpe_per_joint_mm": ratio(pa_sum, pa_cnt).tolist(),
                    "pck3d_150": float(share[-1]), "auc3d": float(share.mean()), "images": images, "pa_invalid_images": pa_bad,
                    "root_invalid_images": root_bad})
    return out
