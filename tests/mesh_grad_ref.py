"""Reference statements behind the mesh-loss gradient tests (test helper, CPU only).

Per image, A = the silhouette pixels (x, y) in tf.where order (constants), B = the P projected vertices:

    L = [ sum_v |B_v - A_nnA(v)|_2  +  sum_a |A_a - B_nnB(a)|_1 ] / (3 + P)

The neighbours are argmins and carry no gradient, so

    (3 + P) dL/dB_v = (B_v - A_nnA(v)) / |B_v - A_nnA(v)|_2  -  sum_{a : nnB(a) = v} sign(A_a - B_v)

with the first term 0 for a vertex exactly on its pixel and sign(0) = 0.  ``closed_form_grad`` states that in float64 numpy GIVEN the
neighbour arrays (in the layout hpe_mesh_loss_grad returns them); ``bidirectional_dist_torch`` restates the reference's
bidirectional_dist (src/ops.py:60-102) in torch with gathers on argmin indices, for autograd."""
import numpy as np
import torch


def exact_neighbours(seg, v):
    """seg [H,W] (> 0 = silhouette), v [P,2] -> (nn_pix [H,W] int32, nn_vert [P] int32) by the exact float64 search, ties to the
    lowest index; -1 off the silhouette / everywhere in nn_vert for an empty silhouette."""
    H, W = seg.shape
    ys, xs = np.where(seg > 0)
    nn_pix = np.full((H, W), -1, np.int32)
    nn_vert = np.full(len(v), -1, np.int32)
    if len(ys) == 0:
        return nn_pix, nn_vert
    A = np.stack([xs, ys], 1).astype(np.float64)
    Bv = np.asarray(v, np.float64)
    best = np.full(len(Bv), np.inf)
    arg = np.zeros(len(Bv), np.int64)
    for i0 in range(0, len(A), 2048):
        D = ((A[i0:i0 + 2048, None, :] - Bv[None, :, :]) ** 2).sum(-1)
        nn_pix[ys[i0:i0 + 2048], xs[i0:i0 + 2048]] = D.argmin(1)
        m = D.min(0)
        upd = m < best
        arg[upd] = i0 + D.argmin(0)[upd]
        best[upd] = m[upd]
    nn_vert[:] = ys[arg] * W + xs[arg]
    return nn_pix, nn_vert


def _pairs(seg, v, nn_pix, nn_vert):
    """-> (A [n,2] silhouette pixels, their vertices B[nn] [n,2], their vertex indices [n], has [P], the vertices' pixels [P,2])"""
    H, W = seg.shape
    Bv = np.asarray(v, np.float64)
    ys, xs = np.where(seg > 0)
    A = np.stack([xs, ys], 1).astype(np.float64).reshape(-1, 2)
    idx = np.asarray(nn_pix)[ys, xs].astype(np.int64)
    nv = np.asarray(nn_vert).astype(np.int64)
    has = nv >= 0
    An = np.stack([nv % W, nv // W], 1).astype(np.float64)
    return A, Bv[idx], idx, has, An


def loss_from_neighbours(seg, v, nn_pix, nn_vert):
    """the image's loss term in float64, evaluated at the given neighbours"""
    A, Bn, _, has, An = _pairs(seg, v, nn_pix, nn_vert)
    Bv = np.asarray(v, np.float64)
    l2 = np.sqrt(((Bv - An) ** 2).sum(1))[has].sum()
    l1 = np.abs(A - Bn).sum()
    return (l1 + l2) / (3 + len(Bv))


def closed_form_grad(seg, v, nn_pix, nn_vert):
    """d(the image's loss term) / d v in float64, [P,2], for the given neighbours"""
    A, Bn, idx, has, An = _pairs(seg, v, nn_pix, nn_vert)
    Bv = np.asarray(v, np.float64)
    d = Bv - An
    n = np.sqrt((d ** 2).sum(1))
    ok = has & (n > 0)
    g = np.zeros_like(Bv)
    g[ok] = d[ok] / n[ok, None]
    sg = np.sign(A - Bn)
    np.subtract.at(g, idx, sg)
    return g / (3 + len(Bv))


def _argmins(A, Bv, chunk=2048):
    """find_nearest_neighbors (src/ops.py:60-71): argmin of D = -2 A B^T + |A|^2 + |B|^2 over each axis, lowest index on ties.  The
    indices carry no gradient, so D is formed without one, ``chunk`` rows at a time."""
    with torch.no_grad():
        bb = (Bv * Bv).sum(1)[None, :]
        ind_ab = []
        best = torch.full((Bv.shape[0],), float("inf"), dtype=Bv.dtype)
        ind_ba = torch.zeros(Bv.shape[0], dtype=torch.int64)
        for i0 in range(0, A.shape[0], chunk):
            a = A[i0:i0 + chunk]
            D = -2.0 * a @ Bv.T + (a * a).sum(1)[:, None] + bb
            ind_ab.append(torch.argmin(D, 1))
            m, am = torch.min(D, 0)
            upd = m < best
            ind_ba = torch.where(upd, am + i0, ind_ba)
            best = torch.where(upd, m, best)
        return torch.cat(ind_ab), ind_ba


def bidirectional_dist_torch(A, Bv, safe_norm=False):
    """src/ops.py:83-102 in torch: gathers on the argmin indices, L2 from B to its neighbour in A + L1 from A to its neighbour in B.
    Also returns the two index vectors.  safe_norm=True replaces sqrt at distance 0 by a constant 0 (the library's convention for a
    vertex exactly on its pixel; torch's gradient, like tf.norm's, is NaN there)."""
    ind_ab, ind_ba = _argmins(A, Bv)
    d = Bv - A[ind_ba]
    sq = (d * d).sum(1)
    if safe_norm:
        on = sq == 0
        dist_ba = torch.where(on, torch.zeros_like(sq), torch.sqrt(torch.where(on, torch.ones_like(sq), sq)))
    else:
        dist_ba = torch.sqrt(sq)
    dist_ab = (A - Bv[ind_ab]).abs().sum(1)
    return dist_ba.sum() + dist_ab.sum(), ind_ab, ind_ba


def silhouette_points_torch(seg, dtype=torch.float64):
    """[n,2] (x, y) in tf.where order"""
    ys, xs = np.where(np.asarray(seg) > 0)
    return torch.from_numpy(np.stack([xs, ys], 1).astype(np.float64).reshape(-1, 2)).to(dtype)


def mesh_loss_torch(segs, verts2d, safe_norm=False):
    """sum over the images of bidirectional_dist / (3 + P) (src/ops.py:117-137); segs: numpy [B,H,W], verts2d: torch [B,P,2].
    An image with an empty silhouette contributes nothing."""
    total = verts2d.new_zeros(())
    for b in range(verts2d.shape[0]):
        A = silhouette_points_torch(segs[b], verts2d.dtype)
        if A.shape[0] == 0:
            continue
        total = total + bidirectional_dist_torch(A, verts2d[b], safe_norm)[0] / (3 + verts2d.shape[1])
    return total


def neighbours_from_indices(seg, ind_ab, ind_ba):
    """argmin index vectors of bidirectional_dist_torch -> (nn_pix [H,W], nn_vert [P]) in the library's layout"""
    H, W = seg.shape
    ys, xs = np.where(seg > 0)
    nn_pix = np.full((H, W), -1, np.int32)
    nn_pix[ys, xs] = np.asarray(ind_ab)
    ib = np.asarray(ind_ba)
    return nn_pix, (ys[ib] * W + xs[ib]).astype(np.int32)
