"""CPU checks behind the mesh-loss gradient: the closed form the GPU tests compare against equals float64 autograd of the torch
restatement of the reference's bidirectional_dist, and the C ABI carries hpe_mesh_loss_grad."""
import ctypes as C

import numpy as np
import torch

from hpe_amd import _lib, build as hbuild

import mesh_grad_ref as R


def _case(seed=5, B=4, H=64, W=72, P=300):
    """random vertices against elliptical silhouettes; image 1: some vertices exactly on silhouette pixels; image 2: ragged
    silhouette and an integer lattice of vertices (exact ties); image 3: empty silhouette"""
    g = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    seg = np.zeros((B, H, W), np.float32)
    for b in range(B):
        seg[b] = ((xx - W * (0.4 + 0.05 * b)) ** 2 / (0.3 * W) ** 2 + (yy - H * 0.5) ** 2 / (0.35 * H) ** 2 <= 1.0)
    seg[2] *= (np.arange(W)[None, :] % 2 == 0)
    seg[3] = 0.0
    v = np.stack([g.uniform(-0.1 * W, 1.1 * W, (B, P)), g.uniform(-0.1 * H, 1.1 * H, (B, P))], -1)
    ys, xs = np.where(seg[1] > 0)
    pick = g.choice(len(ys), 40, replace=False)
    v[1, :40, 0], v[1, :40, 1] = xs[pick], ys[pick]
    v[2] = np.round(v[2])
    return seg, v.astype(np.float32).astype(np.float64)


def test_closed_form_equals_autograd():
    seg, v = _case()
    B, P = v.shape[0], v.shape[1]
    x = torch.from_numpy(v).requires_grad_(True)
    loss = R.mesh_loss_torch(seg, x, safe_norm=True)
    (auto,) = torch.autograd.grad(loss, x)
    auto = auto.numpy()
    assert np.isfinite(auto).all()
    total = 0.0
    for b in range(B):
        A = R.silhouette_points_torch(seg[b])
        if A.shape[0] == 0:
            nn_pix, nn_vert = np.full(seg[b].shape, -1, np.int32), np.full(P, -1, np.int32)
        else:
            _, ind_ab, ind_ba = R.bidirectional_dist_torch(A, torch.from_numpy(v[b]))
            nn_pix, nn_vert = R.neighbours_from_indices(seg[b], ind_ab.numpy(), ind_ba.numpy())
        want = R.closed_form_grad(seg[b], v[b], nn_pix, nn_vert)
        total += R.loss_from_neighbours(seg[b], v[b], nn_pix, nn_vert)
        n = np.linalg.norm(want)
        if n == 0.0:
            assert b == 3 and float(np.abs(auto[b]).max()) == 0.0  # the empty silhouette: an all-zero gradient
            continue
        rel = np.linalg.norm(auto[b] - want) / n
        assert rel <= 1e-12, (b, rel)
    assert abs(total - float(loss.detach())) <= 1e-12 * abs(total)
    # image 1: the 40 vertices on their pixels get no first term -- what is left is the integer count / (3 + P)
    got = auto[1, :40] * (3 + P)
    assert np.abs(got - np.round(got)).max() <= 1e-9 and np.abs(got).max() >= 1.0
    # without the convention torch (as tf.norm) gives NaN exactly there, and the same values elsewhere
    x2 = torch.from_numpy(v).requires_grad_(True)
    (plain,) = torch.autograd.grad(R.mesh_loss_torch(seg, x2), x2)
    plain = plain.numpy()
    assert np.isnan(plain[1, :40]).any()
    assert np.linalg.norm(plain[0] - auto[0]) <= 1e-12 * np.linalg.norm(auto[0])


def test_exact_neighbours_reproduce_the_argmins():
    """the exact search of the helper and the argmins of the expanded form agree on a case without near-ties at float64"""
    seg, v = _case(seed=6, P=200)
    A = R.silhouette_points_torch(seg[0])
    _, ind_ab, ind_ba = R.bidirectional_dist_torch(A, torch.from_numpy(v[0]))
    nn_pix, nn_vert = R.neighbours_from_indices(seg[0], ind_ab.numpy(), ind_ba.numpy())
    e_pix, e_vert = R.exact_neighbours(seg[0], v[0])
    assert np.array_equal(nn_pix, e_pix) and np.array_equal(nn_vert, e_vert)


def test_mesh_loss_grad_symbol_and_argument_checks():
    """hpe_mesh_loss_grad is exported with the declared signature; a null ctx answers HPE_ERR_INVALID, and where a ctx can be created
    (a GPU is visible) a null gradient pointer is refused before any launch."""
    hbuild.build()
    lib = _lib.load()
    assert "hpe_mesh_loss_grad" in _lib.declared_symbols()
    assert lib.hpe_mesh_loss_grad.argtypes == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p]
    assert lib.hpe_mesh_loss_grad.restype == C.c_int
    dummy = C.c_void_p(16)  # never dereferenced: the argument checks come first
    assert lib.hpe_mesh_loss_grad(None, dummy, dummy, 1, 8, 8, 5, dummy, dummy, None, None, None) == 1  # HPE_ERR_INVALID: null ctx
    assert b"null ctx" in lib.hpe_last_error()
    cfg = _lib.HpeConfig()
    lib.hpe_config_init(C.byref(cfg))
    h = C.c_void_p()
    rc = lib.hpe_create(C.byref(cfg), C.byref(h))
    assert rc in (0, 4), rc  # 4 = HPE_ERR_NO_DEVICE (no GPU visible)
    if rc == 0:
        try:
            assert lib.hpe_mesh_loss_grad(h, dummy, dummy, 1, 8, 8, 5, dummy, None, None, None, None) == 1
            assert b"grad_verts2d_dev" in lib.hpe_last_error()
            assert lib.hpe_mesh_loss_grad(h, dummy, dummy, 1, 8, 0, 5, dummy, dummy, None, None, None) == 1
        finally:
            lib.hpe_destroy(h)
