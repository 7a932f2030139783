"""GPU tests of the mesh-loss gradient (run with -m gpu on an MI355X): hpe_mesh_loss_grad under the three pixel -> vertex search
options, the autograd wiring, fit_reprojection and graph capture.

Gradient parity is not checked against neighbours recomputed on the CPU: near-ties (squared distances agreeing to ~1e-3 px^2 out of
1e4) legitimately resolve differently between an fp32 expanded form and an exact search.  Instead the neighbours the call returns
are validated first -- structurally, as the forward's (the float64 loss over them equals hpe_mesh_loss to 1e-5) and as nearest (that
loss equals the exact float64 search's to 1.5e-4) -- and the gradient is then compared with the float64 closed form over those
neighbours with nothing left out: per image ||g - g64|| / ||g64|| <= 1e-4 (the project's fp32 parity bar), exact zeros where the
closed form is exactly zero, everything finite."""
import numpy as np
import pytest
import torch

import hpe_amd
from hpe_amd import synthetic

import mesh_grad_ref as R
from smpl_torch_ref import SmplTorch, make_theta

pytestmark = pytest.mark.gpu
TOL = 1e-4
MODES = ("grid", "valu", "mfma")  # mesh_a2b = 0, 1, 2


@pytest.fixture(scope="module")
def model():
    return synthetic.make_smpl_model()


@pytest.fixture(scope="module")
def engine(model):
    e = hpe_amd.HpeEngine(device=0, max_batch=8)
    e.load_smpl(model)
    e.finalize()
    yield e
    e.close()


@pytest.fixture(scope="module")
def loss_engines():
    """one loss-only context (never finalized) per pixel -> vertex search option"""
    es = {m: hpe_amd.HpeEngine(device=0, max_batch=6, mesh_a2b=m) for m in MODES}
    yield es
    for e in es.values():
        e.close()


def gpu(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


# ------------------------------------------------------------------------------------------------ the input families
def case_lsp(engine):
    """make_lsp_targets silhouettes (one ragged, one empty) against SMPL vertices"""
    B = 3
    seg, _ = synthetic.make_lsp_targets(B, seed=14)
    seg = seg[..., 0].copy()
    seg[1] *= (np.arange(224)[None, :] % 3 == 0)
    seg[2] = 0.0
    th = synthetic.make_thetas(B, seed=15)
    th[:, 0] = 0.8
    v = engine.smpl(gpu(th), want=("verts2d",))["verts2d"].cpu().numpy()
    return seg, v


def case_degenerate():
    """collapsed mesh, off-image mesh against a one-pixel silhouette, integer lattice with exact ties and duplicated vertices"""
    B = 4
    g = np.random.Generator(np.random.Philox(77))
    seg = np.zeros((B, 224, 224), np.float32)
    seg[0, 60:160, 80:150] = 1.0
    seg[1, 10, 200] = 1.0
    seg[2, ::7, ::5] = 1.0
    seg[3, 100:120, 100:120] = 1.0
    v = np.zeros((B, 6890, 2), np.float32)
    v[0] = 112.0 + g.normal(0, 0.5, (6890, 2))
    v[1] = g.uniform(-300, 600, (6890, 2))
    v[2] = np.round(g.uniform(0, 224, (6890, 2)))
    v[2, 1000:2000] = v[2, :1000]
    v[3] = g.uniform(90, 130, (6890, 2))
    return seg, v


def case_edges():
    """around the grid / full-search switch, two thirds off the image, integer and half-pixel lattices, mesh beside the silhouette,
    one-pixel silhouette"""
    g = np.random.Generator(np.random.Philox(4242))
    B = 6
    seg, _ = synthetic.make_lsp_targets(B, seed=31)
    seg = seg[..., 0].copy()
    seg[1] *= (np.arange(224)[None, :] % 3 == 0)
    seg[5] = 0.0
    seg[5, 3, 220] = 1.0
    v = np.zeros((B, 6890, 2), np.float32)
    for b in range(B):
        ys, xs = np.where(seg[b] > 0)
        pick = g.integers(0, len(ys), 6890)
        v[b, :, 0] = xs[pick] + g.uniform(-1, 1, 6890)
        v[b, :, 1] = ys[pick] + g.uniform(-1, 1, 6890)
    v[0] = 112.0 + g.normal(0, 6.0, (6890, 2))
    v[1] = g.uniform(-150, 400, (6890, 2))
    v[2] = np.round(g.uniform(40, 190, (6890, 2)))
    v[2, 3000:4000] = v[2, :1000]
    v[3, :, 0] = g.uniform(0, 60, 6890)
    v[3, :, 1] = g.uniform(0, 224, 6890)
    v[4] = np.round(g.uniform(100, 124, (6890, 2)) * 2) / 2
    return seg, v


GEOMETRIES = [(75, 100, 333), (224, 224, 100), (61, 130, 6890), (8, 8, 5), (224, 224, 12000), (40, 600, 2000)]


def case_geometry(H, W, P):
    """(40, 600, 2000) is wider than the bitmap path takes (point-list vertex -> pixel search); (224, 224, 12000) has more vertices than
    the cell grid's LDS image holds"""
    g = np.random.Generator(np.random.Philox(1000 + H + P))
    B = 3
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    seg = np.zeros((B, H, W), np.float32)
    for b in range(B):
        seg[b] = ((xx - W * (0.4 + 0.1 * b)) ** 2 / (0.3 * W) ** 2 + (yy - H * 0.5) ** 2 / (0.4 * H) ** 2 <= 1.0)
    seg[2] *= (np.arange(W)[None, :] % 2 == 0)
    v = np.stack([g.uniform(-0.1 * W, 1.1 * W, (B, P)), g.uniform(-0.1 * H, 1.1 * H, (B, P))], -1).astype(np.float32)
    return seg, v


_EXACT = {}


def exact_loss(name, seg, v):
    """per-image loss terms over the exact float64 neighbours (does not depend on the search option: computed once per case)"""
    if name not in _EXACT:
        out = []
        for b in range(seg.shape[0]):
            nn_pix, nn_vert = R.exact_neighbours(seg[b], v[b])
            out.append(R.loss_from_neighbours(seg[b], v[b], nn_pix, nn_vert))
        _EXACT[name] = out
    return _EXACT[name]


def check_case(eng, name, seg, v):
    """checks 1-3 and 5 of one case in one context; returns the report line"""
    B, H, W = seg.shape
    P = v.shape[1]
    sg, vg = gpu(seg), gpu(v)
    loss, grad, nn_pix, nn_vert = eng.mesh_loss_grad(sg, vg, want_neighbours=True)
    fwd = eng.mesh_loss(sg, vg)
    loss2, grad2, nn_pix2, nn_vert2 = eng.mesh_loss_grad(sg, vg, want_neighbours=True)
    loss_only, grad_only = eng.mesh_loss_grad(sg, vg)
    # 5: repeatable bit for bit, with and without the neighbour outputs
    assert torch.equal(grad.view(torch.int32), grad2.view(torch.int32)) and torch.equal(grad.view(torch.int32), grad_only.view(torch.int32))
    assert torch.equal(loss.view(torch.int32), loss2.view(torch.int32)) and torch.equal(loss.view(torch.int32), loss_only.view(torch.int32))
    assert torch.equal(nn_pix, nn_pix2) and torch.equal(nn_vert, nn_vert2)
    loss, fwd = float(loss), float(fwd)
    grad, nn_pix, nn_vert = grad.cpu().numpy(), nn_pix.cpu().numpy(), nn_vert.cpu().numpy()
    # 1: structure
    on = seg > 0
    assert ((nn_pix >= 0) == on).all() and nn_pix.max() < P and (nn_pix[~on] == -1).all()
    for b in range(B):
        if on[b].any():
            assert (nn_vert[b] >= 0).all() and (nn_vert[b] < H * W).all()
            assert on[b].reshape(-1)[nn_vert[b]].all(), "nn_vert points off the silhouette"
        else:
            assert (nn_vert[b] == -1).all()
    # 2: the neighbours are the forward's and are nearest
    l64 = [R.loss_from_neighbours(seg[b], v[b], nn_pix[b], nn_vert[b]) for b in range(B)]
    exact = exact_loss(name, seg, v)
    t64, tex = sum(l64), sum(exact)
    e_fwd, e_exact, e_out = abs(t64 - fwd) / abs(fwd), abs(t64 - tex) / abs(tex), abs(loss - fwd) / abs(fwd)
    # 3: the gradient over those neighbours
    assert np.isfinite(grad).all()
    worst, n_on_pixel = 0.0, 0
    for b in range(B):
        want = R.closed_form_grad(seg[b], v[b], nn_pix[b], nn_vert[b])
        zero = (want == 0.0).all(1)
        assert (grad[b][zero] == 0.0).all(), "image %d: %d vertices with an exactly zero reference gradient are not exactly zero" % (
            b, int((grad[b][zero] != 0.0).any(1).sum()))
        if on[b].any():
            px = np.stack([nn_vert[b] % W, nn_vert[b] // W], 1)
            n_on_pixel += int((px == v[b]).all(1).sum())
        n = np.linalg.norm(want)
        if n == 0.0:
            assert not on[b].any() and (grad[b] == 0.0).all()
            continue
        worst = max(worst, np.linalg.norm(grad[b].astype(np.float64) - want) / n)
    line = ("%-28s loss64(nn) vs hpe_mesh_loss %.2e (<= 1e-5) | vs exact search %.2e (<= 1.5e-4) | out[0] vs hpe_mesh_loss %.2e (<= 2e-6, %s) | "
            "grad rel L2 %.2e (<= 1e-4) | vertices on their pixel %d" % (name, e_fwd, e_exact, e_out, "bit-equal" if loss == fwd else "not bit-equal",
                                                                        worst, n_on_pixel))
    print(line)
    assert e_fwd <= 1e-5 and e_exact <= 1.5e-4 and e_out <= 2e-6 and worst <= TOL, line
    return n_on_pixel


@pytest.mark.parametrize("mode", MODES)
def test_lsp_smpl_case(engine, loss_engines, mode):
    seg, v = case_lsp(engine)
    check_case(loss_engines[mode], "lsp + smpl", seg, v)


@pytest.mark.parametrize("mode", MODES)
def test_degenerate_and_far(loss_engines, mode):
    seg, v = case_degenerate()
    n_on = check_case(loss_engines[mode], "degenerate and far", seg, v)
    assert n_on > 0, "the lattice image must hold vertices lying exactly on silhouette pixels"
    seg, v = case_edges()
    assert check_case(loss_engines[mode], "edge cases", seg, v) > 0


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("H,W,P", GEOMETRIES)
def test_other_geometries(loss_engines, mode, H, W, P):
    seg, v = case_geometry(H, W, P)
    check_case(loss_engines[mode], "geometry %dx%d P=%d" % (H, W, P), seg, v)


def test_finalized_context_and_argument_checks(engine):
    """the finalized engine's workspace (sized at finalize) serves the call; bad arguments are refused before any launch"""
    seg, v = case_lsp(engine)
    check_case(engine, "lsp + smpl", seg, v)
    sg, vg = gpu(seg), gpu(v)
    out = torch.zeros(4, device="cuda")
    with pytest.raises(hpe_amd.HpeError):
        hpe_amd._lib.check(engine.lib.hpe_mesh_loss_grad(engine._h, sg.data_ptr(), vg.data_ptr(), 3, 224, 224, 6890, out.data_ptr(), None, None, None, None))
    with pytest.raises(ValueError):
        engine.mesh_loss_grad(sg, vg[:2])


def test_autograd_wiring(engine):
    """6: theta -> engine.smpl -> mesh_reprojection_loss -> backward equals smpl_backward of the gradient mesh_loss_grad returns; without
    requires_grad the old path is taken and returns the same value."""
    B = 3
    seg, _ = synthetic.make_lsp_targets(B, seed=21)
    sg = gpu(seg)
    th = gpu(make_theta(B, seed=22, special=False))
    theta = th.clone().requires_grad_(True)
    v2d = engine.smpl(theta, want=("verts2d",))["verts2d"]
    loss = hpe_amd.mesh_reprojection_loss(engine, sg, v2d)
    assert loss.grad_fn is not None
    loss.backward()
    plain_v = engine.smpl(th, want=("verts2d",))["verts2d"]
    l2, g = engine.mesh_loss_grad(sg[..., 0].contiguous(), plain_v)
    want = engine.smpl_backward(th, {"verts2d": g})
    assert torch.equal(theta.grad, want) and float(theta.grad.abs().max()) > 0.0
    plain = hpe_amd.mesh_reprojection_loss(engine, sg, plain_v)
    assert plain.grad_fn is None and torch.equal(plain, engine.mesh_loss(sg[..., 0].contiguous(), plain_v))
    assert abs(float(plain) - float(loss.detach())) <= 2e-6 * abs(float(plain))
    # a cotangent scales it; no_grad takes the old path
    theta2 = th.clone().requires_grad_(True)
    (0.001 * hpe_amd.mesh_reprojection_loss(engine, sg, engine.smpl(theta2, want=("verts2d",))["verts2d"])).backward()
    assert float((theta2.grad - 0.001 * want).norm()) <= 1e-5 * float((0.001 * want).norm())  # linear in the cotangent, to fp32 round-off
    with torch.no_grad():
        assert hpe_amd.mesh_reprojection_loss(engine, sg, v2d).grad_fn is None


# ------------------------------------------------------------------------------------------------ fit_reprojection
FIT_B, FIT_STEPS, FIT_LR = 2, 30, 0.01


def fit_inputs(model):
    """theta* -> its own projected vertices, splatted (rounded) and dilated 3x3 = the silhouette; the start is theta* with the camera
    translation offset"""
    star = make_theta(FIT_B, seed=3, special=False)
    star[:, 0] = 0.8
    star[:, 1:3] = 0.0
    v = SmplTorch(model, torch.float64)(torch.from_numpy(star).to(torch.float64))["verts2d"].numpy()
    seg = np.zeros((FIT_B, 224, 224), np.float32)
    for b in range(FIT_B):
        x, y = np.rint(v[b, :, 0]).astype(int), np.rint(v[b, :, 1]).astype(int)
        ok = (x >= 0) & (x < 224) & (y >= 0) & (y < 224)
        seg[b, y[ok], x[ok]] = 1.0
        pad = np.pad(seg[b], 1)
        seg[b] = np.max([pad[1 + dy:225 + dy, 1 + dx:225 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1)], 0)
    theta0 = star.copy()
    theta0[:, 1] += 0.12
    theta0[:, 2] -= 0.09
    return seg, theta0


def ref_fit_loop(model, seg, theta0, steps=FIT_STEPS, lr=FIT_LR):
    """the same loop on the CPU in float64: SmplTorch + the torch restatement of the loss (the library's convention at distance 0),
    Adam on the camera columns alone, 0.001 x the mesh loss -> the unweighted loss before each step"""
    ref = SmplTorch(model, torch.float64)
    cam = torch.from_numpy(theta0[:, :3]).to(torch.float64).clone().requires_grad_(True)
    rest = torch.from_numpy(theta0[:, 3:]).to(torch.float64)
    opt = torch.optim.Adam([cam], lr=lr)
    losses = []
    for _ in range(steps + 1):
        opt.zero_grad()
        loss = R.mesh_loss_torch(seg, ref(torch.cat([cam, rest], 1))["verts2d"], safe_norm=True)
        losses.append(float(loss.detach()))
        (0.001 * loss).backward()
        opt.step()
    return np.asarray(losses)


def test_fit_reprojection(engine, model):
    """7: 30 Adam steps on the camera against the silhouette alone.  The float64 reference loop reaches final / initial = r_ref (<= 0.5
    by the choice of inputs); the library's loop must reach (1 + r_ref) / 2 or better, half the reference's reduction (neighbour
    flips and fp32 make the two trajectories part ways)."""
    seg, theta0 = fit_inputs(model)
    lr_ref = ref_fit_loop(model, seg, theta0)
    r_ref = lr_ref[-1] / lr_ref[0]
    print("reference loop: loss %.4f -> %.4f, r_ref = %.4f" % (lr_ref[0], lr_ref[-1], r_ref))
    assert r_ref <= 0.5, lr_ref
    theta, losses = hpe_amd.fit_reprojection(engine, gpu(theta0), seg_gts=gpu(seg), steps=FIT_STEPS, lr=FIT_LR, fit=("cam",))
    assert tuple(losses.shape) == (FIT_STEPS, 2) and losses.is_cuda and tuple(theta.shape) == (FIT_B, 85)
    lh = losses.cpu().numpy().astype(np.float64)
    assert float(np.abs(lh[:, 0]).max()) == 0.0 and np.isfinite(lh).all()
    assert torch.equal(theta[:, 3:], gpu(theta0)[:, 3:])  # only the camera was fitted
    final = float(engine.mesh_loss(gpu(seg), engine.smpl(theta, want=("verts2d",))["verts2d"]))
    r = final / lh[0, 1]
    msg = "library loop: loss %.4f -> %.4f, r = %.4f against (1 + r_ref) / 2 = %.4f\n%s" % (lh[0, 1], final, r, (1 + r_ref) / 2, lh[:, 1])
    print(msg)
    assert abs(lh[0, 1] - lr_ref[0]) <= 1e-3 * lr_ref[0], msg  # the same starting point
    assert r <= (1.0 + r_ref) / 2.0, msg
    with pytest.raises(ValueError):
        hpe_amd.fit_reprojection(engine, gpu(theta0), steps=2)
    # both terms together: shapes and finiteness
    _, kp_gt = synthetic.make_lsp_targets(FIT_B, seed=5)
    _, both = hpe_amd.fit_reprojection(engine, gpu(theta0), kp_gt=gpu(kp_gt), seg_gts=gpu(seg)[..., None], steps=3)
    assert tuple(both.shape) == (3, 2) and torch.isfinite(both).all() and float(both[:, 0].min()) > 0.0 and float(both[:, 1].min()) > 0.0


def test_graph_capture(engine):
    """8: hpe_smpl + hpe_mesh_loss_grad + hpe_smpl_backward captured and replayed give the eager result bit for bit."""
    B = 4
    seg, _ = synthetic.make_lsp_targets(B, seed=41)
    sg = gpu(seg[..., 0])
    th = gpu(make_theta(B, seed=42, special=False))
    v = engine.smpl(th, want=("verts2d",))["verts2d"]
    e_loss, e_g = engine.mesh_loss_grad(sg, v)
    e_loss, e_theta = e_loss.clone(), engine.smpl_backward(th, {"verts2d": e_g}).clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fwd = engine.smpl(th, want=("verts2d",))
        loss, g = engine.mesh_loss_grad(sg, fwd["verts2d"])
        gt = engine.smpl_backward(th, {"verts2d": g})
    gt.zero_()
    g.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(gt.view(torch.int32), e_theta.view(torch.int32))
    assert torch.equal(g.view(torch.int32), e_g.view(torch.int32))
    assert torch.equal(loss.view(torch.int32), e_loss.view(torch.int32))
