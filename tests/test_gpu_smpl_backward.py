"""GPU tests of the SMPL backward (run with -m gpu on an MI355X): hpe_smpl_backward / hpe_kp_loss_backward against the float64
autograd of the torch restatement (tests/smpl_torch_ref.py) and against closed forms, the autograd wiring, fit_keypoints and
graph capture.  Synthetic SMPL model, one engine for the module, fixed seeds.

Bar: per image and per group (cam / pose / betas)  ||g_hip - g_ref64|| / ||g_ref64|| <= 1e-4, the project's fp32 parity bar.
A group whose reference gradient is exactly zero (structurally: e.g. betas under a cotangent on Rs alone) must come back
exactly zero."""
import numpy as np
import pytest
import torch

import hpe_amd
from hpe_amd import synthetic

from smpl_torch_ref import SmplTorch, make_theta

pytestmark = pytest.mark.gpu
TOL = 1e-4
MAX_BATCH = 128
OUTPUTS = ("verts", "joints", "J_transformed", "kp2d", "verts2d", "Rs", "cams", "theta")
GROUPS = (("cam", 0, 3), ("pose", 3, 75), ("betas", 75, 85))


@pytest.fixture(scope="module")
def model():
    return synthetic.make_smpl_model()


@pytest.fixture(scope="module")
def engine(model):
    e = hpe_amd.HpeEngine(device=0, max_batch=MAX_BATCH)
    e.load_smpl(model)
    e.finalize()
    yield e
    e.close()


@pytest.fixture(scope="module")
def refs(model):
    return {torch.float64: SmplTorch(model, torch.float64), torch.float32: SmplTorch(model, torch.float32)}


def cotangents(B, K, seed):
    g = torch.Generator().manual_seed(seed)
    shapes = dict(verts=(B, 6890, 3), joints=(B, K, 3), J_transformed=(B, 24, 3), kp2d=(B, K, 2), verts2d=(B, 6890, 2), Rs=(B, 24, 3, 3),
                  cams=(B, 3), theta=(B, 85))
    return {k: torch.randn(shapes[k], generator=g, dtype=torch.float32) for k in OUTPUTS}


def ref_grads(ref, theta, cot_sets, dtype):
    """one forward of the restatement, then one autograd pass per cotangent set"""
    x = torch.from_numpy(theta).to(dtype).requires_grad_(True)
    out = ref(x)
    res = []
    for cs in cot_sets:
        names = sorted(cs)
        res.append(torch.autograd.grad([out[k] for k in names], x, [cs[k].to(dtype) for k in names], retain_graph=True)[0].to(torch.float64).numpy())
    return res


def group_errors(g, g64):
    """-> (worst relative distance over images and groups, its label); exact-zero reference groups must be exactly zero"""
    worst, label = 0.0, ""
    for b in range(g64.shape[0]):
        for name, lo, hi in GROUPS:
            n = np.linalg.norm(g64[b, lo:hi])
            d = np.linalg.norm(g[b, lo:hi].astype(np.float64) - g64[b, lo:hi])
            if n == 0.0:
                assert d == 0.0, "image %d %s: reference gradient is exactly zero, got norm %.3g" % (b, name, d)
                continue
            if d / n > worst:
                worst, label = d / n, "image %d %s" % (b, name)
    return worst, label


@pytest.mark.parametrize("B", [1, 5, 37, MAX_BATCH + 3])
def test_gradient_parity(engine, refs, B):
    """4: cotangents on every output at once and on each output alone; image 0 at the exact mean pose, image 1 with its pose
    scaled by 1e-4, image 2 with a rotation of angle near pi (B permitting)."""
    theta = make_theta(B, seed=10 + B)
    cot = cotangents(B, engine.num_kp, seed=20 + B)
    sets = [dict(cot)] + [{k: cot[k]} for k in OUTPUTS]
    g64 = ref_grads(refs[torch.float64], theta, sets, torch.float64)
    g32 = ref_grads(refs[torch.float32], theta, sets, torch.float32)
    th = torch.from_numpy(theta).cuda()
    report, worst_all = [], 0.0
    for cs, r64, r32 in zip(sets, g64, g32):
        got = engine.smpl_backward(th, {k: v.cuda() for k, v in cs.items()}).cpu().numpy()
        assert np.isfinite(got).all()
        e_hip, where = group_errors(got, r64)
        e_f32, _ = group_errors(r32, r64)
        name = "all" if len(cs) > 1 else next(iter(cs))
        report.append("%-13s hip %.3g (%s) | fp32 autograd of the restatement %.3g" % (name, e_hip, where, e_f32))
        worst_all = max(worst_all, e_hip)
    msg = "B=%d worst %.3g\n" % (B, worst_all) + "\n".join(report)
    print(msg)
    assert worst_all <= TOL, msg


def test_closed_form_zero_pose_betas(engine, model):
    """5a: at pose = 0 every A_j = [I | 0] whatever beta, so verts = wsum * v_posed (wsum = the row sums of the skinning weights) and
    d(sum c . verts) / d beta_k = sum c . wsum . shapedirs[:, :, k]."""
    B = 3
    theta = make_theta(B, seed=31, special=False)
    theta[:, 3:75] = 0.0
    c = cotangents(B, engine.num_kp, seed=32)["verts"]
    got = engine.smpl_backward(torch.from_numpy(theta).cuda(), {"verts": c.cuda()}).cpu().numpy().astype(np.float64)
    wsum = np.asarray(model["weights"], np.float32).astype(np.float64).sum(1)
    sd = np.asarray(model["shapedirs"], np.float32).astype(np.float64)
    want = np.einsum("bvc,v,vck->bk", c.numpy().astype(np.float64), wsum, sd)
    err = np.linalg.norm(got[:, 75:] - want, axis=1) / np.linalg.norm(want, axis=1)
    print("zero-pose d/dbeta rel", err)
    assert err.max() <= 1e-5, err


def test_closed_form_camera(engine):
    """5b: kp2d = s (joints_xy + t): d kp2d / d s = joints_xy + t, d kp2d / d t = s."""
    B = 6
    theta = make_theta(B, seed=33, special=False)
    th = torch.from_numpy(theta).cuda()
    g = cotangents(B, engine.num_kp, seed=34)["kp2d"]
    joints = engine.smpl(th, want=("joints",))["joints"].cpu().numpy().astype(np.float64)
    got = engine.smpl_backward(th, {"kp2d": g.cuda()}).cpu().numpy().astype(np.float64)
    g64, t64 = g.numpy().astype(np.float64), theta.astype(np.float64)
    want_s = (g64 * (joints[:, :, :2] + t64[:, None, 1:3])).sum((1, 2))
    want_t = t64[:, 0:1] * g64.sum(1)
    e_s = np.abs(got[:, 0] - want_s) / np.abs(want_s)
    e_t = np.abs(got[:, 1:3] - want_t) / np.abs(want_t)
    print("camera closed form rel: s", e_s, "t", e_t.max(0))
    assert e_s.max() <= 1e-5 and e_t.max() <= 1e-5, (e_s, e_t)


def test_closed_form_root_rotation_only(engine, model):
    """5c: with only the root rotated every G_j has the rotation R0 and A_j = [R0 | (I - R0) J_0(beta)], so
    verts = wsum (R0 v_shaped + (I - R0) J_0) and, J_0 being linear in beta through the joint basis,
    d(sum c . verts) / d beta_k = sum_v wsum_v c_v . (R0 shapedirs_k[v] + (I - R0) Jb_k[0])."""
    B = 3
    theta = make_theta(B, seed=35, special=False)
    theta[:, 6:75] = 0.0
    th = torch.from_numpy(theta).cuda()
    c = cotangents(B, engine.num_kp, seed=36)["verts"]
    R0 = engine.smpl(th, want=("Rs",))["Rs"][:, 0].cpu().numpy().astype(np.float64)
    got = engine.smpl_backward(th, {"verts": c.cuda()}).cpu().numpy().astype(np.float64)
    wsum = np.asarray(model["weights"], np.float32).astype(np.float64).sum(1)
    sd = np.asarray(model["shapedirs"], np.float32).astype(np.float64)
    jb0 = np.einsum("v,vck->ck", np.asarray(model["J_regressor"], np.float32).astype(np.float64)[0], sd)  # d J_0 / d beta_k
    c64 = c.numpy().astype(np.float64) * wsum[None, :, None]
    want = np.einsum("bvr,brc,vck->bk", c64, R0, sd) + np.einsum("br,brc,ck->bk", c64.sum(1), np.eye(3)[None] - R0, jb0)
    err = np.linalg.norm(got[:, 75:] - want, axis=1) / np.linalg.norm(want, axis=1)
    print("root-rotation d/dbeta rel", err)
    assert err.max() <= 1e-5, err


def test_pass_through_and_all_null(engine):
    """6: cotangents on theta or cams alone come back unchanged; no cotangent at all gives exact zeros."""
    B = 9
    th = torch.from_numpy(make_theta(B, seed=41)).cuda()
    cot = cotangents(B, engine.num_kp, seed=42)
    g = engine.smpl_backward(th, {"theta": cot["theta"].cuda()}).cpu()
    assert torch.equal(g, cot["theta"])
    g = engine.smpl_backward(th, {"cams": cot["cams"].cuda()}).cpu()
    assert torch.equal(g[:, :3], cot["cams"]) and float(g[:, 3:].abs().max()) == 0.0
    g = engine.smpl_backward(th, {})
    assert float(g.abs().max()) == 0.0


def test_bitwise_repeatable(engine):
    """7: the same inputs twice at B = 100 give the same bits (fixed summation order, no atomics)."""
    B = 100
    th = torch.from_numpy(make_theta(B, seed=51)).cuda()
    cot = {k: v.cuda() for k, v in cotangents(B, engine.num_kp, seed=52).items()}
    a = engine.smpl_backward(th, cot).clone()
    junk = engine.smpl_backward(torch.from_numpy(make_theta(B, seed=53)).cuda(), {"kp2d": cot["kp2d"]})  # other work in between
    b = engine.smpl_backward(th, cot)
    assert junk.shape == a.shape and torch.equal(a, b)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_kp_loss_backward(engine):
    """8: d loss / d pred = -vis sign(gt - pred) / (2 #visible) exactly; zeros (no NaN) when nothing is visible."""
    g = torch.Generator().manual_seed(61)
    B, K = 7, 19
    gt = torch.randn((B, K, 3), generator=g)
    gt[:, :, 2] = (torch.rand((B, K), generator=g) > 0.3).float()
    pred = torch.randn((B, K, 2), generator=g)
    pred[0, :3] = gt[0, :3, :2]  # gt == pred -> zero gradient there
    gt[0, :3, 2] = 1.0
    p = pred.cuda().requires_grad_(True)
    loss = hpe_amd.kp_reprojection_loss(gt.cuda(), p)
    plain = hpe_amd.kp_reprojection_loss(gt.cuda(), pred.cuda())
    assert plain.grad_fn is None and torch.equal(loss.detach(), plain)
    loss.backward()
    vis = gt[:, :, 2:3]
    want = -vis * torch.sign(gt[:, :, :2] - pred) / (2.0 * float((vis != 0).sum()))
    assert torch.equal(p.grad.cpu(), want + 0.0)
    assert float(p.grad[0, :3].abs().max()) == 0.0
    # an incoming cotangent scales it
    p2 = pred.cuda().requires_grad_(True)
    (60.0 * hpe_amd.kp_reprojection_loss(gt.cuda(), p2)).backward()
    assert torch.allclose(p2.grad.cpu(), 60.0 * want, rtol=1e-6, atol=0.0)
    gt0 = gt.clone()
    gt0[:, :, 2] = 0.0
    p3 = pred.cuda().requires_grad_(True)
    hpe_amd.kp_reprojection_loss(gt0.cuda(), p3).backward()
    assert float(p3.grad.abs().max()) == 0.0 and torch.isfinite(p3.grad).all()


def test_autograd_wiring(engine, refs):
    """9: SMPL(...)(beta, theta, get_skin=True) backpropagates to both inputs when they require grad; without requires_grad it is
    today's path: no grad_fn, bits equal to engine.smpl called directly."""
    B = 5
    th85 = make_theta(B, seed=71)
    smpl = hpe_amd.SMPL(None, engine=engine)
    beta = torch.from_numpy(th85[:, 75:]).cuda().requires_grad_(True)
    pose = torch.from_numpy(th85[:, 3:75]).cuda().requires_grad_(True)
    verts, joints, Rs = smpl(beta, pose, get_skin=True)
    assert verts.grad_fn is not None and smpl.J_transformed.grad_fn is not None
    cot = cotangents(B, engine.num_kp, seed=72)
    ((verts * cot["verts"].cuda()).sum() + (joints * cot["joints"].cuda()).sum() + (Rs * cot["Rs"].cuda()).sum()
     + (smpl.J_transformed * cot["J_transformed"].cuda()).sum()).backward()
    full = th85.copy()
    full[:, 0], full[:, 1:3] = 1.0, 0.0  # SMPL.__call__ runs with the identity camera
    r64 = ref_grads(refs[torch.float64], full, [{k: cot[k] for k in ("verts", "joints", "Rs", "J_transformed")}], torch.float64)[0]
    got = np.zeros((B, 85), np.float32)
    got[:, 3:75], got[:, 75:] = pose.grad.cpu().numpy(), beta.grad.cpu().numpy()
    r64[:, :3] = 0.0
    worst, where = group_errors(got, r64)
    assert worst <= TOL, (worst, where)
    # forward-only path untouched
    v2, j2, R2 = smpl(beta.detach(), pose.detach(), get_skin=True)
    direct = engine.smpl(torch.from_numpy(full).cuda(), want=("verts", "joints", "J_transformed", "Rs"))
    assert v2.grad_fn is None and j2.grad_fn is None and R2.grad_fn is None and smpl.J_transformed.grad_fn is None
    assert torch.equal(v2, direct["verts"]) and torch.equal(j2, direct["joints"]) and torch.equal(R2, direct["Rs"])
    assert torch.equal(smpl.J_transformed, direct["J_transformed"]) and torch.equal(v2, verts.detach())


def _adam_loop(ref, theta0, kp_gt, dtype, steps, lr):
    x = torch.from_numpy(theta0).to(dtype).clone().requires_grad_(True)  # Adam updates x in place: never the caller's array
    gt = torch.from_numpy(kp_gt).to(dtype)
    opt = torch.optim.Adam([x], lr=lr)
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        vis = gt[:, :, 2:3]
        loss = (vis * (ref(x)["kp2d"] - gt[:, :, :2]).abs()).sum() / (2.0 * (vis != 0).sum())
        losses.append(float(loss.detach()))
        (60.0 * loss).backward()
        opt.step()
    return np.asarray(losses, np.float64)


def test_fit_keypoints(engine, refs):
    """10: 10 Adam steps at lr 0.01 from theta* with pose + 0.1 N and cam + 0.05, all keypoints visible.  The float64 restatement
    loop must at least halve the loss; the library's per-step losses follow that trajectory within 4x the largest per-step relative
    distance between the float32 and the float64 restatement loops."""
    B, steps, lr = 4, 10, 0.01
    g = np.random.RandomState(0)
    star = make_theta(B, seed=0, special=False)
    kp = refs[torch.float64](torch.from_numpy(star).to(torch.float64))["kp2d"].numpy()
    kp_gt = np.concatenate([kp, np.ones((B, kp.shape[1], 1))], 2).astype(np.float32)
    theta0 = star.copy()
    theta0[:, 3:75] += (0.1 * g.randn(B, 72)).astype(np.float32)
    theta0[:, :3] += 0.05
    l64 = _adam_loop(refs[torch.float64], theta0, kp_gt, torch.float64, steps, lr)
    l32 = _adam_loop(refs[torch.float32], theta0, kp_gt, torch.float32, steps, lr)
    assert l64[-1] <= 0.5 * l64[0], l64
    theta, losses = hpe_amd.fit_keypoints(engine, torch.from_numpy(theta0).cuda(), torch.from_numpy(kp_gt).cuda(), steps=steps, lr=lr)
    lh = losses.cpu().numpy().astype(np.float64)
    d32 = float((np.abs(l32 - l64) / l64).max())
    dh = float((np.abs(lh - l64) / l64).max())
    msg = "fp64 %s\nhip  %s\nper-step rel distance: hip %.3g, fp32 restatement %.3g (bound 4x = %.3g)" % (l64, lh, dh, d32, 4 * d32)
    print(msg)
    assert theta.shape == (B, 85) and losses.is_cuda and np.isfinite(lh).all()
    assert dh <= 4.0 * d32, msg


def test_graph_capture(engine):
    """11: one hpe_smpl + hpe_smpl_backward pair captured on a side stream and replayed gives the eager gradient bit for bit."""
    B = 12
    th = torch.from_numpy(make_theta(B, seed=81)).cuda()
    cot = {k: v.cuda() for k, v in cotangents(B, engine.num_kp, seed=82).items() if k in ("verts", "kp2d", "Rs")}
    eager = engine.smpl_backward(th, cot).clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # torch captures on a side stream of its own
        fwd = engine.smpl(th, want=("verts", "kp2d", "Rs"))
        grad = engine.smpl_backward(th, cot)
    grad.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(grad.view(torch.int32), eager.view(torch.int32))
    assert torch.equal(fwd["kp2d"], engine.smpl(th, want=("kp2d",))["kp2d"])
