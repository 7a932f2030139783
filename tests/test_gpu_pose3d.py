"""GPU tests of hpe_pose3d_scores and what is built on it (run with -m gpu on an MI355X; DESIGN.md "3-D pose scores").

The reference is tests/pose3d_ref.py (float64, np.linalg.svd) on the same float32 inputs.  Every output is held to
    |out - ref| <= 1e-6 * max(|ref|, rms radius of the ground-truth cloud)
(the radius about the cloud's own mean, over the scored points; the joint cloud's for the joint outputs, the vertex cloud's for the vertex
outputs): float32 rounding of the outputs is 6e-8 relative, everything before it is float64, so the bar is about 16 roundings wide.
Shapes: B in {1, 3}, n_stage in {1, 3}, K = 19 with 14 scored, P in {1, 70, 257, 6890} -- below one wave, no multiple of the wave or of
the workgroup, and the real mesh."""
import ctypes as C

import numpy as np
import pytest
import torch

import hpe_amd
from hpe_amd import metrics

import pose3d_ref as PR
from test_gpu_trainer import data, make_trainer, weights  # noqa: F401  (fixtures of the small trainer)

pytestmark = pytest.mark.gpu
K, J = 19, 14
BAR = 1e-6


def rotation(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    x, y, z = axis
    S = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
    return np.eye(3) + np.sin(angle) * S + (1 - np.cos(angle)) * S @ S


def clouds(seed, n, B, P, noise=0.05, size=0.3):
    """ground truth of body size and per stage a rotated, scaled, shifted, noisy copy of it, float32"""
    rng = np.random.RandomState(seed)
    gt_j, gt_v = rng.standard_normal((B, K, 3)) * size, rng.standard_normal((B, P, 3)) * size
    pj, pv = np.zeros((n, B, K, 3)), np.zeros((n, B, P, 3))
    for s in range(n):
        for i in range(B):
            R, sc, t = rotation(rng.standard_normal(3), rng.uniform(0, 1.0)), rng.uniform(0.8, 1.2), rng.standard_normal(3) * 0.2
            pj[s, i] = sc * gt_j[i] @ R.T + t + rng.standard_normal((K, 3)) * noise
            pv[s, i] = sc * gt_v[i] @ R.T + t + rng.standard_normal((P, 3)) * noise
    return [a.astype(np.float32) for a in (pj, gt_j, pv, gt_v)]


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def run(pj, gt_j, pv=None, gt_v=None, w=None, num_joints=J, roots=(2, 3)):
    out = metrics.pose3d_scores([dev(x) for x in pj], dev(gt_j), None if pv is None else [dev(x) for x in pv], dev(gt_v), dev(w), roots=roots,
                                num_joints=num_joints)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def ref(pj, gt_j, pv=None, gt_v=None, w=None, num_joints=J, roots=(2, 3)):
    w = np.ones(gt_j.shape[:2]) if w is None else np.array(w, np.float64)
    w[:, num_joints:] = 0
    return PR.pose3d_scores(pj, gt_j, w, pv, gt_v, roots), w


def radius(cloud, sel=None):
    c = np.asarray(cloud, np.float64)
    c = c if sel is None else c[np.asarray(sel) > 0]
    return float(np.sqrt(((c - c.mean(0)) ** 2).sum(1).mean())) if len(c) else 0.0


def within(out, want, rad, what):
    """the bar, elementwise; NaN must meet NaN.  The ratio is printed before it is asserted (shown with -s: the source of the figure in
    DESIGN.md's "Measured") and returned"""
    out, want = np.asarray(out, np.float64), np.asarray(want, np.float64)
    assert out.shape == want.shape, what
    assert np.array_equal(np.isnan(out), np.isnan(want)), (what, out, want)
    ok = ~np.isnan(want)
    if not ok.any():
        return 0.0
    diff, denom = np.abs(out[ok] - want[ok]), np.maximum(np.abs(want[ok]), rad)
    ratio = np.where(diff == 0, 0.0, diff / np.where(denom > 0, denom, 1.0))
    ratio[(denom == 0) & (diff > 0)] = np.inf  # a reference of exactly 0 with no radius to measure against: only 0 will do
    r = float(ratio.max())
    print("pose3d %s: worst |out - ref| / max(|ref|, radius) = %.3g" % (what, r))
    assert r <= BAR, (what, r)
    return r


def check(got, pj, gt_j, pv=None, gt_v=None, w=None, what="", xform=True, **kw):
    (err, summ, xf), w = ref(pj, gt_j, pv, gt_v, w, **kw)
    g_err, g_summ, g_xf = got
    n, B = err.shape[:2]
    for i in range(B):
        rj = radius(gt_j[i], w[i])
        rv = radius(gt_v[i]) if gt_v is not None else 0.0
        within(g_err[:, i], err[:, i], rj, what + " joint_err")
        within(g_summ[:, i, :2], summ[:, i, :2], rj, what + " mpjpe")
        within(g_summ[:, i, 2:4], summ[:, i, 2:4], rv, what + " pve")
        assert np.array_equal(g_summ[:, i, 4:], summ[:, i, 4:]), (what, g_summ[:, i, 4:], summ[:, i, 4:])  # count and flags: exact
        if xform:
            within(g_xf[:, i, 0], xf[:, i, 0], rj, what + " joint fit")
            within(g_xf[:, i, 1], xf[:, i, 1], rv, what + " vertex fit")
    return err, summ, xf


@pytest.mark.parametrize("P", [1, 70, 257, 6890])
@pytest.mark.parametrize("B,n", [(1, 1), (3, 3)])
def test_random_clouds_match_the_float64_reference(B, n, P):
    pj, gt_j, pv, gt_v = clouds(100 + P + B, n, B, P)
    got = run(pj, gt_j, pv, gt_v)
    err, summ, xf = check(got, pj, gt_j, pv, gt_v, what="random B%d n%d P%d" % (B, n, P))
    assert got[0].shape == (n, B, 2, K) and got[1].shape == (n, B, 6) and got[2].shape == (n, B, 2, 13)
    assert (got[0][..., J:] == -1).all() and (got[0][..., :J] > 0).all() and (got[1][..., 4] == J).all()
    assert (got[1][..., 5] == (PR.FLAG_PA_VERTS if P < 3 else 0)).all()  # one vertex: its fit is undefined, PVE is not
    assert np.isfinite(got[1][..., 2]).all() and np.isnan(got[1][..., 3]).all() == (P < 3)


def test_identity_scores_exactly_zero():
    _, gt_j, _, gt_v = clouds(1, 1, 3, 257)
    err, summ, xf = run([gt_j] * 2, gt_j, [gt_v] * 2, gt_v)
    assert (err[:, :, 0, :J] == 0).all() and (summ[:, :, 0] == 0).all() and (summ[:, :, 2] == 0).all()  # x - y is exact
    check((err, summ, xf), np.stack([gt_j] * 2), gt_j, np.stack([gt_v] * 2), gt_v, what="identity")
    assert np.abs(xf[..., 0] - 1).max() < 1e-5 and np.abs(xf[..., 1:10] - np.eye(3).reshape(-1)).max() < 1e-5 and np.abs(xf[..., 10:]).max() < 1e-5


def test_known_similarity_transform_is_recovered():
    _, gt_j, _, gt_v = clouds(2, 1, 3, 70)
    gt_j[:, J:] = 0
    R, sc, t = rotation([1, -2, 0.5], 0.9), 1.25, np.array([0.3, -0.7, 2.0])
    # prediction = the inverse transform of the ground truth, so the fit that maps it back is (sc, R, t)
    pj = (((gt_j.astype(np.float64) - t) @ R) / sc).astype(np.float32)[None]
    pv = (((gt_v.astype(np.float64) - t) @ R) / sc).astype(np.float32)[None]
    got = run(pj, gt_j, pv, gt_v)
    check(got, pj, gt_j, pv, gt_v, what="similarity")
    for i in range(3):  # the clouds were rounded to float32 after the transform: the residual is that rounding, far under the bar's radius
        assert got[0][0, i, 1, :J].max() <= BAR * radius(gt_j[i, :J]) and got[1][0, i, 3] <= BAR * radius(gt_v[i])
    want = np.concatenate([[sc], R.reshape(-1), t])
    assert np.abs(got[2] - want).max() < 1e-5, np.abs(got[2] - want).max()


def test_mirrored_ground_truth_is_not_reflected():
    pj, gt_j, pv, gt_v = clouds(3, 1, 3, 257, noise=0.0)
    gt_j, gt_v = gt_j * np.float32([1, 1, -1]), gt_v * np.float32([1, 1, -1])
    got = run(pj, gt_j, pv, gt_v)
    check(got, pj, gt_j, pv, gt_v, what="mirrored")
    Rs = got[2][..., 1:10].reshape(-1, 3, 3).astype(np.float64)
    assert np.abs(np.linalg.det(Rs) - 1).max() < 1e-5 and (got[1][..., 1] > 0.01).all() and (got[1][..., 3] > 0.01).all()


def test_coplanar_cloud_errors():
    """rank-2 K: R is unique but touchy in the plane's normal, so only the errors are compared"""
    pj, gt_j, pv, gt_v = clouds(4, 3, 1, 70)
    pj[..., 2] = 0.25
    pv[..., 2] = -1.0
    got = run(pj, gt_j, pv, gt_v)
    check(got, pj, gt_j, pv, gt_v, what="coplanar", xform=False)
    gt_j[..., 2], gt_v[..., 2] = 0.5, 0.5  # both sides in a plane
    check(run(pj, gt_j, pv, gt_v), pj, gt_j, pv, gt_v, what="coplanar both", xform=False)


def test_weights_with_zeros():
    pj, gt_j, pv, gt_v = clouds(5, 3, 3, 70)
    w = np.ones((3, K), np.float32)
    w[0, [0, 7]] = 0            # two unscored joints
    w[1, 3] = 0                 # an unscored hip: no root
    w[2, :] = 0
    w[2, [2, 3]] = 0.5          # two scored joints, the hips: a root, no fit
    got = run(pj, gt_j, pv, gt_v, w)
    check(got, pj, gt_j, pv, gt_v, w, what="weights")
    err, summ, xf = got
    assert (err[:, 0, :, [0, 7]] == -1).all() and (err[:, 0, :, 1] > 0).all() and (summ[:, 0, 4] == 12).all() and (summ[:, 0, 5] == 0).all()
    assert (summ[:, 1, 5] == PR.FLAG_ROOT).all() and np.isnan(summ[:, 1, [0, 2]]).all() and np.isfinite(summ[:, 1, [1, 3]]).all()
    assert np.isnan(err[:, 1, 0, :3]).all() and (err[:, 1, :, 3] == -1).all() and (err[:, 1, 1, :3] > 0).all()
    assert (summ[:, 2, 5] == PR.FLAG_PA_JOINTS).all() and (summ[:, 2, 4] == 2).all() and np.isnan(summ[:, 2, 1]).all()
    assert np.isnan(err[:, 2, 1, 2:4]).all() and (err[:, 2, 0, 2:4] > 0).all() and np.isnan(xf[:, 2, 0]).all() and np.isfinite(xf[:, 2, 1]).all()
    # a NaN in an unscored joint is not read into anything
    pj[:, 0, 7] = np.nan
    again = run(pj, gt_j, pv, gt_v, w)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(got, again))
    # root_a == root_b: a pelvis joint
    check(run(pj, gt_j, pv, gt_v, w[:, :], roots=(1, 1)), pj, gt_j, pv, gt_v, w, what="pelvis root", roots=(1, 1))


def test_coinciding_predictions_have_no_fit():
    """var1 == 0 with three or more scored points: every predicted joint of image 1 and every predicted vertex of image 2 in one place,
    far from the origin and not representable in few bits.  The fit is undefined (flag 2 / 4, NaN), the root-aligned values are not"""
    pj, gt_j, pv, gt_v = clouds(12, 3, 3, 257)
    pj[:, 1, :] = np.float32([1000.1, -0.3, 7.7])
    pv[:, 2, :] = np.float32([-3.3, 1000.7, 0.1])
    got = run(pj, gt_j, pv, gt_v)
    check(got, pj, gt_j, pv, gt_v, what="coinciding")
    err, summ, xf = got
    assert (summ[:, 0, 5] == 0).all() and (summ[:, 1, 5] == PR.FLAG_PA_JOINTS).all() and (summ[:, 2, 5] == PR.FLAG_PA_VERTS).all()
    assert np.isnan(summ[:, 1, 1]).all() and np.isnan(err[:, 1, 1, :J]).all() and np.isnan(xf[:, 1, 0]).all()
    assert np.isfinite(summ[:, 1, [0, 2, 3]]).all() and (err[:, 1, 0, :J] > 0).all() and np.isfinite(xf[:, 1, 1]).all()
    assert np.isnan(summ[:, 2, 3]).all() and np.isnan(xf[:, 2, 1]).all() and np.isfinite(summ[:, 2, :3]).all() and np.isfinite(xf[:, 2, 0]).all()
    # the ground truth in one place is a defined fit: scale 0, every point lands on the ground truth's mean
    gt_j2 = gt_j.copy()
    gt_j2[0, :] = np.float32([0.3, 0.2, 0.1])
    pj, _, pv, gt_v = clouds(12, 3, 3, 257)
    got = run(pj, gt_j2, pv, gt_v)
    check(got, pj, gt_j2, pv, gt_v, what="coinciding ground truth", xform=False)
    assert (got[1][:, 0, 5] == 0).all() and (got[1][:, 0, 1] == 0).all() and (got[2][:, 0, 0, 0] == 0).all()


def grid(a, step=2.0 ** -13):
    """onto a grid that float32 still holds exactly 1000 m from the origin"""
    return (np.round(a.astype(np.float64) / step) * step).astype(np.float32)


def test_clouds_1000_m_from_the_origin_score_the_same():
    pj, gt_j, pv, gt_v = [grid(a) for a in clouds(6, 3, 3, 6890)]
    near = run(pj, gt_j, pv, gt_v)
    shift = np.float32([1000, -1000, 1000])
    far = [a + shift for a in (pj, gt_j, pv, gt_v)]
    assert all(np.array_equal(f.astype(np.float64) - shift, a.astype(np.float64)) for f, a in zip(far, (pj, gt_j, pv, gt_v)))  # exact shifts
    got = run(*far)
    check(got, *far, what="1000 m", xform=False)  # t is then of the order of 1000 m: compared below
    for i in range(3):
        rj, rv = radius(gt_j[i, :J]), radius(gt_v[i])
        within(got[0][:, i], near[0][:, i], rj, "1000 m against unshifted: joint_err")
        within(got[1][:, i, :2], near[1][:, i, :2], rj, "1000 m against unshifted: mpjpe")
        within(got[1][:, i, 2:4], near[1][:, i, 2:4], rv, "1000 m against unshifted: pve")
        within(got[2][:, i, 0, :10], near[2][:, i, 0, :10], rj, "1000 m against unshifted: joint scale, R")
        within(got[2][:, i, 1, :10], near[2][:, i, 1, :10], rv, "1000 m against unshifted: vertex scale, R")
    (_, _, xf), _ = ref(*far)
    assert np.abs(got[2][..., 10:] - xf[..., 10:]).max() <= 1e-6 * 2000  # |ref| of a translation is the distance it bridges


def test_millimetre_magnitudes_score_to_the_same_relative_accuracy():
    pj, gt_j, pv, gt_v = [a * np.float32(1e-3) for a in clouds(7, 1, 3, 257)]
    got = run(pj, gt_j, pv, gt_v)
    check(got, pj, gt_j, pv, gt_v, what="x 1e-3")
    assert radius(gt_v[0]) < 1e-3 and (got[1][..., :4] < 1e-3).all()


def test_a_nan_coordinate_stays_in_its_image():
    pj, gt_j, pv, gt_v = clouds(8, 3, 3, 257)
    clean = run(pj, gt_j, pv, gt_v)
    pv[1, 1, 100, 2] = np.nan   # stage 1, image 1: a vertex
    pj[2, 2, 5, 0] = np.nan     # stage 2, image 2: a scored joint
    got = run(pj, gt_j, pv, gt_v)
    for s in range(3):
        for i in range(3):
            if (s, i) == (1, 1):
                assert np.isnan(got[1][s, i, 2:4]).all() and np.isnan(got[2][s, i, 1]).all()
                assert np.array_equal(got[0][s, i], clean[0][s, i]) and np.array_equal(got[1][s, i, :2], clean[1][s, i, :2])
            elif (s, i) == (2, 2):
                assert np.isnan(got[1][s, i, :2]).all() and np.isnan(got[0][s, i, 1, :J]).all() and np.isnan(got[0][s, i, 0, 5])
                assert np.array_equal(got[1][s, i, 3], clean[1][s, i, 3])  # the vertex fit does not read the joints
            else:
                assert all(np.array_equal(g[s, i], c[s, i]) for g, c in zip(got, clean)), (s, i)


def test_outputs_keep_64_guard_floats_on_either_side():
    n, B, P, G = 3, 3, 70, 64
    pj, gt_j, pv, gt_v = clouds(9, n, B, P)
    want = run(pj, gt_j, pv, gt_v, num_joints=K)
    lib = hpe_amd._lib.load()
    jd, vd, gj, gv = [dev(x) for x in pj], [dev(x) for x in pv], dev(gt_j), dev(gt_v)
    sizes = (n * B * 2 * K, n * B * 6, n * B * 26)
    bufs = [torch.full((s + 2 * G,), -12345.0, device="cuda") for s in sizes]
    jp, vp = (C.c_void_p * n)(*[t.data_ptr() for t in jd]), (C.c_void_p * n)(*[t.data_ptr() for t in vd])
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    hpe_amd._lib.check(lib.hpe_pose3d_scores(jp, gj.data_ptr(), None, vp, gv.data_ptr(), n, B, K, P, 2, 3, *[b.data_ptr() + 4 * G for b in bufs], st))
    torch.cuda.synchronize()
    for b, s, w in zip(bufs, sizes, want):
        h = b.cpu().numpy()
        assert (h[:G] == -12345.0).all() and (h[G + s:] == -12345.0).all()
        assert np.array_equal(h[G:G + s].view(np.int32), w.reshape(-1).view(np.int32))
    # each output alone writes what it wrote together with the others
    for k in range(3):
        outs = [None, None, None]
        outs[k] = torch.full((sizes[k],), -1.0, device="cuda")
        hpe_amd._lib.check(lib.hpe_pose3d_scores(jp, gj.data_ptr(), None, vp, gv.data_ptr(), n, B, K, P, 2, 3,
                                                 *[None if o is None else o.data_ptr() for o in outs], st))
        torch.cuda.synchronize()
        assert np.array_equal(outs[k].cpu().numpy().view(np.int32), want[k].reshape(-1).view(np.int32))


def bits(out):
    return [t.cpu().numpy().view(np.int32).copy() for t in out]


def test_same_bits_again_and_from_a_replayed_graph():
    pj, gt_j, pv, gt_v = clouds(10, 3, 3, 6890)
    args = ([dev(x) for x in pj], dev(gt_j), [dev(x) for x in pv], dev(gt_v))
    first = bits(metrics.pose3d_scores(*args))
    again = bits(metrics.pose3d_scores(*args))
    assert all(np.array_equal(x, y) for x, y in zip(first, again))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = metrics.pose3d_scores(*args)
    for _ in range(2):
        for t in out:
            t.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        assert all(np.array_equal(x, y) for x, y in zip(first, bits(out)))


def test_joints_only_and_procrustes_align_equal_the_full_call():
    pj, gt_j, pv, gt_v = clouds(11, 3, 3, 257)
    full = run(pj, gt_j, pv, gt_v)
    alone = run(pj, gt_j)
    assert np.array_equal(alone[0], full[0]) and np.array_equal(alone[1][..., :2], full[1][..., :2]) and np.array_equal(alone[2][:, :, 0], full[2][:, :, 0])
    assert np.isnan(alone[1][..., 2:4]).all() and (alone[1][..., 5] == PR.FLAG_NO_VERTS).all() and np.isnan(alone[2][:, :, 1]).all()
    check(alone, pj, gt_j, what="joints only")
    # the vertex fit of the full call is procrustes_align of the vertex clouds; the joint fit is the weighted one
    aligned, scale, R, t = metrics.procrustes_align(dev(pv[1]), dev(gt_v))
    torch.cuda.synchronize()
    got = torch.cat([scale[:, None], R.reshape(-1, 9), t], 1).cpu().numpy()
    assert np.array_equal(got, full[2][1, :, 1])
    w = np.zeros((3, K), np.float32)
    w[:, :J] = 1
    a1, s1, R1, t1 = metrics.procrustes_align(dev(pj[2, 0]), dev(gt_j[0]), dev(w[0]))  # [N,3]: no batch axis
    torch.cuda.synchronize()
    assert a1.shape == (K, 3) and s1.dim() == 0 and R1.shape == (3, 3) and t1.shape == (3,)
    assert np.array_equal(torch.cat([s1[None], R1.reshape(-1), t1]).cpu().numpy(), full[2][2, 0, 0])
    res = np.linalg.norm(a1.cpu().numpy().astype(np.float64) - gt_j[0], axis=1)[:J]
    assert np.abs(res - full[0][2, 0, 1, :J]).max() <= 1e-5  # aligned is float32 arithmetic on the float32 fit: a looser statement on purpose
    assert np.abs(aligned.cpu().numpy() - (scale.cpu().numpy()[:, None, None] * pv[1] @ R.cpu().numpy().transpose(0, 2, 1) + t.cpu().numpy()[:, None])).max() < 1e-5


# ---------------------------------------------------------------------------------------------- end to end, on the small trainer
@pytest.fixture(scope="module")
def trainer3d(weights, data, tmp_path_factory):  # noqa: F811
    tr = make_trainer(weights, data, tmp_path_factory.mktemp("ckpt3d"))
    batches = [tr._load_images(b, augment=False)[0] for b in tr.dataset]
    assert len(batches) == 2
    yield tr, batches
    tr.engine.close()


def test_score_step_3d_against_the_predictors_own_theta(trainer3d):
    tr, batches = trainer3d
    images = batches[0]
    stages = tr.engine.forward(images, all_stages=True, want=("theta", "verts", "joints"))
    theta = stages[-1]["theta"].clone()
    err, summ, xf = [t.cpu().numpy() for t in tr.predictor.score_step_3d(images, theta_gt=theta)]
    assert err.shape == (3, 2, 2, K) and summ.shape == (3, 2, 6) and xf.shape == (3, 2, 2, 13)
    assert (summ[..., 5] == 0).all() and (summ[..., 4] == J).all() and (err[..., J:] == -1).all()
    gt_v, gt_j = stages[-1]["verts"].cpu().numpy(), stages[-1]["joints"].cpu().numpy()
    for i in range(2):
        rj, rv = radius(gt_j[i, :J]), radius(gt_v[i])
        print("pose3d own theta, image %d: last-stage mpjpe %.3g pa %.3g pve %.3g pa_pve %.3g; radius %.3g / %.3g" % ((i,) + tuple(summ[-1, i, :4]) + (rj, rv)))
        assert (summ[-1, i, :2] <= BAR * rj).all() and (summ[-1, i, 2:4] <= BAR * rv).all() and (err[-1, i, :, :J] <= BAR * rj).all()
        for s in range(2):  # an earlier stage's theta differs: strictly positive
            assert not torch.equal(stages[s]["theta"][i], theta[i])
            assert (summ[s, i, :4] > 0).all()
    last = [t.cpu().numpy() for t in tr.predictor.score_step_3d(images, theta_gt=theta, all_stages=False)]
    assert np.array_equal(last[1], summ[-1:]) and np.array_equal(last[0], err[-1:])
    # the same ground truth given as joints and vertices
    again = [t.cpu().numpy() for t in tr.predictor.score_step_3d(images, joints3d_gt=stages[-1]["joints"], verts_gt=stages[-1]["verts"])]
    assert all(np.allclose(a, b, rtol=0, atol=1e-6, equal_nan=True) for a, b in zip(again, (err, summ, xf)))
    only14 = [t.cpu().numpy() for t in tr.predictor.score_step_3d(images, joints3d_gt=stages[-1]["joints"][:, :J].contiguous())]
    assert np.allclose(only14[0], err, rtol=0, atol=1e-6) and (only14[1][..., 5] == PR.FLAG_NO_VERTS).all()
    with pytest.raises(ValueError, match="theta_gt or joints3d_gt"):
        tr.predictor.score_step_3d(images)


def axis_angle_compose(delta, aa):
    """the axis-angle of R(delta) R(aa), in float64"""
    def to_R(v):
        a = np.linalg.norm(v)
        return np.eye(3) if a == 0 else rotation(v / a, a)

    R = to_R(np.asarray(delta, np.float64)) @ to_R(np.asarray(aa, np.float64))
    ang = np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))
    ax = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return ax / np.linalg.norm(ax) * ang


def test_a_changed_root_rotation_moves_mpjpe_and_leaves_the_pa_scores(trainer3d):
    tr, batches = trainer3d
    images = batches[1]
    theta = tr.engine.forward(images, all_stages=True, want=("theta",))[-1]["theta"].clone()
    base = [t.cpu().numpy() for t in tr.predictor.score_step_3d(images, theta_gt=theta)]
    turned = theta.cpu().numpy().copy()
    for i in range(2):
        turned[i, 3:6] = axis_angle_compose([0.0, 0.5, 0.0], turned[i, 3:6])  # the whole body turns by 0.5 rad about the pelvis
    gt = tr.engine.smpl(torch.from_numpy(turned).cuda(), want=("verts", "joints"))
    got = [t.cpu().numpy() for t in tr.predictor.score_step_3d(images, theta_gt=torch.from_numpy(turned).cuda())]
    gt_v, gt_j = gt["verts"].cpu().numpy(), gt["joints"].cpu().numpy()
    for i in range(2):
        rj, rv = radius(gt_j[i, :J]), radius(gt_v[i])
        print("pose3d turned root, image %d: mpjpe %s pve %s; radius %.3g / %.3g" % (i, got[1][:, i, 0], got[1][:, i, 2], rj, rv))
        assert (got[1][-1, i, [0, 2]] > 1e-3 * rj).all() and (base[1][-1, i, [0, 2]] <= BAR * rv).all()  # MPJPE and PVE see the turn
        within(got[1][:, i, 1], base[1][:, i, 1], rj, "turned root: pa_mpjpe")
        within(got[1][:, i, 3], base[1][:, i, 3], rv, "turned root: pa_pve")
        within(got[0][:, i, 1, :J], base[0][:, i, 1, :J], rj, "turned root: pa joint_err")


def test_score_checkpoint_3d_equals_scores3d_fed_by_hand(trainer3d):
    tr, batches = trainer3d
    rng = np.random.RandomState(12)
    thetas = [tr.engine.forward(b, all_stages=True, want=("theta",))[0]["theta"].clone() for b in batches]  # the first stage's: a real error
    jw = torch.from_numpy((rng.rand(2, J) > 0.2).astype(np.float32)).cuda()
    g1 = tr.engine.smpl(thetas[1], want=("verts", "joints"))
    data3d = [(batches[0], {"theta": thetas[0]}), (batches[1], {"joints3d": g1["joints"], "verts": g1["verts"], "joint_weights": jw})]
    lines = []
    tr.log = lines.append
    out = tr.score_checkpoint_3d(data3d, restore=False)
    tr.log = lambda s: None
    by_hand = metrics.Scores3D()
    by_hand.add(*tr.predictor.score_step_3d(batches[0], theta_gt=thetas[0])[:2])
    by_hand.add(*tr.predictor.score_step_3d(batches[1], joints3d_gt=g1["joints"], verts_gt=g1["verts"], joint_weights=jw)[:2])
    assert out["batches"] == 2 and out["images"] == 4 and len(out["stages"]) == 3 and len(lines) == 1
    want = by_hand.results()
    assert out["stages"] == want and {k: v for k, v in out.items() if k not in ("stages", "batches")} == want[-1]  # the same adds, the same bits
    assert out["stages"][0]["mpjpe_mm"] < 1e-3 < out["mpjpe_mm"] and out["pa_mpjpe_mm"] > 0 and out["pve_mm"] > out["pa_pve_mm"] > 0
    assert 0 <= out["auc3d"] <= out["pck3d_150"] <= 1
