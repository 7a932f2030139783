"""GPU tests of the 3-D supervision terms (run with -m gpu on an MI355X; DESIGN.md "3-D supervision"): hpe_loss3d / hpe_loss3d_backward
against the float64 restatement of tests/loss3d_ref.py under the project's bar -- max |out - ref64| <= 4 x max(max |ref32 - ref64|,
2^-22 max |ref64|) per output tensor, the float32 figures from the same functions run in float32 --, the rows that are not supervised, the
exact zero of a prediction that equals its ground truth, the mirrored labels, determinism and the data-parallel shares; then the terms
inside ``GeneratorTrainer.step`` and ``Trainer`` on the small trainer of tests/test_gpu_trainer.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import hpe_amd
from hpe_amd import synthetic

import loss3d_ref as LR
from smpl_torch_ref import SmplTorch
from test_gpu_trainer import B as TB, data, make_trainer, same, weights  # noqa: F401  (fixtures of the small trainer)

pytestmark = pytest.mark.gpu
# the package's own modules, by what it exports (``hpe_amd`` is an alias of a package whose name is no identifier: a dotted import through
# the alias elsewhere in the suite makes second copies of submodules, and the attributes of the alias may name those)
augment, records = sys.modules[hpe_amd.gt3d_real.__module__], sys.modules[hpe_amd.load_training_batch_3d.__module__]
E, ops = sys.modules[hpe_amd.HpeEngine.__module__], sys.modules[hpe_amd.joints3d_loss.__module__]
GT_KEYS = ("joints_gt", "Rs_gt", "shape_gt", "w_joints", "w_smpl", "flip")
WORST = {"ratio": 0.0}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def gt_of(c):
    return hpe_amd.Gt3D(dev(c["joints_gt"]), dev(c["Rs_gt"]), dev(c["shape_gt"]), dev(c["w_joints"]), dev(c["w_smpl"]),
                        None if c["flip"] is None else dev(c["flip"]))


def stages_of(seed, B, n, K):
    """n stages of predictions against one ground truth -> (list of per-stage cases, the ground truth's arrays)"""
    cases = [LR.random_case(seed + 17 * s, B, K) for s in range(n)]
    gt = {k: cases[0][k] for k in GT_KEYS}
    return [dict(c, **gt) for c in cases], gt


def within(got, ref32, ref64, what):
    err, allowed = LR.bar(got, ref32, ref64, what)
    if allowed > 0:
        WORST["ratio"] = max(WORST["ratio"], err / allowed)
    assert err <= allowed, (what, err, allowed)


def run_gpu(cases, gt, scale_j=None, scale_s=None, betas=None, want=("joints", "betas", "Rs")):
    """-> (parts [n,5], per_image [n,B,3], gradient dict of per-stage lists) as numpy"""
    j, R = [dev(c["joints"]) for c in cases], [dev(c["Rs"]) for c in cases]
    b = [dev(c["betas"]) for c in cases] if betas is None else betas
    parts, per = E.loss3d_parts(j, b, R, gt, want_per_image=True)
    n = len(cases)
    sj = dev(np.ones(n, np.float32) if scale_j is None else scale_j)
    ss = dev(np.ones(n, np.float32) if scale_s is None else scale_s)
    g = E.loss3d_backward(j, b, R, gt, sj, ss, want=want)
    return parts.cpu().numpy(), per.cpu().numpy(), {k: [t.cpu().numpy() for t in v] for k, v in g.items()}


def check_against_reference(cases, got, scale_j, scale_s, what):
    parts, per, grads = got
    for s, c in enumerate(cases):
        r64 = LR.run(**c, scale_j=scale_j[s], scale_s=scale_s[s])
        r32 = LR.run(**c, scale_j=scale_j[s], scale_s=scale_s[s], dtype=torch.float32)
        assert np.array_equal(parts[s, 3:], r64["parts"][3:]), (what, s, parts[s])  # the counts are exact
        for i, name in enumerate(("num_j", "num_pose", "num_shape")):
            within(parts[s, i], r32["parts"][i], r64["parts"][i], "%s stage %d %s" % (what, s, name))
        within(per[s], r32["per_image"], r64["per_image"], "%s stage %d per_image" % (what, s))
        for k, key in (("joints", "grad_joints"), ("Rs", "grad_Rs"), ("betas", "grad_betas")):
            if k in grads:
                within(grads[k][s], r32[key], r64[key], "%s stage %d %s" % (what, s, key))


def mixed_weights(gt, B):
    """row 0 has joints only, row 1 the SMPL parameters only; the others keep their random weights"""
    if B >= 3:
        gt["w_joints"][:2], gt["w_smpl"][:2] = (1.0, 0.0), (0.0, 1.0)


# ---------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("B,n,K,in_theta", [(1, 1, 19, False), (3, 3, 19, False), (5, 3, 19, True), (5, 1, 14, False), (3, 1, 24, False)])
def test_parity_with_the_float64_reference(B, n, K, in_theta):
    cases, gt = stages_of(100 + B + n, B, n, K)
    mixed_weights(gt, B)
    g = np.random.RandomState(B)
    scale_j, scale_s = (g.rand(n) + 0.1).astype(np.float32), (g.rand(n) * 0.01 + 1e-3).astype(np.float32)
    betas = None
    if in_theta:  # theta + 75 with stride 85, read in place
        thetas = [dev(g.randn(B, 85).astype(np.float32)) for _ in range(n)]
        betas = [t[:, 75:] for t in thetas]
        for c, t in zip(cases, thetas):
            c["betas"] = t[:, 75:].cpu().numpy()
        assert betas[0].stride(0) == 85 and not betas[0].is_contiguous()
    got = run_gpu(cases, gt_of(gt), scale_j, scale_s, betas=betas)
    assert got[0].shape == (n, 5) and got[1].shape == (n, B, 3) and got[2]["joints"][0].shape == (B, K, 3)
    assert all((gj[:, 14:] == 0).all() for gj in got[2]["joints"])
    check_against_reference(cases, got, scale_j, scale_s, "B=%d n=%d K=%d" % (B, n, K))
    if in_theta:  # the ABI itself with the pointer into theta, against the engine's call
        lib, st = hpe_amd._lib.load(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
        G = gt_of(gt)
        j, R = [dev(c["joints"]) for c in cases], [dev(c["Rs"]) for c in cases]
        arr = lambda ts, off=0: (C.c_void_p * n)(*[t.data_ptr() + off for t in ts])  # noqa: E731
        parts, fl = torch.empty((n, 5), device="cuda"), G.flip.to(torch.uint8)
        hpe_amd._lib.check(lib.hpe_loss3d(arr(j), arr(R), arr(thetas, 75 * 4), 85, G.joints.data_ptr(), G.Rs.data_ptr(), G.shape.data_ptr(),
                                          G.w_joints.data_ptr(), G.w_smpl.data_ptr(), fl.data_ptr(), n, B, K,
                                          parts.data_ptr(), None, st))
        assert np.array_equal(parts.cpu().numpy(), got[0])
    print("loss3d: worst ratio to the bar so far %.3g" % WORST["ratio"])


def test_the_hip_term_is_there():
    """the gradient of a hip joint carries the derivative of the alignment: without it the error would be of the gradient's own size"""
    cases, gt = stages_of(7, 2, 1, 19)
    got = run_gpu(cases, gt_of(gt))
    r64 = LR.run(**cases[0])
    hips = np.abs(got[2]["joints"][0][:, 2:4] - r64["grad_joints"][:, 2:4]).max()
    others = np.abs(r64["grad_joints"][:, :14]).max()
    assert hips <= 1e-5 * others


# ---------------------------------------------------------------------------------------------- rows that are not supervised
def bits(got):
    parts, per, grads = got
    return [parts.view(np.int32), per.view(np.int32)] + [a.view(np.int32) for k in sorted(grads) for a in grads[k]]


def test_all_weights_zero():
    cases, gt = stages_of(11, 3, 2, 19)
    gt["w_joints"][:], gt["w_smpl"][:] = 0, 0
    for k in ("joints_gt", "Rs_gt", "shape_gt"):
        gt[k][:] = np.nan
    parts, per, grads = run_gpu(cases, gt_of(gt))
    assert (parts == 0).all() and (per == 0).all()
    assert all((a.view(np.int32) == 0).all() for v in grads.values() for a in v)  # exact zeros, not -0 and not NaN
    lj, ls = ops.loss3d(dev(cases[0]["joints"]), dev(cases[0]["betas"]), dev(cases[0]["Rs"]), gt_of(gt))
    assert float(lj) == 0.0 and float(ls) == 0.0
    assert (ops.loss3d_counts(gt_of(gt)).cpu().numpy() == 0).all()


def test_nan_labels_of_unsupervised_rows_reach_nothing():
    cases, gt = stages_of(12, 5, 2, 19)
    mixed_weights(gt, 5)
    gt["w_joints"][3], gt["w_smpl"][3] = 0.0, 0.0
    clean = {k: v.copy() for k, v in gt.items()}
    clean["joints_gt"][[1, 3]], clean["Rs_gt"][[0, 3]], clean["shape_gt"][[0, 3]] = 0, 0, 0
    dirty = {k: v.copy() for k, v in gt.items()}
    dirty["joints_gt"][[1, 3]], dirty["Rs_gt"][[0, 3]], dirty["shape_gt"][[0, 3]] = np.nan, np.nan, np.inf
    a, b = run_gpu(cases, gt_of(clean)), run_gpu(cases, gt_of(dirty))
    assert all(np.isfinite(x.view(np.float32)).all() for x in bits(b))
    assert all(np.array_equal(x, y) for x, y in zip(bits(a), bits(b)))
    assert a[0][0, 3] == 42 * 3 and a[0][0, 4] == 226 * 3
    assert (a[2]["joints"][0][[1, 3]] == 0).all() and (a[2]["Rs"][0][[0, 3]] == 0).all() and (a[2]["betas"][0][[0, 3]] == 0).all()
    assert (a[2]["joints"][0][0] != 0).any() and (a[2]["Rs"][0][1] != 0).any()


# ---------------------------------------------------------------------------------------------- predictions made by engine.smpl
@pytest.fixture(scope="module")
def model():
    return synthetic.make_smpl_model()


@pytest.fixture(scope="module")
def smpl_engine(model):
    e = hpe_amd.HpeEngine(device=0, max_batch=4)
    e.load_smpl(model)
    e.finalize()
    yield e
    e.close()


def test_a_prediction_equal_to_its_ground_truth_is_exactly_zero(smpl_engine):
    th = synthetic.make_thetas(3, seed=21).astype(np.float32)
    gt = augment.gt3d_real(smpl_engine, {"pose": th[:, 3:75], "shape": th[:, 75:]})
    assert gt.w_joints.tolist() == [1, 1, 1] and gt.w_smpl.tolist() == [1, 1, 1] and gt.flip is None
    theta = dev(th)
    o = smpl_engine.smpl(theta, want=("joints", "Rs"))
    parts, per = E.loss3d_parts(o["joints"], theta[:, 75:], o["Rs"], gt, want_per_image=True)
    parts, per = parts.cpu().numpy(), per.cpu().numpy()
    assert parts[0, 1] == 0.0 and parts[0, 2] == 0.0 and (per[0, :, 1:] == 0.0).all()  # no Rodrigues in the kernel: exact
    assert parts[0, 0] == 0.0  # the joints of the same call too
    assert parts[0, 3] == 126 and parts[0, 4] == 678


def test_mirrored_predictions_against_flipped_labels(smpl_engine, model):
    """every row flipped, the prediction engine.smpl of reflect_pose of the ground truth: the rotation term is small, not exactly zero
    (Rodrigues of the reflected vector rounds differently), and the joint term is NOT small -- the synthetic body is not symmetric --,
    so both are compared with the reference"""
    th = synthetic.make_thetas(3, seed=22).astype(np.float32)
    gt = augment.gt3d_real(smpl_engine, {"pose": th[:, 3:75], "shape": th[:, 75:]}, flip=np.ones(3, bool))
    mirrored = th.copy()
    mirrored[:, 3:75] = augment.reflect_pose(th[:, 3:75])
    theta = dev(mirrored)
    o = smpl_engine.smpl(theta, want=("joints", "Rs"))
    case = dict(joints=o["joints"].cpu().numpy(), betas=mirrored[:, 75:], Rs=o["Rs"].cpu().numpy(), joints_gt=gt.joints.cpu().numpy(),
                Rs_gt=gt.Rs.cpu().numpy(), shape_gt=gt.shape.cpu().numpy(), w_joints=np.ones(3, np.float32), w_smpl=np.ones(3, np.float32),
                flip=np.ones(3, bool))
    got = run_gpu([case], gt)
    check_against_reference([case], got, [1.0], [1.0], "mirrored")
    num_pose = got[0][0, 1]
    unflipped = E.loss3d_parts(o["joints"], theta[:, 75:], o["Rs"], hpe_amd.Gt3D(*gt[:5], None))[0, 1].item()
    print("loss3d mirrored: num_pose %.3g with the flip, %.3g without; num_j %.3g" % (num_pose, unflipped, got[0][0, 0]))
    assert got[0][0, 2] == 0.0 and num_pose <= 1e-6 * unflipped  # the shape is the same; the rotations match only through the flip


# ---------------------------------------------------------------------------------------------- determinism and shares
def test_same_bits_again_and_row_gradients_do_not_depend_on_the_batch():
    cases, gt = stages_of(31, 5, 2, 19)
    mixed_weights(gt, 5)
    sj, ss = np.float32([0.3, 0.7]), np.float32([0.01, 0.02])
    a, b = run_gpu(cases, gt_of(gt), sj, ss), run_gpu(cases, gt_of(gt), sj, ss)
    assert all(np.array_equal(x, y) for x, y in zip(bits(a), bits(b)))
    for i in range(5):
        row = [{k: (v[i:i + 1] if v is not None else None) for k, v in c.items()} for c in cases]
        one = run_gpu(row, gt_of({k: row[0][k] for k in GT_KEYS}), sj, ss)
        for k in ("joints", "Rs", "betas"):
            for s in range(2):
                assert np.array_equal(one[2][k][s].view(np.int32), a[2][k][s][i:i + 1].view(np.int32)), (i, k, s)
        assert np.array_equal(one[1].view(np.int32), a[1][:, i:i + 1].view(np.int32))


def test_a_replayed_graph_gives_the_eager_bits():
    cases, gt = stages_of(32, 3, 2, 19)
    G = gt_of(gt)
    j, b, R = ([dev(c[k]) for c in cases] for k in ("joints", "betas", "Rs"))
    scale = dev(np.float32([0.3, 0.7]))

    def both():
        parts, per = E.loss3d_parts(j, b, R, G, want_per_image=True)
        g = E.loss3d_backward(j, b, R, G, scale, scale)
        return [parts, per] + [t for k in sorted(g) for t in g[k]]

    eager = [t.cpu().numpy().view(np.int32).copy() for t in both()]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = both()
    for t in out:
        t.fill_(-7)
    graph.replay()
    torch.cuda.synchronize()
    assert all(np.array_equal(x, t.cpu().numpy().view(np.int32)) for x, t in zip(eager, out))


def test_shares_of_a_split_batch():
    cases, gt = stages_of(41, 4, 1, 19)
    gt["w_joints"][1], gt["w_smpl"][2] = 0.0, 0.0
    c = cases[0]
    whole_gt = gt_of(gt)
    counts = ops.loss3d_counts(whole_gt)
    assert counts.cpu().tolist() == [42.0 * 3, 226.0 * 3]

    def losses(lo, hi, counts):
        j, b, R = (dev(c[k][lo:hi]).requires_grad_(True) for k in ("joints", "betas", "Rs"))
        lj, ls = ops.loss3d(j, b, R, whole_gt.rows(lo, hi), counts)
        (1.5 * lj + 0.25 * ls).backward()
        return lj.detach().cpu().numpy(), ls.detach().cpu().numpy(), [t.grad.cpu().numpy() for t in (j, b, R)]

    whole = losses(0, 4, None)
    halves = [losses(0, 2, counts), losses(2, 4, counts)]
    r64, r32 = LR.run(**c), LR.run(**c, dtype=torch.float32)
    for i, name in enumerate(("joints3d_loss", "smpl_param_loss")):
        l64, l32 = (float(LR.losses_of(torch.from_numpy(r["parts"]))[i]) for r in (r64, r32))
        within(whole[i], l32, l64, "whole-batch " + name)
        within(np.float64(halves[0][i]) + np.float64(halves[1][i]), l32, l64, "sum of the shares, " + name)
    for k in range(3):
        assert np.array_equal(np.concatenate([halves[0][2][k], halves[1][2][k]]).view(np.int32), whole[2][k].view(np.int32))
    # the public single-term functions are the two halves of the same launch
    assert ops.joints3d_loss(dev(c["joints"]), whole_gt).item() == whole[0] and ops.smpl_param_loss(dev(c["betas"]), dev(c["Rs"]), whole_gt).item() == whole[1]


def test_needs_input_grad_is_honoured():
    cases, gt = stages_of(51, 2, 1, 19)
    c, G = cases[0], gt_of(gt)
    j, R = dev(c["joints"]).requires_grad_(True), dev(c["Rs"])
    lj, ls = ops.loss3d(j, dev(c["betas"]), R, G)
    (lj + ls).backward()
    assert j.grad is not None and R.grad is None
    r64 = LR.run(**c, scale_j=0.5 / 84.0, scale_s=0.0)
    assert np.abs(j.grad.cpu().numpy() - r64["grad_joints"]).max() <= 1e-6 * np.abs(r64["grad_joints"]).max()


def test_argument_errors_launch_nothing():
    cases, gt = stages_of(61, 2, 1, 19)
    c, G = cases[0], gt_of(gt)
    j, b, R = dev(c["joints"]), dev(c["betas"]), dev(c["Rs"])
    lib = hpe_amd._lib.load()
    one = lambda t: (C.c_void_p * 1)(t.data_ptr())  # noqa: E731
    parts = torch.full((5,), -7.0, device="cuda")
    tail = (G.joints.data_ptr(), G.Rs.data_ptr(), G.shape.data_ptr(), G.w_joints.data_ptr(), G.w_smpl.data_ptr(), None)
    for n, B, K, stride in ((0, 2, 19, 10), (1, 0, 19, 10), (1, 2, 13, 10), (1, 2, 25, 10), (1, 2, 19, 9)):
        assert lib.hpe_loss3d(one(j), one(R), one(b), stride, *tail, n, B, K, parts.data_ptr(), None, None) == 1
        assert lib.hpe_last_error().decode().startswith("hpe_loss3d:")
    out = torch.full((2, 19, 3), -7.0, device="cuda")
    assert lib.hpe_loss3d_backward(one(j), one(R), one(b), 10, *tail, 1, 2, 19, None, None, one(out), None, None, None) == 1
    assert lib.hpe_loss3d_backward(one(j), one(R), one(b), 10, *tail, 1, 2, 19, parts.data_ptr(), parts.data_ptr(), None, None, None, None) == 1
    torch.cuda.synchronize()
    assert (parts == -7.0).all() and (out == -7.0).all()
    with pytest.raises(ValueError):
        E.loss3d_parts(j, b[:1], R, G)
    with pytest.raises(ValueError):
        E.loss3d_backward(j, b, R, G, None, None, want=("joints",))


# ---------------------------------------------------------------------------------------------- through SMPL, against the float64 chain
def test_theta_gradient_through_smpl_matches_the_float64_chain(smpl_engine, model):
    th_gt = synthetic.make_thetas(2, seed=23).astype(np.float32)
    flip = np.array([True, False])
    gt = augment.gt3d_real(smpl_engine, {"pose": th_gt[:, 3:75], "shape": th_gt[:, 75:]}, flip=flip)
    th = synthetic.make_thetas(2, seed=24).astype(np.float32)
    theta = dev(th).requires_grad_(True)
    o = smpl_engine.smpl(theta, want=("joints", "Rs"))
    lj, ls = ops.loss3d(o["joints"], theta[:, 75:], o["Rs"], gt)
    (lj + ls).backward()
    arrays = dict(joints_gt=gt.joints.cpu().numpy(), Rs_gt=gt.Rs.cpu().numpy(), shape_gt=gt.shape.cpu().numpy())
    ref = {}
    for dtype in (torch.float64, torch.float32):
        t = torch.from_numpy(th).to(dtype).requires_grad_(True)
        out = SmplTorch(model, dtype)(t)
        gj, gR, gs = (torch.from_numpy(arrays[k]).to(dtype) for k in ("joints_gt", "Rs_gt", "shape_gt"))
        w = torch.ones(2, dtype=dtype)
        per = LR.per_row(out["joints"], t[:, 75:], out["Rs"], gj, gR, gs, w, w, flip)
        l_j, l_s = LR.losses_of(LR.parts_of(per, w, w))
        (l_j + l_s).backward()
        ref[dtype] = (float(l_j.detach()), float(l_s.detach()), t.grad.to(torch.float64).numpy())
    within(lj.item(), ref[torch.float32][0], ref[torch.float64][0], "through SMPL: joints3d_loss")
    within(ls.item(), ref[torch.float32][1], ref[torch.float64][1], "through SMPL: smpl_param_loss")
    within(theta.grad.cpu().numpy(), ref[torch.float32][2], ref[torch.float64][2], "through SMPL: theta.grad")
    assert (theta.grad[:, :3] == 0).all() and (theta.grad[:, 3:] != 0).any()


# ---------------------------------------------------------------------------------------------- end to end, on the small trainer
@pytest.fixture(scope="module")
def data3d(data, tmp_path_factory):  # noqa: F811
    """the small trainer's four image records with 3-D labels: all three fields, joints only, pose and shape only, none"""
    images, mocap = data
    recs = [records.parse_image_example(p) for p in records.read_tfrecords(images)]
    th = synthetic.make_thetas(4, seed=33).astype(np.float32)
    g = np.random.RandomState(34)
    j3 = (0.3 * g.randn(4, 14, 3)).astype(np.float32)
    labels = [dict(gt3d=j3[0], pose=th[0, 3:75], shape=th[0, 75:]), dict(gt3d=j3[1]), dict(pose=th[2, 3:75], shape=th[2, 75:]), {}]
    payloads = []
    for r, lab in zip(recs, labels):
        kp = r["kp"]
        payloads.append(records.image_example(r["image"], r["seg"], r["height"], r["width"], r["center"].tolist(), r["filename"], kp[:14, 0].tolist(),
                                              kp[:14, 1].tolist(), kp[:14, 2].astype(np.int64).tolist(), kp[14:].T.reshape(-1).tolist(), **lab))
    path = str(tmp_path_factory.mktemp("records3d") / "images3d.tfrecords")
    records.write_tfrecords(path, payloads)
    return path, mocap


@pytest.fixture(scope="module")
def trainer3d(weights, data3d, tmp_path_factory):  # noqa: F811
    d = tmp_path_factory.mktemp("loss3d")
    tr = make_trainer(weights, data3d, d / "ckpt", epoch=1, model_dir=str(d / "model"), log_img_step=0, joints3d_loss_weight=1.0,
                      smpl_loss_weight=1.0)
    batch = next(iter(tr.dataset))
    draws = augment.draw_augmentation(TB, generator=torch.Generator().manual_seed(4))
    draws["flip"][:] = torch.tensor([True, False])
    images, segs, kp, gt = records.load_training_batch_3d(batch, tr.engine, draws=draws)
    plain = records.load_training_batch(batch, draws=draws)
    assert all(same(a, b) for a, b in zip((images, segs, kp), plain))  # the first three outputs are load_training_batch's, bit for bit
    assert gt.w_joints.tolist() == [1, 1] and gt.w_smpl.tolist() == [1, 0] and gt.flip.tolist() == [True, False]
    with torch.no_grad():
        features = tr.engine.encoder(images).clone()
    out = {"trainer": tr, "images": images, "segs": segs, "features": features, "kp": kp, "gt": gt, "start": tr.engine.regressor_params().clone(), "model_dir": str(d / "model")}
    yield out
    tr.engine.close()


def generator_trainer(t, **kw):
    """a fresh GeneratorTrainer on the small trainer's engine, its regressor back at the starting weights"""
    eng = t["trainer"].engine
    eng.set_regressor_params(t["start"])
    return hpe_amd.GeneratorTrainer(eng, dropout=0.0, **kw)


def test_step_without_3d_terms_is_the_parents_step(trainer3d):
    t = trainer3d
    ends, outs = [], []
    for kw, gt in (({}, None), ({}, t["gt"]), ({"joints3d_loss_weight": 0.0, "smpl_loss_weight": 0.0}, t["gt"])):
        g = generator_trainer(t, **kw)
        outs.append(g.step(t["features"], t["kp"], drop=None, gt3d=gt))
        ends.append(g.params.detach().clone())
    assert not same(ends[0], t["start"])
    assert same(ends[0], ends[1]) and same(ends[0], ends[2])
    assert all("joints3d_losses" not in o and "smpl_param_losses" not in o for o in outs)
    assert all(same(outs[0][k][-1], o[k][-1]) for o in outs[1:] for k in ("kpr_losses", "generator_critic_losses"))
    on = generator_trainer(t, joints3d_loss_weight=1.0, smpl_loss_weight=1.0)
    on.step(t["features"], t["kp"], drop=None, gt3d=t["gt"])
    assert not same(on.params.detach(), ends[0])  # and with the weights on the step is another one


def test_step_returns_the_terms_of_every_stage_and_ten_steps_lower_them(trainer3d):
    t = trainer3d
    g = generator_trainer(t, kpr_loss_weight=0.0, critic_loss_weight=0.0, joints3d_loss_weight=1.0, smpl_loss_weight=1.0)
    first = last = None
    for i in range(10):
        r = g.step(t["features"], t["kp"], use_critic=False, drop=None, gt3d=t["gt"])
        assert len(r["joints3d_losses"]) == 3 and len(r["smpl_param_losses"]) == 3
        value = torch.stack(r["joints3d_losses"] + r["smpl_param_losses"]).cpu().numpy()
        assert np.isfinite(value).all() and (value > 0).all()
        last = float(value[2]) + float(value[5])
        first = last if first is None else first
    print("loss3d ten steps: last stage joints3d + smpl_param %.6g -> %.6g" % (first, last))
    assert last < first
    # the logged terms are the functions' values on the stage's own outputs
    th = r["thetas"][-1]
    o = t["trainer"].engine.smpl(th, want=("joints", "Rs"))
    assert ops.joints3d_loss(o["joints"], t["gt"]).item() == r["joints3d_losses"][-1].item()
    only_j = generator_trainer(t, joints3d_loss_weight=2.0)
    r = only_j.step(t["features"], t["kp"], drop=None, gt3d=t["gt"])
    assert len(r["joints3d_losses"]) == 3 and r["smpl_param_losses"] == []


class WorldOfOne(object):
    """a reducer whose sums are those of one rank: records what would cross the ranks"""

    def __init__(self):
        self.blocks, self.grads = [], 0

    def sum_block(self, block):
        self.blocks.append(int(block.numel()))
        return block

    def sum_grad(self, grad):
        self.grads += 1
        return grad


def test_with_a_reducer_the_counts_share_the_keypoint_counts_collective(trainer3d):
    t = trainer3d
    kw = dict(joints3d_loss_weight=1.0, smpl_loss_weight=1.0)
    alone = generator_trainer(t, **kw).step(t["features"], t["kp"], drop=None, gt3d=t["gt"])
    red = WorldOfOne()
    g = generator_trainer(t, reducer=red, global_batch=TB, **kw)
    shared = g.step(t["features"], t["kp"], drop=None, gt3d=t["gt"])
    assert red.blocks == [3, 12] and red.grads == 1  # (kp count, cnt_j, cnt_s) before the forward; 4 terms x 3 stages at the end
    for k in ("joints3d_losses", "smpl_param_losses"):  # the global counts of a world of one are the local ones: the same bits
        assert all(same(a, b) for a, b in zip(alone[k], shared[k])), k
    red = WorldOfOne()
    generator_trainer(t, reducer=red, global_batch=TB).step(t["features"], t["kp"], drop=None, gt3d=t["gt"])
    assert red.blocks == [1, 6]  # both weights 0: the collectives the step had


def test_val_step_carries_the_terms(trainer3d):
    t, tr = trainer3d, trainer3d["trainer"]
    r = tr.val_step(t["images"], t["segs"], t["kp"], gt3d=t["gt"])
    o = tr.engine.forward(t["images"], all_stages=False, want=("joints", "theta", "Rs"))[0]
    assert len(r["joints3d_losses"]) == 1 and len(r["smpl_param_losses"]) == 1
    for got, want in ((r["joints3d_losses"][0], ops.joints3d_loss(o["joints"], t["gt"])),
                      (r["smpl_param_losses"][0], ops.smpl_param_loss(o["theta"][:, 75:], o["Rs"], t["gt"]))):
        assert np.isfinite(got.item()) and got.item() > 0 and abs(got.item() - want.item()) <= 2.0 ** -22 * want.item()
    assert "joints3d_losses" not in tr.val_step(t["images"], t["segs"], t["kp"])


def test_trainer_runs_an_epoch_and_writes_the_two_scalars(trainer3d):
    tr = trainer3d["trainer"]
    tr.engine.set_regressor_params(tr.generator.params.detach())  # the tests above stepped the engine's regressor on their own
    lines = []
    tr.log = lines.append
    out = tr.train(save_every=100)
    tr.log = lambda s: None
    assert out["steps"] == 2 and out["epochs"] == 1
    folder = os.path.join(trainer3d["model_dir"], "training")
    (name,) = os.listdir(folder)
    ev = hpe_amd.read_events(os.path.join(folder, name))
    scalars = {}
    for e in ev[1:]:
        for v in e["values"]:
            scalars.setdefault(v["tag"], []).append((e["step"], v["simple_value"]))
    for tag in ("generator/joints3d_loss", "generator/smpl_param_loss", "generator/kpr_loss"):
        assert [s for s, _ in scalars[tag]] == [1, 2] and all(np.isfinite(v) and v > 0 for _, v in scalars[tag]), (tag, sorted(scalars))
    epoch_line = [s for s in lines if s.startswith("Finished epoch")]
    assert len(epoch_line) == 1 and " j3d=" in epoch_line[0] and " smpl=" in epoch_line[0]
