"""CPU tests of the 3-D pose scores (DESIGN.md "3-D pose scores"): the float64 reference tests/pose3d_ref.py on cases with known answers,
the host build of the 3x3 solver (hpe_debug_procrustes3) against np.linalg.svd, the argument refusals of hpe_pose3d_scores (they come
before any HIP call), the arithmetic of ``metrics.Scores3D`` against loops, ``Trainer.score_checkpoint_3d`` with a stub in place of the
engine, and the optional 3-D features of an image record."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import hpe_amd
from hpe_amd import metrics, records, trainer as T

import pose3d_ref as PR
import records_writer as RW

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "records")


def rotation(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    x, y, z = axis
    S = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
    return np.eye(3) + math.sin(angle) * S + (1 - math.cos(angle)) * S @ S


# ---------------------------------------------------------------------------------------------- the reference on known answers
def test_reference_recovers_a_known_similarity_transform():
    rng = np.random.RandomState(0)
    X = rng.standard_normal((14, 3))
    R, scale, t = rotation([1, 2, 3], 0.7), 1.3, np.array([0.5, -2.0, 4.0])
    Y = scale * X @ R.T + t
    got_s, got_R, got_t, _mu1, _mu2 = PR.similarity(X, Y)
    assert abs(got_s - scale) < 1e-12 and np.abs(got_R - R).max() < 1e-12 and np.abs(got_t - t).max() < 1e-12
    assert PR.pa_errors(X, Y, PR.similarity(X, Y)).max() < 1e-12
    w = np.ones(14)
    w[[1, 5, 6]] = 0  # the unscored points may lie anywhere
    X2 = X.copy()
    X2[[1, 5, 6]] += 100.0
    got = PR.similarity(X2, Y, w)
    assert abs(got[0] - scale) < 1e-12 and np.abs(got[1] - R).max() < 1e-12


def test_reference_never_reflects_a_mirrored_cloud():
    """Y = X mirrored in z, X centred with the diagonal covariance diag(a, b, c), a >= b >= c: K = diag(a, b, -c), the best proper rotation
    is the identity, scale = (a + b - c) / (a + b + c), and the residual is closed-form"""
    X = np.array([[2, 0, 0], [-2, 0, 0], [0, 1.5, 0], [0, -1.5, 0], [0, 0, 0.5], [0, 0, -0.5]], np.float64)
    Y = X * [1, 1, -1]
    a, b, c = 8.0, 4.5, 0.5
    scale, R, t, _mu1, _mu2 = PR.similarity(X, Y)
    assert abs(np.linalg.det(R) - 1) < 1e-12 and np.abs(R - np.eye(3)).max() < 1e-12 and np.abs(t).max() < 1e-12
    assert abs(scale - (a + b - c) / (a + b + c)) < 1e-12
    want = np.linalg.norm(scale * X - Y, axis=1)
    assert np.abs(PR.pa_errors(X, Y, (scale, R, t, _mu1, _mu2)) - want).max() < 1e-12
    assert abs(want[4] - (1 + scale) * 0.5) < 1e-12 and abs(want[0] - (1 - scale) * 2) < 1e-12


def test_reference_root_aligned_error_of_one_displaced_joint():
    rng = np.random.RandomState(1)
    Y = rng.standard_normal((1, 19, 3))
    X = Y[None] + np.array([3.0, -1.0, 2.0])  # a translation of the whole body is aligned away
    X[0, 0, 7] += [0.3, 0.0, 0.4]
    err, summ, _ = PR.pose3d_scores(X, Y, weights=np.concatenate([np.ones((1, 14)), np.zeros((1, 5))], 1))
    want = np.zeros(14)
    want[7] = 0.5
    assert np.abs(err[0, 0, 0, :14] - want).max() < 1e-12 and (err[0, 0, :, 14:] == -1).all()
    assert abs(summ[0, 0, 0] - 0.5 / 14) < 1e-12 and summ[0, 0, 4] == 14 and summ[0, 0, 5] == PR.FLAG_NO_VERTS
    # a displaced hip moves the root by half of it: every other joint is then off by half the displacement
    X = Y[None].copy()
    X[0, 0, 2] += [0.0, 0.2, 0.0]
    err, _, _ = PR.pose3d_scores(X, Y)
    assert np.abs(err[0, 0, 0, [0, 1, 3, 4]] - 0.1).max() < 1e-12 and abs(err[0, 0, 0, 2] - 0.1) < 1e-12


# ---------------------------------------------------------------------------------------------- the host solver against the SVD
def solve(lib, K):
    K = np.ascontiguousarray(K, np.float64)
    R, tr = np.zeros(9), C.c_double()
    dp = C.POINTER(C.c_double)
    assert lib.hpe_debug_procrustes3(K.ctypes.data_as(dp), R.ctypes.data_as(dp), C.byref(tr)) == 0
    return R.reshape(3, 3), tr.value


def check_solver(lib, K, compare_R):
    """the bars of the issue: trace within 1e-12 |K|_F, R entries within 1e-9 where R is well determined, orthogonality and det to 1e-12"""
    R, tr = solve(lib, K)
    Rr, trr = PR.solve_rotation(K)
    assert abs(tr - trr) <= 1e-12 * np.linalg.norm(K), (K, tr, trr)
    assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(R) - 1.0) <= 1e-12, (K, R)
    if compare_R:
        assert PR.gap_ratio(K) > 1e-3, K  # the generator's promise: R is compared only where it is well conditioned
        assert np.abs(R - Rr).max() <= 1e-9, (K, R, Rr)


def test_solver_matches_svd_on_random_matrices():
    lib = hpe_amd._lib.load()
    rng = np.random.RandomState(20240607)
    compared = 0
    for _ in range(10000):
        K = rng.standard_normal((3, 3))
        well = PR.gap_ratio(K) > 1e-3
        check_solver(lib, K, well)
        compared += well
    assert compared > 9900


def test_solver_on_deficient_mirrored_scaled_and_nan_matrices():
    lib = hpe_amd._lib.load()
    rng = np.random.RandomState(3)
    for _ in range(200):
        a, b, c, d = rng.standard_normal((4, 3))
        rank2 = np.outer(a, b) + np.outer(c, d)
        check_solver(lib, rank2, PR.gap_ratio(rank2) > 1e-3)  # a coplanar cloud: R is unique
        check_solver(lib, np.outer(a, b), False)  # rank 1: many optimal rotations, one optimum
        Q = rotation(rng.standard_normal(3), rng.uniform(0, 3))
        mirrored = np.diag([1.0 + rng.rand(), 0.6 + 0.4 * rng.rand(), -0.5 * rng.rand()]) @ Q  # det < 0: the optimum gives up sigma_3
        assert np.linalg.det(mirrored) <= 0
        check_solver(lib, mirrored, PR.gap_ratio(mirrored) > 1e-3)
        K = rng.standard_normal((3, 3))
        for s in (1e-12, 1e12):
            check_solver(lib, K * s, PR.gap_ratio(K) > 1e-3)
    check_solver(lib, np.zeros((3, 3)), False)
    check_solver(lib, np.diag([1.0, 1.0, -1.0]), False)  # sigma_2 - sigma_3 = 0: a circle of optimal rotations
    R, tr = solve(lib, np.diag([2.0, 1.0, -0.5]))
    assert np.abs(R - np.eye(3)).max() < 1e-12 and abs(tr - 2.5) < 1e-12
    for pos in range(9):
        K = rng.standard_normal(9)
        K[pos] = np.nan
        R, tr = solve(lib, K.reshape(3, 3))
        assert np.isnan(R).all() and math.isnan(tr)
    assert lib.hpe_debug_procrustes3(None, None, None) == 1 and b"hpe_debug_procrustes3" in lib.hpe_last_error()


# ---------------------------------------------------------------------------------------------- argument refusals: no device is touched
def test_pose3d_scores_refuses_bad_arguments_before_any_hip_call():
    lib = hpe_amd._lib.load()
    p = C.c_void_p(0x1000)  # never dereferenced: every call below is refused first
    one = (C.c_void_p * 1)(0x1000)
    null_entry = (C.c_void_p * 1)(None)

    def call(joints=one, gt=p, w=None, verts=one, vgt=p, n=1, B=1, K=19, P=10, a=2, b=3, err=p, summ=p, xf=p):
        rc = lib.hpe_pose3d_scores(joints, gt, w, verts, vgt, n, B, K, P, a, b, err, summ, xf, None)
        return rc, lib.hpe_last_error().decode()

    cases = [(dict(joints=None), "joints"), (dict(gt=None), "joints"), (dict(joints=null_entry), r"joints_dev\[0\]"), (dict(K=0), "K 0"),
             (dict(a=-1), "roots"), (dict(b=19), "roots"), (dict(a=19), "roots"), (dict(verts=None), "together"), (dict(vgt=None), "together"),
             (dict(verts=null_entry), r"verts_dev\[0\]"), (dict(P=0), "P 0"), (dict(B=0), "batch 0"), (dict(n=0), "n_stage 0"), (dict(n=17), "n_stage 17"),
             (dict(err=None, summ=None, xf=None), "every output is NULL")]
    import re

    for kw, pattern in cases:
        rc, msg = call(**kw)
        assert rc == 1 and msg.startswith("hpe_pose3d_scores:") and re.search(pattern, msg), (kw, rc, msg)
    assert "hpe_pose3d_scores" in hpe_amd._lib.declared_symbols() and "hpe_debug_procrustes3" in hpe_amd._lib.declared_symbols()
    assert hpe_amd.pose3d_scores is metrics.pose3d_scores and hpe_amd.procrustes_align is metrics.procrustes_align
    assert hpe_amd.Scores3D is metrics.Scores3D
    with pytest.raises(TypeError, match="CUDA"):
        metrics.pose3d_scores([torch.zeros(1, 19, 3)], torch.zeros(1, 19, 3))


# ---------------------------------------------------------------------------------------------- Scores3D
def made_up_batches():
    """two batches of three stages, K = 19 with 14 scored; images with an unscored joint, an unscored hip (root undefined), two scored
    joints (PA undefined), no vertices, and an undefined vertex fit"""
    rng = np.random.RandomState(5)
    out = []
    for B in (3, 4):
        weights = np.concatenate([np.ones((B, 14)), np.zeros((B, 5))], 1)
        weights[0, 7] = 0
        flags = np.zeros(B, int)
        if B == 4:
            weights[1, 2] = 0
            flags[1] |= PR.FLAG_ROOT
            weights[2, 2:14] = 0
            flags[2] |= PR.FLAG_ROOT | PR.FLAG_PA_JOINTS
            flags[3] |= PR.FLAG_NO_VERTS
            flags[0] |= PR.FLAG_PA_VERTS
        err = rng.uniform(0, 0.3, (3, B, 2, 19))  # metres: up to 300 mm, so the 150 mm threshold cuts through
        for i in range(B):
            err[:, i][:, :, weights[i] == 0] = -1
        summ = rng.uniform(0, 0.2, (3, B, 6))
        for i in range(B):
            if flags[i] & PR.FLAG_ROOT:
                err[:, i, 0][:, weights[i] > 0] = np.nan
                summ[:, i, [0, 2]] = np.nan
            if flags[i] & PR.FLAG_PA_JOINTS:
                err[:, i, 1][:, weights[i] > 0] = np.nan
                summ[:, i, 1] = np.nan
            if flags[i] & PR.FLAG_NO_VERTS:
                summ[:, i, 2:4] = np.nan
            if flags[i] & PR.FLAG_PA_VERTS:
                summ[:, i, 3] = np.nan
        summ[:, :, 4], summ[:, :, 5] = (weights > 0).sum(1), flags
        out.append((err.astype(np.float32), summ.astype(np.float32)))
    return out


def same_result(a, b, rel=1e-12):
    assert set(a) == set(b)
    for k in a:
        x, y = (a[k], b[k]) if isinstance(a[k], list) else ([a[k]], [b[k]])
        assert len(x) == len(y)
        for p, q in zip(x, y):
            assert (math.isnan(p) and math.isnan(q)) or abs(p - q) <= rel * abs(q), (k, a[k], b[k])


KEYS = {"mpjpe_mm", "pa_mpjpe_mm", "pve_mm", "pa_pve_mm", "mpjpe_per_joint_mm", "pa_mpjpe_per_joint_mm", "pck3d_150", "auc3d", "images",
        "pa_invalid_images", "root_invalid_images"}


def test_scores3d_sums_and_ratios_match_the_loops():
    batches = made_up_batches()
    sc = metrics.Scores3D()
    for b in batches:
        assert sc.add(torch.from_numpy(b[0]), b[1]) is sc  # tensors or arrays
    want = PR.scores3d(batches)
    got = sc.results()
    assert len(got) == 3 and set(got[0]) == KEYS
    for g, w in zip(got, want):
        same_result(g, w)
    same_result(sc.result(), want[-1])
    last = got[-1]
    assert last["images"] == 7 and last["root_invalid_images"] == 2 and last["pa_invalid_images"] == 1
    assert 0 < last["pck3d_150"] < 1 and 0 < last["auc3d"] < last["pck3d_150"] and len(last["mpjpe_per_joint_mm"]) == 14
    assert sc.sums.dtype == torch.float64 and sc.sums.shape[0] == 3
    with pytest.raises(ValueError, match="stages"):
        sc.add(batches[0][0][:2], batches[0][1][:2])
    with pytest.raises(ValueError, match="nothing was added"):
        metrics.Scores3D().result()


def test_scores3d_zero_denominators_are_nan():
    err = np.full((1, 1, 2, 19), -1.0, np.float32)
    summ = np.array([[[np.nan, np.nan, np.nan, np.nan, 0, PR.FLAG_ROOT | PR.FLAG_PA_JOINTS | PR.FLAG_NO_VERTS]]], np.float32)
    r = metrics.Scores3D().add(err, summ).result()
    for k in ("mpjpe_mm", "pa_mpjpe_mm", "pve_mm", "pa_pve_mm", "pck3d_150", "auc3d"):
        assert math.isnan(r[k]), k
    assert all(math.isnan(v) for v in r["mpjpe_per_joint_mm"]) and r["images"] == 1
    # the thresholds are inclusive, and the units are the caller's
    err = np.full((1, 1, 2, 14), 0.150, np.float64)
    summ = np.array([[[0.15, 0.15, 0.1, 0.1, 14, 0]]])
    r = metrics.Scores3D().add(err, summ).result()
    assert r["pck3d_150"] == 1.0 and abs(r["auc3d"] - 1 / 31) < 1e-15 and abs(r["mpjpe_mm"] - 150) < 1e-9 and abs(r["pve_mm"] - 100) < 1e-9
    r = metrics.Scores3D(to_mm=1.0).add(err * 1000, summ).result()
    assert r["pck3d_150"] == 1.0 and abs(r["mpjpe_mm"] - 150) < 1e-9


class DoublingReducer(object):
    """a world of two ranks that hold the same shard: the sum over the ranks is twice the block"""

    def __init__(self):
        self.calls = 0

    def sum_block(self, block):
        self.calls += 1
        block *= 2
        return block


def test_scores3d_reduce_is_one_block_sum():
    batches = made_up_batches()
    one, two = metrics.Scores3D(), metrics.Scores3D()
    for b in batches:
        one.add(*b)
        two.add(*b)
    before = one.sums.clone()
    red = DoublingReducer()
    assert one.reduce(red) is one and red.calls == 1 and torch.equal(one.sums, 2 * before)
    for b in batches:  # the same as a pass that saw every batch twice
        two.add(*b)
    for g, w in zip(one.results(), two.results()):
        same_result(g, w)
    assert one.result()["images"] == 14
    with pytest.raises(ValueError, match="nothing was added"):
        metrics.Scores3D().reduce(red)


class StubPredictor3D(object):
    def __init__(self, batches):
        self.batches, self.calls, self.seen = batches, 0, []

    def score_step_3d(self, images, theta_gt=None, joints3d_gt=None, verts_gt=None, joint_weights=None, all_stages=True):
        err, summ = self.batches[self.calls]
        self.calls += 1
        self.seen.append((theta_gt is not None, joints3d_gt is not None, verts_gt is not None, joint_weights is not None))
        assert images.shape[0] == err.shape[1]
        return torch.from_numpy(err), torch.from_numpy(summ), None


def bare_trainer(**attrs):
    tr = object.__new__(T.Trainer)
    for k, v in dict(dict(rank=0, world=1, reducer=None, log=lambda s: None), **attrs).items():
        setattr(tr, k, v)
    return tr


def test_score_checkpoint_3d_sums_the_pass_without_an_engine():
    batches = made_up_batches()
    lines = []
    red = DoublingReducer()
    data = [(torch.zeros(3, 1), {"theta": torch.zeros(3, 85)}), (torch.zeros(4, 1), {"joints3d": torch.zeros(4, 14, 3), "joint_weights": torch.ones(4, 14)})]
    tr = bare_trainer(predictor=StubPredictor3D(batches), log=lines.append)
    out = tr.score_checkpoint_3d(data, restore=False)
    whole = metrics.Scores3D()
    for b in batches:
        whole.add(*b)
    assert out["batches"] == 2 and len(out["stages"]) == 3 and tr.predictor.calls == 2
    assert tr.predictor.seen == [(True, False, False, False), (False, True, False, True)]
    same_result({k: v for k, v in out.items() if k not in ("stages", "batches")}, whole.result(), rel=0.0)
    for i in range(3):
        same_result(out["stages"][i], whole.result(i), rel=0.0)
    assert len(lines) == 1 and "mpjpe=" in lines[0] and "7 images" in lines[0]
    tr = bare_trainer(predictor=StubPredictor3D(batches), reducer=red)
    assert tr.score_checkpoint_3d(data, restore=False)["images"] == 14 and red.calls == 1
    with pytest.raises(ValueError, match="no batch"):
        bare_trainer(predictor=StubPredictor3D([])).score_checkpoint_3d([], restore=False)


# ---------------------------------------------------------------------------------------------- records
def test_image_record_round_trip_with_and_without_the_3d_features():
    payloads = list(records.read_tfrecords(os.path.join(GOLDEN, "images.tfrecords")))
    r = records.parse_image_example(payloads[0])
    assert not {"gt3d", "pose", "shape", "has_3d"} & set(r)  # a record without the features parses to the keys it always had
    kp = r["kp"]
    args = (r["image"], r["seg"], r["height"], r["width"], r["center"].tolist(), r["filename"], kp[:14, 0].tolist(), kp[:14, 1].tolist(),
            kp[:14, 2].astype(np.int64).tolist())
    face = kp[14:].T.reshape(-1).tolist()
    for kw in ({}, {"face_pts": face}):
        plain = records.image_example(*args, **kw)
        assert plain == RW.image_example(*args, **kw)  # the bytes of an independent writer: nothing was added to a record without 3-D
        assert plain == records.image_example(*args, gt3d=None, pose=None, shape=None, **kw)
    rng = np.random.RandomState(2)
    gt3d, pose, shape = (rng.standard_normal(s).astype(np.float32) for s in ((14, 3), 72, 10))
    full = records.parse_image_example(records.image_example(*args, face_pts=face, gt3d=gt3d, pose=pose, shape=shape))
    assert full["gt3d"].shape == (14, 3) and np.array_equal(full["gt3d"], gt3d) and np.array_equal(full["pose"], pose)
    assert np.array_equal(full["shape"], shape) and full["has_3d"] == 1
    for k in ("image", "seg", "height", "width", "filename"):
        assert full[k] == r[k]
    assert np.array_equal(full["kp"], r["kp"]) and np.array_equal(full["center"], r["center"])
    only = records.parse_image_example(records.image_example(*args, gt3d=gt3d.reshape(-1)))
    assert np.array_equal(only["gt3d"], gt3d) and only["has_3d"] == 1 and "pose" not in only and "shape" not in only
    feats = records.parse_example(records.image_example(*args, pose=pose))
    assert list(feats)[-2:] == ["mosh/pose", "meta/has_3d"] and feats["mosh/pose"].dtype == np.float32 and feats["meta/has_3d"].tolist() == [1]
    with pytest.raises(records.RecordError, match="mosh/gt3d"):
        records.image_example(*args, gt3d=np.zeros((19, 3)))
    bad = records.serialize_example(list(records.parse_example(plain).items()) + [("mosh/shape", np.zeros(9, np.float32))])
    with pytest.raises(records.RecordError, match="mosh/shape"):
        records.parse_image_example(bad)
