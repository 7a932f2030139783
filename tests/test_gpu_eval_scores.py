"""GPU tests of hpe_eval_scores and what is built on it (run with -m gpu on an MI355X; DESIGN.md "Checkpoint scores").

The silhouette counts are integers and are compared for equality with tests/eval_ref.py run on the very float32 vertices the kernel read.
The keypoint part is compared with float64 to 4 ulp of the pixel scale (the spacing of float32 at max(H, W)): the error is a difference,
a scale by 0.5 W, two squares, a sum and a square root in float32, each within half an ulp of a value no larger than the image."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

import hpe_amd
from hpe_amd import _lib, metrics, synthetic

import eval_ref as R
from test_eval_scores_cpu import LOWER, UPPER, same_result
from test_gpu_summaries import events_of
from test_gpu_trainer import B as TRAINER_B, STAGES, data, make_config, weights  # noqa: F401  (weights, data: fixtures)

pytestmark = pytest.mark.gpu
Scores = metrics.Scores


def cuda(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def gpu_counts(verts_stages, faces, segs, trusted=False):
    """verts_stages: list of [B,P,2] float32 arrays -> int64 [n_stage,B,4]; trusted: the faces go up unchecked, as a device tensor"""
    f = cuda(faces, np.int32) if trusted else np.asarray(faces)
    counts, kp_err, norm = metrics.eval_scores([cuda(v) for v in verts_stages], f, cuda(segs), None, None)
    assert kp_err is None and norm is None and counts.dtype == torch.int32
    return counts.cpu().numpy().astype(np.int64)


def blob_masks(g, B, H, W):
    """an ellipse per image, somewhere in the frame"""
    yy, xx = np.mgrid[:H, :W]
    out = np.zeros((B, H, W), np.float32)
    for b in range(B):
        cx, cy, rx, ry = g.uniform(0.2 * W, 0.8 * W), g.uniform(0.2 * H, 0.8 * H), g.uniform(0.15 * W, 0.45 * W), g.uniform(0.15 * H, 0.45 * H)
        out[b] = (((xx - cx) / rx) ** 2 + ((yy - cy) / ry) ** 2 <= 1.0) * g.uniform(0.1, 2.0)
    return out


def check_counts(verts_stages, faces, segs, trusted=False):
    got = gpu_counts(verts_stages, faces, segs, trusted)
    want = R.batch_counts(verts_stages, faces, segs)
    assert np.array_equal(got, want), (got.tolist(), want.tolist())
    assert (got.sum(-1) == segs.shape[1] * segs.shape[2]).all()
    return got


# ---------------------------------------------------------------------------------------------- the integer part
def test_hand_cases_through_the_abi():
    seg = np.zeros((1, 8, 8), np.float32)
    seg[0, 2:6, 2:4] = 1.0
    v = np.array(LOWER + UPPER, np.float32)[None]
    lower = check_counts([v], [[0, 1, 2]], seg)
    upper = check_counts([v], [[3, 4, 5]], seg)
    both = check_counts([v], [[0, 1, 2], [3, 4, 5]], seg)
    assert lower[0, 0, :2].sum() == 6 and upper[0, 0, :2].sum() == 10 and both[0, 0].tolist() == [8, 8, 0, 48]  # the quad {2..5}^2, once
    assert np.array_equal(both, check_counts([v], [[0, 2, 1], [3, 5, 4]], seg))  # the other winding
    # dropped faces next to a good one: zero area, NaN, inf, outside the guard band, an index that is no vertex (device list: unchecked)
    d = np.array(LOWER + [(3, 3), (2, 2), (4, 4), (np.nan, 2), (20000, 3), (6, 6), (np.inf, 0)], np.float32)[None]
    for faces in ([[3, 4, 5], [0, 0, 1]], [[0, 1, 6], [0, 1, 9]], [[0, 1, 7]], [[0, 1, 10], [0, -1, 2]]):
        assert check_counts([d], faces, seg, trusted=True)[0, 0, :2].sum() == 0
        assert np.array_equal(check_counts([d], faces + [[0, 1, 2]], seg, trusted=True), lower)
    # larger than the image; W = 50: the last dword of a row is partial
    big = np.array([(-100, -100), (1000, -100), (-100, 1000)], np.float32)[None]
    seg50 = np.zeros((1, 8, 50), np.float32)
    seg50[0, 2:5, 30:50] = 1.0
    assert check_counts([big], [[0, 1, 2]], seg50)[0, 0].tolist() == [60, 340, 0, 0]
    half = np.array([(40.5, -5), (60, -5), (40.5, 20), (60, 20)], np.float32)[None]
    assert check_counts([half], [[0, 1, 2], [1, 3, 2]], seg50)[0, 0].tolist() == [27, 45, 33, 295]
    assert check_counts([big], [[0, 1, 2]], np.ones((1, 40, 50), np.float32))[0, 0].tolist() == [2000, 0, 0, 0]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", [(224, 224), (40, 50), (33, 31)])
def test_random_meshes(H, W, B):
    g = np.random.Generator(np.random.Philox(H * 1000 + W * 10 + B))
    stages = [np.stack([g.uniform(-0.2, 1.2, (12, 2)) * (W, H) for _ in range(B)]).astype(np.float32) for _ in range(2)]
    faces = g.integers(0, 12, (20, 3))
    got = check_counts(stages, faces, blob_masks(g, B, H, W))
    assert got[..., 0].sum() > 0 and got[..., 1].sum() > 0 and got[..., 2:].sum() > 0  # covered on and off the mask, and something uncovered
    empty = check_counts(stages, faces, np.zeros((B, H, W), np.float32))               # all background
    full = check_counts(stages, faces, np.full((B, H, W), 0.5, np.float32))            # all foreground
    assert (empty[..., 0] == 0).all() and (empty[..., 2] == 0).all() and (full[..., 1] == 0).all() and (full[..., 3] == 0).all()
    assert np.array_equal(empty[..., 1], full[..., 0])


def test_slivers_and_an_image_sized_face():
    """300 thin faces, short ones (walked by their own lane) and long ones (boxes of more than 64 samples, walked by the wave), plus one
    face over half of the image: both paths in one image"""
    g = np.random.Generator(np.random.Philox(11))
    H = W = 224
    a = g.uniform(0, 224, (300, 2))
    length, angle = np.where(np.arange(300) % 2, g.uniform(1, 6, 300), g.uniform(20, 150, 300)), g.uniform(0, 2 * np.pi, 300)
    along = np.stack([np.cos(angle), np.sin(angle)], 1)
    across = np.stack([-along[:, 1], along[:, 0]], 1) * g.uniform(0.2, 0.8, (300, 1))
    tip = a + along * length[:, None]
    v = np.concatenate([np.stack([a, tip + across, tip - across], 1).reshape(-1, 2), [(0, 0), (223, 0), (0, 223)]]).astype(np.float32)
    faces = np.arange(903).reshape(301, 3)
    boxes = (np.ptp(v[faces][..., 0], 1) + 1) * (np.ptp(v[faces][..., 1], 1) + 1)
    assert (boxes[:300] < 40).sum() > 100 and (boxes[:300] > 200).sum() > 100
    segs = blob_masks(g, 2, H, W)
    got = check_counts([np.stack([v, v[::-1] * 0.9 + 5])], faces[:, ::-1], segs)
    assert got[0, :, :2].sum(-1).min() > 224 * 224 // 3


@pytest.fixture(scope="module")
def predictor(tmp_path_factory):
    face_path = str(tmp_path_factory.mktemp("faces") / "smpl_faces.npy")
    np.save(face_path, synthetic.make_faces(0))
    cfg = types.SimpleNamespace(img_size=224, num_stage=3, batch_size=3, data_format="NHWC", checkpoint_dir=None, smpl_model_path=None,
                                smpl_face_path=face_path)
    p = hpe_amd.Predictor(cfg, smpl_model=synthetic.make_smpl_model(), mean_params=synthetic.make_mean_params(),
                          encoder_params=synthetic.make_encoder_params(), regressor_params=synthetic.make_regressor_params(variant="bounded"))
    yield p
    p.engine.close()


def lsp_targets(B, seed):
    g = np.random.Generator(np.random.Philox(seed))
    kp = np.concatenate([g.uniform(-0.6, 0.6, (B, 19, 2)), (g.uniform(0, 1, (B, 19, 1)) > 0.2)], 2).astype(np.float32)
    return kp


def test_full_body_three_stages_from_a_real_forward(predictor):
    images = cuda(synthetic.make_images(2, seed=21))
    stages = predictor.engine.forward(images, all_stages=True, want=("kp2d", "verts2d"))
    assert len(stages) == 3 and tuple(stages[0]["verts2d"].shape) == (2, 6890, 2)
    faces = synthetic.make_faces(0)
    assert faces.shape == (13776, 3)
    g = np.random.Generator(np.random.Philox(5))
    segs = blob_masks(g, 2, 224, 224)
    counts, _, _ = metrics.eval_scores([st["verts2d"] for st in stages], faces, cuda(segs), None, None)
    verts = [st["verts2d"].cpu().numpy() for st in stages]
    want = R.batch_counts(verts, faces, segs)
    got = counts.cpu().numpy()
    print("full body counts", got.tolist())
    assert np.array_equal(got, want) and got[..., :2].sum(-1).min() > 0  # every image has a silhouette in the frame


# ---------------------------------------------------------------------------------------------- the keypoint part
def test_keypoints_against_float64_and_equal_pck_counts():
    B, H, W = 6, 224, 224
    g = np.random.Generator(np.random.Philox(42))
    kp_gt = lsp_targets(B, 7)
    kp_gt[0, 9, 2] = 0    # no torso
    kp_gt[1, 12, 2] = 0   # no head
    kp_gt[2, :, 2] = 0    # nothing visible
    kp_gt[3, [9, 2, 13, 12], 2] = 1
    preds = [(kp_gt[:, :, :2] + g.normal(0, s, (B, 19, 2))).astype(np.float32) for s in (0.2, 0.08, 0.03)]
    counts, err, norm = metrics.eval_scores(None, None, None, cuda(kp_gt), [cuda(p) for p in preds], img_size=(H, W))
    assert counts is None
    err, norm = err.cpu().numpy(), norm.cpu().numpy()
    want_err, want_norm = R.keypoints(kp_gt, preds, H, W)
    tol = 4 * float(np.spacing(np.float32(max(H, W))))
    print("kp_err max |diff| %.3g, norm max |diff| %.3g, tol %.3g" % (np.abs(err - want_err).max(), np.abs(norm - want_norm).max(), tol))
    assert err.shape == (3, B, 19) and norm.shape == (B, 2)
    assert np.array_equal(err == -1.0, want_err == -1.0) and np.array_equal(norm == -1.0, want_norm == -1.0)  # exactly -1, nowhere else
    assert (err[:, kp_gt[:, :, 2] == 0] == -1.0).all() and norm[0, 0] == -1.0 and norm[1, 1] == -1.0 and (norm[2] == -1.0).all()
    assert (norm[3] > 0).all() and np.abs(err - want_err).max() <= tol and np.abs(norm - want_norm).max() <= tol
    # PCK: no visible joint of the float64 reference within 1e-4 relative of a threshold, then the hit counts must be equal
    e = want_err[:, :, :14]
    for c, alphas in ((0, metrics.PCK_ALPHAS), (1, metrics.PCKH_ALPHAS)):
        for a in alphas:
            thr = np.broadcast_to(a * want_norm[None, :, c, None], e.shape)
            live = (e >= 0) & (thr > 0)
            assert live.any() and (np.abs(e[live] - thr[live]) > 1e-4 * thr[live]).all(), (c, a)
    got, ref = Scores().add(None, err, norm), Scores().add(None, want_err, want_norm)
    hit_columns = [c for c in range(got.M) if c != 7]  # all but the pixel-error sum
    assert np.array_equal(got.sums.numpy()[:, hit_columns], ref.sums.numpy()[:, hit_columns])
    assert got.result()["pck_torso_0.2"] == ref.result()["pck_torso_0.2"] and 0 < got.result(0)["pck_torso_0.5"] < 1
    assert got.result()["torso_invalid_images"] == (want_norm[:, 0] < 0).sum() >= 2 and got.result()["head_invalid_images"] == (want_norm[:, 1] < 0).sum() >= 2
    # at another image size the scale follows H and W separately
    err2, norm2 = [t.cpu().numpy() for t in metrics.eval_scores(None, None, None, cuda(kp_gt), [cuda(preds[1])], img_size=(40, 50))[1:]]
    w2 = R.keypoints(kp_gt, preds[1:2], 40, 50)
    tol2 = 4 * float(np.spacing(np.float32(50)))
    assert np.abs(err2 - w2[0]).max() <= tol2 and np.abs(norm2 - w2[1]).max() <= tol2


# ---------------------------------------------------------------------------------------------- the contract
def scene(seed, B=3, H=40, W=50, stages=2):
    g = np.random.Generator(np.random.Philox(seed))
    verts = [cuda(np.stack([g.uniform(-0.2, 1.2, (12, 2)) * (W, H) for _ in range(B)])) for _ in range(stages)]
    faces = cuda(g.integers(0, 12, (20, 3)), np.int32)
    kp_gt = cuda(lsp_targets(B, seed))
    kp2d = [(kp_gt[:, :, :2] + 0.05 * (s + 1)).contiguous() for s in range(stages)]
    return verts, faces, cuda(blob_masks(g, B, H, W)), kp_gt, kp2d


def bits(out):
    return [t.cpu().numpy().view(np.int32).copy() for t in out]


def test_same_bits_again_and_from_a_replayed_graph():
    a, b = scene(1), scene(2)
    first = bits(metrics.eval_scores(*a))
    other = bits(metrics.eval_scores(*b))
    again = bits(metrics.eval_scores(*a))
    assert all(np.array_equal(x, y) for x, y in zip(first, again)) and not np.array_equal(first[0], other[0])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # one stream, one kernel node
        out = metrics.eval_scores(*a)
    for _ in range(2):
        for t in out:
            t.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        assert all(np.array_equal(x, y) for x, y in zip(first, bits(out)))


def test_either_part_alone():
    verts, faces, segs, kp_gt, kp2d = scene(3)
    counts, err, norm = metrics.eval_scores(verts, faces, segs, kp_gt, kp2d)
    sil = metrics.eval_scores(verts, faces, segs, None, None)
    kps = metrics.eval_scores(None, None, None, kp_gt, kp2d, img_size=(40, 50))
    assert sil[1] is None and sil[2] is None and kps[0] is None
    assert torch.equal(sil[0], counts) and torch.equal(kps[1], err) and torch.equal(kps[2], norm)
    assert torch.equal(metrics.eval_scores(None, None, segs, kp_gt, kp2d)[1], err)  # the image size from the masks


def test_refusals():
    lib = _lib.load()
    verts, faces, segs, kp_gt, kp2d = scene(4)
    B, P, K, H, W, n = 3, 12, 19, 40, 50, 2
    counts = torch.full((n, B, 4), -5, dtype=torch.int32, device="cuda")
    err = torch.full((n, B, K), -5.0, device="cuda")
    norm = torch.full((B, 2), -5.0, device="cuda")
    vp = (C.c_void_p * n)(*[t.data_ptr() for t in verts])
    kp = (C.c_void_p * n)(*[t.data_ptr() for t in kp2d])

    def call(vp=vp, faces=faces.data_ptr(), F=20, seg=segs.data_ptr(), gt=kp_gt.data_ptr(), kp=kp, n=n, B=B, P=P, K=K, H=H, W=W,
             counts=counts.data_ptr(), err=err.data_ptr(), norm=norm.data_ptr()):
        rc = lib.hpe_eval_scores(vp, faces, F, seg, gt, kp, n, B, P, K, H, W, counts, err, norm, None)
        return rc, lib.hpe_last_error().decode()

    hole = (C.c_void_p * n)(verts[0].data_ptr(), None)
    for name, kw, word in (("counts", dict(counts=None), "counts_dev"), ("kp_err", dict(err=None), "kp_err_dev"), ("norm", dict(norm=None), "norm_dev"),
                           ("B", dict(B=0), "batch"), ("n_stage", dict(n=0), "n_stage"), ("n_stage", dict(n=17), "n_stage"),
                           ("faces", dict(faces=None), "faces_dev"), ("seg", dict(seg=None), "seg_dev"), ("kp2d", dict(kp=None), "kp2d_dev"),
                           ("a stage", dict(vp=hole), "verts2d_dev[1]"), ("nothing", dict(vp=None, gt=None), "nothing"),
                           ("LDS", dict(H=1024, W=1024), "LDS"), ("LDS", dict(H=256, W=1000), "LDS"), ("size", dict(H=0), "image size")):
        rc, msg = call(**kw)
        assert rc == 1 and word in msg, (name, rc, msg)  # HPE_ERR_INVALID, and the message names the clause
    torch.cuda.synchronize()
    assert (counts == -5).all() and (err == -5).all() and (norm == -5).all()  # nothing was launched
    assert call()[0] == 0
    wide = torch.zeros(3, 255, 1000, device="cuda")  # 2 * 255 * 32 dwords + 16 bytes = 65296 <= 65536: the tallest 1000-wide image that fits
    assert call(H=255, W=1000, seg=wide.data_ptr(), gt=None)[0] == 0
    torch.cuda.synchronize()
    assert (counts[..., 2] == 0).all() and (counts.sum(-1) == 255 * 1000).all()
    with pytest.raises(hpe_amd.HpeError, match="outside \\[0, 12\\)"):  # the host path checks what it uploads
        metrics.eval_scores(verts, np.array([[0, 1, 12]]), segs, None, None)


# ---------------------------------------------------------------------------------------------- Predictor and Trainer
def test_score_step_and_scores_over_two_batches(predictor):
    g = np.random.Generator(np.random.Philox(8))
    batches = []
    for B, seed in ((3, 31), (2, 32)):
        batches.append((cuda(synthetic.make_images(B, seed=seed)), cuda(blob_masks(g, B, 224, 224))[..., None], cuda(lsp_targets(B, seed))))
    outs = [predictor.score_step(*b) for b in batches]
    counts, err, norm, iou = outs[0]
    assert tuple(counts.shape) == (3, 3, 4) and tuple(err.shape) == (3, 3, 19) and tuple(norm.shape) == (3, 2) and tuple(iou.shape) == (3, 3)
    c = counts.cpu().numpy().astype(np.float64)
    assert np.array_equal(iou.cpu().numpy(), c[..., 0] / (c[..., 0] + c[..., 1] + c[..., 2])) and iou.dtype == torch.float64
    last = predictor.score_step(*batches[0], all_stages=False)
    assert tuple(last[0].shape) == (1, 3, 4) and torch.equal(last[0][0], counts[-1]) and torch.equal(last[1][0], err[-1])
    two, one = Scores(), Scores()
    for o in outs:
        two.add(*o[:3])
    one.add(*[torch.cat([outs[0][i], outs[1][i]], 0 if i == 2 else 1) for i in range(3)])
    a, b = two.sums.cpu().numpy(), one.sums.cpu().numpy()
    ints = [k for k in range(two.M) if k not in (4, 7)]  # the counts; columns 4 and 7 are float64 sums of floats
    assert two.sums.is_cuda and np.array_equal(a[:, ints], b[:, ints]) and np.allclose(a, b, rtol=1e-12, atol=0)
    r = two.result()
    assert r["images"] == 5 and r["kp_images"] == 5 and r["tp"] + r["fp"] + r["fn"] + r["tn"] == 5 * 224 * 224 and 0 <= r["iou"] <= 1
    nofaces = types.SimpleNamespace(**{k: v for k, v in vars(predictor).items()})
    nofaces.smpl_face_path, nofaces._score_faces = None, None
    with pytest.raises(FileNotFoundError, match="needs the SMPL faces: set config.smpl_face_path"):
        hpe_amd.Predictor.score_faces(nofaces)


def test_score_checkpoint_draws_best_and_worst(weights, data, tmp_path):  # noqa: F811
    faces = str(tmp_path / "smpl_faces.npy")
    np.save(faces, synthetic.make_faces())
    images, mocap = data
    model_dir = str(tmp_path / "model")
    cfg = make_config(weights, tmp_path / "ckpt", use_validation=True, model_dir=model_dir, smpl_face_path=faces)
    tr = hpe_amd.Trainer(cfg, hpe_amd.RecordDataset(images, TRAINER_B), None, val_dataset=hpe_amd.RecordDataset(images, TRAINER_B),
                         validation_only=True, log=lambda s: None)
    try:
        out = tr.score_checkpoint(restore=False, draw_best_worst=1)  # the live weights, two batches of two records
        assert out["batches"] == 2 and len(out["stages"]) == STAGES and out["images"] == out["kp_images"] == 4
        assert out["tp"] + out["fp"] + out["fn"] + out["tn"] == 4 * 224 * 224
        assert out["iou"] == out["tp"] / (out["tp"] + out["fp"] + out["fn"]) and out["fb_f1"] == 2 * out["tp"] / (2 * out["tp"] + out["fp"] + out["fn"])
        same_result(out["stages"][-1], {k: v for k, v in out.items() if k not in ("stages", "batches")})
        ev = events_of(model_dir, "checkpoint_scores")
        assert [v["tag"] for _s, v in ev] == ["best_kp/0", "worst_kp/0", "best_iou/0", "worst_iou/0"]
        assert all(1 <= s <= 4 for s, _v in ev) and all((v["image"]["height"], v["image"]["width"]) == (STAGES * 224, 3 * 224) for _s, v in ev)
        # config.score_validation's block, from what val_step returns: the same keypoints, and vertices reprojected by another kernel
        # than the forward's (one float32 rounding apart at most, which can move a sample across an edge only where the sample is
        # within 1/256 px of it: a handful of the ~1e4 pixels of a union)
        loaded = tr._load_images(next(iter(tr.val_dataset)), augment=False)
        t = tr.score_val_result(tr.val_step(*loaded), loaded[1], loaded[2])
        want = Scores().add(*tr.predictor.score_step(*loaded)[:3]).result()
        assert all(t[k].is_cuda and t[k].dim() == 0 for k in ("iou", "fb_f1", "pck_torso_0.2", "pckh_0.5"))
        for k in ("pck_torso_0.2", "pckh_0.5"):
            assert float(t[k]) == want[k] or (want[k] != want[k] and float(t[k]) != float(t[k])), k
        print("score_validation iou %.6f, score_step iou %.6f" % (float(t["iou"]), want["iou"]))
        assert abs(float(t["iou"]) - want["iou"]) <= 2e-3 and abs(float(t["fb_f1"]) - want["fb_f1"]) <= 2e-3
    finally:
        tr.engine.close()
