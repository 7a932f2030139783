"""CPU tests of the checkpoint scores (DESIGN.md "Checkpoint scores"): the integer silhouette reference tests/eval_ref.py on cases worked out
by hand, the arithmetic of ``metrics.Scores`` in float64 on made-up counts, its reduction over a world-2 gloo group, and the plumbing of
``Trainer.score_checkpoint`` / ``config.score_validation`` with stubs in place of the engine."""
import json
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import hpe_amd
from hpe_amd import metrics, trainer as T
from hpe_amd.summary import SummaryWriter, read_events

Scores = metrics.Scores

import _scores_reduce_worker as RW
import eval_ref as R


def pixels(mask):
    """the covered pixels as a set of (x, y) = (column, row)"""
    return {(int(x), int(y)) for y, x in zip(*np.nonzero(mask))}


def same_result(a, b, float_keys=()):
    """equal results, NaN == NaN; float_keys: ratios of float64 sums, which depend on how the sum was associated: 1e-12 relative"""
    assert set(a) == set(b)
    for k in a:
        x, y = (a[k], b[k]) if isinstance(a[k], list) else ([a[k]], [b[k]])
        tol = 1e-12 if k in float_keys else 0.0
        assert len(x) == len(y) and all((math.isnan(p) and math.isnan(q)) or abs(p - q) <= tol * abs(q) for p, q in zip(x, y)), (k, a[k], b[k])


FLOAT_SUMS = (4, 7)  # Scores.sums columns that are sums of floats (per-image IoU, pixel error); every other column counts
FLOAT_KEYS = ("iou_mean", "mean_px_error")


def same_sums(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ints = [c for c in range(a.shape[1]) if c not in FLOAT_SUMS]
    assert a.shape == b.shape and np.array_equal(a[:, ints], b[:, ints])
    assert np.all(np.abs(a[:, FLOAT_SUMS] - b[:, FLOAT_SUMS]) <= 1e-12 * np.abs(b[:, FLOAT_SUMS]))


# ---------------------------------------------------------------------------------------------- eval_ref.silhouette by hand
# Mask pixel (row i, column j) is the point (j, i), so integer vertices lie exactly on samples.  In the renderer's orientation (positive
# edge function with y down) an edge owns the samples on it when it points down, or along -x when horizontal.
LOWER = [(1, 1), (5, 1), (1, 5)]  # right angle at (1, 1): the top edge (y = 1, along +x) and the left edge (x = 1, pointing up) own nothing,
#                                   the hypotenuse x + y = 6 points down and owns its samples
UPPER = [(5, 5), (1, 5), (5, 1)]  # the other half of the square [1, 5]^2: its hypotenuse points up (owns nothing), x = 5 points down and
#                                   y = 5 runs along -x: both own their samples
LOWER_PIXELS = {(2, 2), (3, 2), (4, 2), (2, 3), (3, 3), (2, 4)}  # x > 1, y > 1, x + y <= 6


def test_one_triangle_top_left_rule_on_all_three_edges():
    got = pixels(R.silhouette(np.array(LOWER, np.float32), [[0, 1, 2]], 8, 8))
    assert got == LOWER_PIXELS
    assert not any(x == 1 or y == 1 for x, y in got)      # the two edges that own nothing, vertices included
    assert {(4, 2), (3, 3), (2, 4)} <= got                # the samples exactly on the owning edge


def test_two_triangles_sharing_an_edge_tile_the_quad():
    v = np.array(LOWER + UPPER, np.float32)
    lower = R.silhouette(v, [[0, 1, 2]], 8, 8)
    upper = R.silhouette(v, [[3, 4, 5]], 8, 8)
    both = R.silhouette(v, [[0, 1, 2], [3, 4, 5]], 8, 8)
    assert not (lower & upper).any()                       # no sample of the shared edge x + y = 6 belongs to both
    assert np.array_equal(both, lower | upper)
    assert pixels(both) == {(x, y) for x in range(2, 6) for y in range(2, 6)}  # the quad, half open at the top and at the left
    assert lower.sum() + upper.sum() == both.sum() == 16


def test_both_windings_give_the_same_bits():
    g = np.random.Generator(np.random.Philox(1))
    v = g.uniform(-3, 40, (12, 2)).astype(np.float32)
    f = g.integers(0, 12, (20, 3))
    a = R.silhouette(v, f, 33, 31)
    assert a.any() and np.array_equal(a, R.silhouette(v, f[:, [0, 2, 1]], 33, 31))
    assert np.array_equal(a, R.silhouette(v, f[::-1], 33, 31))  # a union: the order of the faces does not matter


def test_dropped_faces():
    v = np.array(LOWER + [(3, 3), (2, 2), (4, 4), (np.nan, 2), (20000, 3), (6, 6), (np.inf, 0)], np.float32)
    zero_area = [[3, 4, 5], [0, 0, 1]]       # collinear, repeated vertex
    bad = [[0, 1, 6], [0, 1, 9]]             # NaN, inf
    guard = [[0, 1, 7]]                      # x = 20000 > 16384
    outside = [[0, 1, 10], [0, -1, 2]]       # an index that is no vertex
    for faces in (zero_area, bad, guard, outside):
        assert not R.silhouette(v, faces, 8, 8).any(), faces
        assert pixels(R.silhouette(v, faces + [[0, 1, 2]], 8, 8)) == LOWER_PIXELS  # the good face next to them is still drawn
    assert R.silhouette(np.array([(0, 0), (16384, 0), (0, 16384)], np.float32), [[0, 1, 2]], 8, 8)[1:, 1:].all()  # on the band: kept


def test_triangle_larger_than_the_image_and_partial_last_dword():
    big = np.array([(-100, -100), (1000, -100), (-100, 1000)], np.float32)
    for H, W in ((40, 50), (8, 50), (33, 31)):
        assert R.silhouette(big, [[0, 1, 2]], H, W).all()
    seg = np.zeros((8, 50), np.float32)
    seg[2:5, 30:50] = 1.0   # columns 32..49 live in the partial second dword of a row
    assert R.counts(big, [[0, 1, 2]], seg).tolist() == [60, 340, 0, 0]
    half = np.array([(40.5, -5), (60, -5), (40.5, 20), (60, 20)], np.float32)  # covers columns 41..49 of every row
    p = R.silhouette(half, [[0, 1, 2], [1, 3, 2]], 8, 50)
    assert p[:, 41:].all() and not p[:, :41].any()
    assert R.counts(half, [[0, 1, 2], [1, 3, 2]], seg).tolist() == [27, 45, 33, 295]


def test_snapping_is_round_half_even_at_1_256():
    X, Y, ok = R.snap(np.array([[0.5 / 256, 1.5 / 256], [2.5 / 256, -0.5 / 256], [16384.0, -16384.0], [16384.01, 0]], np.float32))
    assert X[:3].tolist() == [0, 2, 16384 * 256] and Y[:3].tolist() == [2, 0, -16384 * 256] and ok.tolist() == [True, True, True, False]


def test_keypoint_reference_by_hand():
    gt = np.zeros((1, 14, 3), np.float32)
    gt[0, :, 2] = 1
    gt[0, 9, :2], gt[0, 2, :2] = (0.5, 0.0), (0.0, 0.0)      # torso: 0.5 * 0.5 * 200 = 50 px
    gt[0, 13, :2], gt[0, 12, :2] = (0.0, -0.25), (0.0, 0.0)  # head: 0.25 * 0.5 * 100 = 12.5 px
    gt[0, 5, 2] = 0
    pred = gt[:, :, :2].copy()
    pred[0, 0] += (0.03, 0.08)   # 3 px and 4 px at W = 200, H = 100
    err, norm = R.keypoints(gt, [pred], 100, 200)
    assert abs(err[0, 0, 0] - 5.0) < 1e-5 and err[0, 0, 5] == -1.0 and err[0, 0, 1] == 0.0
    assert np.allclose(norm, [[50.0, 12.5]])
    gt[0, 12, 2] = 0
    assert R.keypoints(gt, [pred], 100, 200)[1].tolist() == [[50.0, -1.0]]


# ---------------------------------------------------------------------------------------------- Scores
def test_scores_silhouette_arithmetic_and_empty_union():
    counts = np.array([[[10, 5, 5, 80], [0, 0, 0, 100], [50, 0, 50, 0]]], np.int32)
    r = Scores().add(counts).result()
    assert r["iou"] == 60 / 120 and r["fb_f1"] == 120 / 180 and r["fb_accuracy"] == 240 / 300
    assert (r["iou_mean"], r["iou_images"], r["iou_empty_union"], r["images"]) == (0.5, 2, 1, 3)  # the empty image is counted, not averaged
    assert math.isnan(r["mean_px_error"]) and math.isnan(r["pck_torso_0.2"]) and r["kp_images"] == 0
    iou = metrics.image_iou(torch.from_numpy(counts))
    assert iou[0, 0] == 0.5 and torch.isnan(iou[0, 1]) and iou[0, 2] == 0.5
    only_empty = Scores().add(counts[:, 1:2]).result()
    assert math.isnan(only_empty["iou"]) and math.isnan(only_empty["iou_mean"]) and only_empty["fb_accuracy"] == 1.0


def pck_by_loops(err, norm, col, alpha, joints=14):
    hits = seen = 0
    per_joint = [[0, 0] for _ in range(joints)]
    for b in range(err.shape[0]):
        if not norm[b, col] > 0:
            continue
        for k in range(joints):
            if err[b, k] >= 0:
                seen += 1
                per_joint[k][1] += 1
                if float(err[b, k]) <= alpha * float(norm[b, col]):
                    hits += 1
                    per_joint[k][0] += 1
    return hits, seen, per_joint


def test_scores_keypoint_arithmetic_and_invalid_torso():
    err = np.full((1, 3, 19), -1.0, np.float32)
    err[0, 0, :6] = [0.5, 1.5, 2.5, 6.0, 0.0, 4.0]     # torso 10: 0.1 -> 2 hits (0.5, 0.0), 0.2 -> 3, 0.5 -> 5 of 6
    err[0, 1, :4] = [1.0, 1.0, 1.0, 1.0]               # torso invalid: in no PCK, in the pixel error
    err[0, 2, 10:16] = [2.0, 9.0, 30.0, 3.0, 0.1, 0.1]  # torso 20, head -1; joints 14, 15 are not LSP joints: in nothing
    norm = np.array([[10.0, 4.0], [-1.0, 5.0], [20.0, -1.0]], np.float32)
    r = Scores().add(None, err, norm).result()
    assert r["pck_torso_0.1"] == 3 / 10 and r["pck_torso_0.2"] == 5 / 10 and r["pck_torso_0.5"] == 8 / 10
    assert r["pckh_0.5"] == (3 + 4) / (6 + 4)          # image 0: <= 2 px: 0.5, 1.5, 0.0; image 1: <= 2.5 px: all four
    assert (r["kp_images"], r["torso_invalid_images"], r["head_invalid_images"]) == (3, 1, 1)
    assert abs(r["mean_px_error"] - (14.5 + 4.0 + 44.0) / 14) < 1e-12
    for alpha in (0.1, 0.2, 0.5):
        hits, seen, per_joint = pck_by_loops(err[0], norm, 0, alpha)
        assert r["pck_torso_%g" % alpha] == hits / seen
    want = [h / s if s else float("nan") for h, s in pck_by_loops(err[0], norm, 0, 0.2)[2]]
    assert len(r["pck_per_joint"]) == 14
    assert all((math.isnan(a) and math.isnan(b)) or a == b for a, b in zip(r["pck_per_joint"], want))
    assert math.isnan(r["iou"]) and r["images"] == 0


def test_scores_thresholds_are_arguments():
    err = np.full((2, 1, 14), -1.0, np.float32)
    err[0, 0, :4] = [1.0, 2.9, 3.1, 7.0]
    err[1, 0, :4] = [1.0, 2.0, 3.0, 8.0]
    norm = np.array([[10.0, 10.0]], np.float32)
    s = Scores(pck_alphas=(0.3, 0.75), pckh_alphas=(0.25, 0.1), per_joint_alpha=0.75).add(None, err, norm)
    first, last = s.result(0), s.result()
    assert set(k for k in last if k.startswith("pck")) == {"pck_torso_0.3", "pck_torso_0.75", "pckh_0.25", "pckh_0.1", "pck_per_joint"}
    assert (first["pck_torso_0.3"], first["pck_torso_0.75"], first["pckh_0.25"], first["pckh_0.1"]) == (0.5, 1.0, 0.25, 0.25)
    assert (last["pck_torso_0.3"], last["pck_torso_0.75"], last["pckh_0.25"], last["pckh_0.1"]) == (0.75, 0.75, 0.5, 0.25)
    assert last["pck_per_joint"][:4] == [1.0, 1.0, 1.0, 0.0] and len(s.results()) == 2
    same_result(s.results()[0], first)
    with pytest.raises(ValueError):
        Scores(pck_alphas=(0.1,), per_joint_alpha=0.2)
    with pytest.raises(ValueError):
        Scores().result()


def test_two_batches_equal_their_concatenation():
    batches = RW.made_up_batches()
    two, one = Scores(), Scores()
    for b in batches:
        two.add(*b)
    one.add(np.concatenate([b[0] for b in batches], 1), np.concatenate([b[1] for b in batches], 1), np.concatenate([b[2] for b in batches]))
    assert two.sums.dtype == torch.float64
    same_sums(two.sums.numpy(), one.sums.numpy())
    for i in range(3):
        same_result(two.result(i), one.result(i), FLOAT_KEYS)
    t = two.result_tensors()
    assert all(v.dtype == torch.float64 for v in t.values()) and float(t["iou"]) == two.result()["iou"]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_scores_reduce_on_gloo_world2(tmp_path):
    mp.spawn(RW.worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    ranks = [json.load(open(tmp_path / ("rank%d.json" % k))) for k in range(2)]
    batches = RW.made_up_batches()
    whole = Scores().add(np.concatenate([b[0] for b in batches], 1), np.concatenate([b[1] for b in batches], 1),
                         np.concatenate([b[2] for b in batches]))
    for r in ranks:  # both ranks end with the sums of the concatenated batches
        same_sums(r["sums"], whole.sums.numpy())
        assert r["stages"] == 3
        same_result(r["result"], whole.result(), FLOAT_KEYS)
    assert ranks[0]["sums"] == ranks[1]["sums"]
    assert whole.result()["images"] == 5 and whole.result()["iou_empty_union"] == 2


def test_exports():
    assert hpe_amd.Scores is Scores and hpe_amd.eval_scores is metrics.eval_scores
    assert not hasattr(hpe_amd, "upload_faces") and not hasattr(hpe_amd, "_cuda_f32")  # helpers stay in the module
    assert "hpe_eval_scores" in hpe_amd._lib.declared_symbols()


def test_upload_faces_refuses_an_index_that_is_no_vertex():
    for bad in ([[0, 1, 12]], [[0, -1, 2]]):
        with pytest.raises(hpe_amd.HpeError, match="error 1.*outside \\[0, 12\\)"):
            metrics.upload_faces(np.array(bad), 12, "cpu")
    with pytest.raises(hpe_amd.HpeError, match="error 1"):
        metrics.upload_faces(np.zeros((3, 2), np.int64), 12, "cpu")
    f = metrics.upload_faces(np.array([[0, 1, 11]], np.int64), 12, "cpu")
    assert f.dtype == torch.int32 and f.tolist() == [[0, 1, 11]]


# ---------------------------------------------------------------------------------------------- Trainer plumbing, no engine
def test_best_worst_ranks_by_value_then_record_order():
    bw = T.BestWorst(2)
    for record, value in enumerate([3.0, 1.0, float("nan"), 1.0, 7.0, 7.0, 0.5]):
        bw.add(value, record)
    assert [r for _v, r in bw.low] == [6, 1] and [r for _v, r in bw.high] == [4, 5]  # ties: the earlier record first; NaN is not ranked
    assert bw.records() == {1, 4, 5, 6}
    none = T.BestWorst(0)
    none.add(1.0, 0)
    assert none.records() == set()


class StubPredictor(object):
    """score_step from a table of made-up outputs, one entry per call"""

    def __init__(self, batches):
        self.batches, self.calls, self.img_size = batches, 0, 224

    def score_step(self, images, seg_gts, kp2d_gts, all_stages=True):
        counts, err, norm = [torch.from_numpy(a) for a in self.batches[self.calls]]
        self.calls += 1
        assert images.shape[0] == counts.shape[1]
        return counts, err, norm, metrics.image_iou(counts)


def bare_trainer(**attrs):
    tr = object.__new__(T.Trainer)  # the methods under test read attributes only
    base = dict(rank=0, world=1, reducer=None, model_dir=None, checkpoint_dir=None, use_kpr_loss=True, use_mesh_repro_loss=False, log_img_step=0,
                score_validation=False, val_writer=None)
    base.update(attrs)
    for k, v in base.items():
        setattr(tr, k, v)
    return tr


def test_score_checkpoint_sums_the_pass_without_an_engine():
    batches = RW.made_up_batches()
    loaded = [tuple(torch.zeros(b[0].shape[1], 1) for _ in range(3)) for b in batches]  # ready (images, segs, kp) triples pass through
    tr = bare_trainer(predictor=StubPredictor(batches), val_dataset=loaded)
    out = tr.score_checkpoint(restore=False)
    whole = Scores()
    for b in batches:
        whole.add(*b)
    assert out["batches"] == 2 and len(out["stages"]) == 3 and tr.predictor.calls == 2
    same_result({k: v for k, v in out.items() if k not in ("stages", "batches")}, whole.result())  # the same adds in the same order
    for i in range(3):
        same_result(out["stages"][i], whole.result(i))
    with pytest.raises(RuntimeError, match="model_dir or config.checkpoint_dir"):
        tr.score_checkpoint(restore=False, draw_best_worst=1)
    with pytest.raises(RuntimeError, match="validation dataset"):
        bare_trainer(predictor=None, val_dataset=None).score_checkpoint(restore=False)
    with pytest.raises(ValueError, match="no batch"):
        bare_trainer(predictor=StubPredictor([]), val_dataset=[]).score_checkpoint(restore=False)


def event_bytes(path):
    return open(path, "rb").read()


def test_validation_events_with_and_without_score_validation(tmp_path):
    """flag unset: the validation event file holds exactly the bytes the block wrote before the flag existed (one kpr scalar per step,
    restated here with a writer of its own); flag set: the four metrics/ scalars follow, read from result["scores"]"""
    clock = lambda: 1234.5  # noqa: E731
    result = {"kpr_losses": [torch.tensor(0.25), torch.tensor(0.5)]}
    with SummaryWriter(str(tmp_path / "want"), clock=clock) as w:
        w.scalar("generator/kpr_loss", result["kpr_losses"][-1], 2)
        w.scalar("generator/kpr_loss", result["kpr_losses"][-1], 4)
        want = w.path
    tr = bare_trainer(val_writer=SummaryWriter(str(tmp_path / "off"), clock=clock))
    for step in (2, 4):
        tr._summarize_val_step(step, dict(result), None)
    tr.val_writer.close()
    assert event_bytes(tr.val_writer.path) == event_bytes(want)

    scores = Scores().add(*RW.made_up_batches()[1]).result_tensors()
    on = bare_trainer(val_writer=SummaryWriter(str(tmp_path / "on"), clock=clock), score_validation=True)
    on._summarize_val_step(2, dict(result, scores=scores), None)
    on.val_writer.close()
    ev = read_events(on.val_writer.path)[1:]
    assert [(e["step"], e["values"][0]["tag"]) for e in ev] == [(2, "generator/kpr_loss")] + [(2, "metrics/" + t) for t in T.SCORE_TAGS]
    assert T.SCORE_TAGS == ("iou", "fb_f1", "pck_torso_0.2", "pckh_0.5")
    for e, tag in zip(ev[1:], T.SCORE_TAGS):
        assert e["values"][0]["simple_value"] == float(np.float32(float(scores[tag])))
