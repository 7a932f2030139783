"""GPU tests of the Trainer's summaries (run with -m gpu on an MI355X), on the smallest trainer tests/test_gpu_trainer.py uses (its
helpers are imported): one epoch of two steps with a validation step at step 2, once with summaries off and once with
``model_dir`` set and ``log_img_step = 2``.  Watching must not change the run: parameters, statistics and losses are bit-identical.
The event files hold the reference's tags at steps 1 and 2 and the ``vis_images`` panels at step 2, which decode to [T*224, 672, 3].
The bone-length keys appear only with ``do_bone_evaluation`` and match a float64 evaluation of the same joints."""
import os

import numpy as np
import pytest
import torch

import hpe_amd
from hpe_amd import synthetic

from test_gpu_trainer import B, STAGES, data, make_trainer, same, tensors_of, weights  # noqa: F401  (weights, data: fixtures)

pytestmark = pytest.mark.gpu
S = 224
SCALAR_TAGS = ["generator/kpr_loss", "critic/critic_network_loss", "critic/generator_critic_loss", "critic/penalty"]
RESULT_OF_TAG = {"generator/kpr_loss": lambda r: r["kpr_losses"][-1], "critic/critic_network_loss": lambda r: r["critic_network_loss"],
                 "critic/generator_critic_loss": lambda r: r["generator_critic_losses"][-1], "critic/penalty": lambda r: r["critic_penalty"]}


def run(weights, data, ckpt, **kw):  # noqa: F811
    tr = make_trainer(weights, data, ckpt, epoch=1, use_validation=True, **kw)
    results, step = [], tr.train_step
    tr.train_step = lambda *a, **k: results.append(step(*a, **k)) or results[-1]
    out = tr.train(save_every=100)
    assert out == {"steps": 2, "epochs": 1, "saved": [], "validations": 1}
    return tr, results


@pytest.fixture(scope="module")
def runs(weights, data, tmp_path_factory):  # noqa: F811
    d = tmp_path_factory.mktemp("summaries")
    faces = str(d / "smpl_faces.npy")
    np.save(faces, synthetic.make_faces())
    off, off_results = run(weights, data, d / "ckpt_off")
    out = {"off": tensors_of(off), "off_results": off_results, "off_keys": set(off_results[0])}
    off.engine.close()
    model_dir = str(d / "model")
    on, on_results = run(weights, data, d / "ckpt_on", model_dir=model_dir, log_img_step=2, smpl_face_path=faces)
    out.update(on=tensors_of(on), on_results=on_results, model_dir=model_dir, trainer=on)
    yield out
    on.engine.close()


def events_of(model_dir, name):
    files = os.listdir(os.path.join(model_dir, name))
    assert len(files) == 1 and files[0].startswith("events.out.tfevents.") and files[0].endswith(".v2")
    ev = hpe_amd.read_events(os.path.join(model_dir, name, files[0]))
    assert ev[0]["file_version"] == "brain.Event:2" and all(len(e["values"]) == 1 for e in ev[1:])
    return [(e["step"], e["values"][0]) for e in ev[1:]]


def test_summaries_do_not_change_the_run(runs):
    for k in ("regressor", "encoder", "critic", "stats"):
        assert same(runs["on"][k], runs["off"][k]), k
    assert len(runs["on_results"]) == len(runs["off_results"]) == 2
    for a, b in zip(runs["on_results"], runs["off_results"]):
        assert set(a) == set(b) == runs["off_keys"]
        for tag, pick in RESULT_OF_TAG.items():
            assert same(pick(a), pick(b)), tag
        assert same(a["pred_keypoints"], b["pred_keypoints"]) and all(same(x, y) for x, y in zip(a["thetas"], b["thetas"]))
    assert not os.path.exists(os.path.join(os.path.dirname(runs["model_dir"]), "ckpt_off", "training"))  # off: nothing was written


def test_training_events_hold_the_references_tags(runs):
    ev = events_of(runs["model_dir"], "training")
    scalars = [(s, v["tag"], v["simple_value"]) for s, v in ev if "simple_value" in v]
    assert [(s, t) for s, t, _ in scalars] == [(s, t) for s in (1, 2) for t in SCALAR_TAGS]
    for s, tag, value in scalars:  # the values are the step's losses, as float32
        assert value == float(RESULT_OF_TAG[tag](runs["on_results"][s - 1]).float().cpu()), (s, tag)
    images = [(s, v) for s, v in ev if "image" in v]
    assert [(s, v["tag"]) for s, v in images] == [(2, "vis_images/%d" % i) for i in range(3)]  # show_these of a batch of 2: rows 0, 1, 0
    # the reference's order inside a step: generator scalars, images, critic scalars
    order = [v["tag"] for s, v in ev if s == 2]
    assert order == SCALAR_TAGS[:1] + ["vis_images/0", "vis_images/1", "vis_images/2"] + SCALAR_TAGS[1:]
    streams = [v["image"]["encoded_image_string"] for _, v in images]
    for _, v in images:
        assert (v["image"]["height"], v["image"]["width"], v["image"]["colorspace"]) == (STAGES * S, 3 * S, 3)
    frames = [f.cpu().numpy() for f in hpe_amd.decode_png_batch(streams, channels=3).frames]
    assert all(f.shape == (STAGES * S, 3 * S, 3) for f in frames)
    assert np.array_equal(frames[0], frames[2]) and not np.array_equal(frames[0], frames[1])  # rows 0, 1, 0
    assert all(f[:, :S].std() > 0 and f[:, S:2 * S].std() > 0 for f in frames)  # the crop column and the rendered column hold a picture


def test_validation_events(runs):
    ev = events_of(runs["model_dir"], "validation")
    assert [(s, v["tag"]) for s, v in ev] == [(2, "generator/kpr_loss")] + [(2, "vis_images/%d" % i) for i in range(3)]
    frames = hpe_amd.decode_png_batch([v["image"]["encoded_image_string"] for _, v in ev[1:]], channels=3).frames
    assert all(tuple(f.shape) == (STAGES * S, 3 * S, 3) for f in frames)


def bone_sum(joints, dtype):
    """the restatement: B = X^T C per row with the reference's C (src/models.py:97-112), the diagonal of B^T B summed over the 13
    bones, averaged over the rows -- in ``dtype`` throughout"""
    ends = [1, 2, 8, 9, 3, 4, 7, 8, 12, 12, 9, 10, 13]
    Cm = np.zeros((14, 13), dtype)
    Cm[np.arange(13), np.arange(13)] = 1
    Cm[ends, np.arange(13)] = -1
    X = joints[:, :14].astype(dtype)
    Bm = np.einsum("njc,jk->nck", X, Cm).astype(dtype)
    kcs = np.einsum("nck,ncl->nkl", Bm, Bm).astype(dtype)
    return np.diagonal(kcs, axis1=1, axis2=2).sum(axis=1, dtype=dtype).mean(dtype=dtype)


def test_bone_lengths_only_when_asked_and_equal_to_float64(runs, data):  # noqa: F811
    """Tolerance: what float32 costs the restatement itself on these joints -- |float32 run - float64 run| --, but no less than one
    rounding of the result to float32 (2^-24 relative: a float32 evaluation cannot be held to less), times 4 as the project's other
    bars are."""
    assert "avg_total_bone_length_pred" not in runs["off_keys"] and "avg_total_bone_length_gt" not in runs["off_keys"]
    tr = runs["trainer"]
    images, segs, kp = tr._load_images(next(iter(tr.dataset)))
    real = tr._load_mocap(next(iter(tr.mocap_dataset)))
    tr.do_bone_evaluation = True
    try:
        r = tr.train_step(images, segs, kp, *real)
    finally:
        tr.do_bone_evaluation = False
    assert set(r) == runs["off_keys"] | {"avg_total_bone_length_pred", "avg_total_bone_length_gt"}
    fake = torch.cat([tr.engine.smpl(t, want=("joints",))["joints"] for t in r["thetas"]]).cpu().numpy()
    for key, joints in (("avg_total_bone_length_pred", fake), ("avg_total_bone_length_gt", real[0].cpu().numpy())):
        want = float(bone_sum(joints, np.float64))
        tol = 4 * max(abs(float(bone_sum(joints, np.float32)) - want), 2.0 ** -24 * abs(want))
        got = float(r[key].double().cpu())
        print("%s: got %.9g want %.9g |diff| %.3g tol %.3g" % (key, got, want, abs(got - want), tol))
        assert r[key].dim() == 0 and r[key].is_cuda and want > 0 and abs(got - want) <= tol, (key, got, want, tol)


def test_validate_checkpoint_draws_every_image(runs):
    """draw_every_image: every image of both validation batches as vis_images/<i>, at step = the batch's number"""
    tr = runs["trainer"]
    out = tr.validate_checkpoint(restore=False, draw_every_image=True)
    assert out["batches"] == 2 and np.isfinite(out["kpr_loss"])
    ev = events_of(runs["model_dir"], "checkpoint_validation")
    assert [(s, v["tag"]) for s, v in ev] == [(b, "vis_images/%d" % i) for b in (1, 2) for i in range(B)]
    assert all((v["image"]["height"], v["image"]["width"]) == (STAGES * S, 3 * S) for _, v in ev)
