"""GPU tests of hpe_amd.Trainer (run with -m gpu on an MI355X): train_step with the Keras optimiser, save / restore / resume bit for bit,
a Predictor built from the saved directory, the untouched default optimiser of the two trainers, and one short train() run.

Synthetic full-size weights, max_batch = B = 2, records written to tmp_path with tests/records_writer.py from the JPEG streams of the
golden records, fixed dropout masks, interpolation draws and augmentation draws.  The mesh reprojection term is left out
(use_mesh_repro_loss = False, the reference's default): the bit comparisons here rest on the kp loss, the critic term and the encoder /
regressor / critic gradients, whose kernels DESIGN.md states are free of atomics; the mesh gradient is tested on its own
(tests/test_gpu_mesh_loss_grad.py)."""
import os
import types

import numpy as np
import pytest
import torch

import hpe_amd
from hpe_amd import critic_spec, records, synthetic, tf_checkpoint

import records_writer as RW

pytestmark = pytest.mark.gpu
B, STAGES = 2, 3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "records")


def same(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.fixture(scope="module")
def weights():
    w = dict(synthetic.make_encoder_params())
    w.update(synthetic.make_regressor_params(variant="bounded"))
    w.update(synthetic.make_critic_params())
    return w


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """four image records (the three golden ones and the first again) and six mocap rows, as files"""
    d = tmp_path_factory.mktemp("records")
    recs = [records.parse_image_example(p) for p in records.read_tfrecords(os.path.join(GOLDEN, "images.tfrecords"))]
    recs = recs + recs[:1]
    payloads = []
    for r in recs:
        kp = r["kp"]
        payloads.append(RW.image_example(r["image"], r["seg"], r["height"], r["width"], r["center"].tolist(), r["filename"], kp[:14, 0].tolist(),
                                         kp[:14, 1].tolist(), kp[:14, 2].astype(np.int64).tolist(), kp[14:].T.reshape(-1).tolist()))
    images = str(d / "images.tfrecords")
    RW.write_tfrecords(images, payloads)
    th = synthetic.make_thetas(B * STAGES, seed=9)
    mocap = str(d / "mocap.tfrecords")
    RW.write_tfrecords(mocap, [RW.mocap_example(t[3:75].tolist(), t[75:].tolist()) for t in th])
    return images, mocap


def make_config(weights, checkpoint_dir, **kw):
    cfg = types.SimpleNamespace(batch_size=B, epoch=2, smpl_model=synthetic.make_smpl_model(), mean_params=synthetic.make_mean_params(),
                                checkpoint_dir=str(checkpoint_dir), use_validation=False, validation_step_size=2, augment_seed=5)
    if weights is not None:
        cfg.weights = weights
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def make_trainer(weights, data, checkpoint_dir, log=None, **kw):
    images, mocap = data
    ds = hpe_amd.RecordDataset(images, B)
    mo = hpe_amd.RecordDataset(mocap, B * STAGES, parse=hpe_amd.parse_mocap_example)
    val = hpe_amd.RecordDataset(images, B) if kw.get("use_validation") else None
    return hpe_amd.Trainer(make_config(weights, checkpoint_dir, **kw), ds, mo, val_dataset=val, log=log if log is not None else (lambda s: None),
                           generator=torch.Generator(device="cuda").manual_seed(1))


def tensors_of(tr):
    g = tr.generator
    return {"regressor": g.params.detach().clone(), "encoder": g.encoder_params.detach().clone(), "stats": g.encoder_stats.clone(),
            "critic": tr.critic.params.detach().clone()}


def result_tensors(r):
    out = [r["kpr_losses"][-1], r["generator_critic_losses"][-1], r["critic_network_loss"], r["critic_penalty"], r["pred_keypoints"],
           r["generated_cams"]] + list(r["thetas"])
    return [t.detach().clone() for t in out]


@pytest.fixture(scope="module")
def runs(weights, data, tmp_path_factory):
    """run A: two steps, save, a third step.  run B: a fresh engine, restore, the saved state's outputs, the third step."""
    ckpt = tmp_path_factory.mktemp("ckpt")
    out = {"dir": str(ckpt)}
    a = make_trainer(weights, data, ckpt)
    batch = next(iter(a.dataset))
    images, segs, kp = a._load_images(batch)  # one fixed batch: records -> JPEG decode -> augmentation with the seeded draws
    real = a._load_mocap(next(iter(a.mocap_dataset)))
    g = torch.Generator(device="cuda").manual_seed(3)
    drops = [a.generator.draw_masks(B) for _ in range(3)]
    N = B * STAGES
    interps = [(torch.rand((N, 14, 3), generator=g, device="cuda"), torch.rand((N, 10), generator=g, device="cuda"),
                torch.rand((N, 24, 3, 3), generator=g, device="cuda")) for _ in range(3)]
    out["inputs"] = (images, segs, kp, real, drops, interps)
    out["start"] = tensors_of(a)
    out["results"] = [a.train_step(images, segs, kp, *real, drop=drops[i], interp=interps[i]) for i in range(2)]
    out["after2"] = tensors_of(a)
    out["iterations"] = (a.generator.optimizer.iterations, a.critic.optimizer.iterations)
    out["prefix"] = a.save()
    out["saved_features"] = a.engine.encoder(images).clone()
    out["saved_predict"] = {k: v.clone() for k, v in a.predictor.predict(images).items()}
    out["third"] = result_tensors(a.train_step(images, segs, kp, *real, drop=drops[2], interp=interps[2]))
    out["after3"] = tensors_of(a)
    a.engine.close()
    b = make_trainer(weights, data, tmp_path_factory.mktemp("ckpt_b"))
    out["restored_prefix"] = b.restore(str(ckpt), verify=False)  # the checksums: tests/test_checkpoint_writer_cpu.py and the Predictor test below
    out["b_after_restore"] = tensors_of(b)
    out["b_iterations"] = (b.generator.optimizer.iterations, b.critic.optimizer.iterations, b.save_counter)
    out["b_features"] = b.engine.encoder(images).clone()
    out["b_third"] = result_tensors(b.train_step(images, segs, kp, *real, drop=drops[2], interp=interps[2]))
    out["b_after3"] = tensors_of(b)
    out["b"] = b
    yield out
    b.engine.close()


def test_two_steps_move_every_tensor_and_share_one_step_count(runs):
    for r in runs["results"]:
        assert set(r) == {"kpr_losses", "pred_keypoints", "generated_cams", "thetas", "generator_critic_losses", "critic_penalty", "critic_network_loss"}
        assert len(r["kpr_losses"]) == STAGES and len(r["generator_critic_losses"]) == STAGES and len(r["thetas"]) == STAGES
        for t in r["kpr_losses"] + r["generator_critic_losses"] + [r["critic_penalty"], r["critic_network_loss"]]:
            assert t.is_cuda and t.dim() == 0 and bool(torch.isfinite(t))
    for k in ("regressor", "encoder", "stats", "critic"):
        assert not torch.equal(runs["start"][k], runs["after2"][k]), k
    assert runs["iterations"] == (2, 2)  # one count for the encoder, the regressor and mean theta; one for the critic


def test_save_restore_resume_is_bit_exact(runs):
    assert runs["restored_prefix"] == runs["prefix"] == os.path.join(runs["dir"], "ckpt-1")
    assert runs["b_iterations"] == (2, 2, 1)
    for k, t in runs["after2"].items():  # weights and encoder statistics as saved
        assert same(runs["b_after_restore"][k], t), k
    assert same(runs["b_features"], runs["saved_features"])
    for x, y in zip(runs["third"], runs["b_third"]):  # the third step's losses, keypoints, cameras and thetas
        assert same(x, y)
    for k, t in runs["after3"].items():  # ... and every parameter tensor and the statistics after it
        assert same(runs["b_after3"][k], t), k


def test_restored_moments_are_the_saved_ones(runs):
    st = tf_checkpoint.load_training_state(runs["dir"], verify=False)
    assert st["generator_optimizer"]["iter"] == 2 and st["discriminator_optimizer"]["iter"] == 2
    assert st["generator_optimizer"]["missing"] == [] and st["discriminator_optimizer"]["missing"] == []
    assert st["generator_optimizer"]["encoder"]["v"].any() and st["generator_optimizer"]["regressor"]["m"].any()
    assert st["discriminator_optimizer"]["critic"]["m"].shape == (critic_spec.PARAM_FLOATS,)


def test_predictor_from_the_saved_directory_matches_the_training_engine(runs):
    images = runs["inputs"][0]
    p = hpe_amd.Predictor(make_config(None, runs["dir"]))
    try:
        assert p.checkpoint_info["prefix"] == runs["prefix"] and p.engine.has_critic
        assert same(p.engine.encoder(images), runs["saved_features"])
        got = p.predict(images)
        for k, v in runs["saved_predict"].items():
            assert same(got[k], v), k
    finally:
        p.engine.close()


def test_default_optimizer_is_untouched(weights):
    """optimizer="torch" and no argument at all: the same torch.optim.Adam, the same bits"""
    from oracle import hmr_oracle as O

    feats = torch.from_numpy(np.random.RandomState(2).standard_normal((B, 2048)).astype(np.float32)).cuda().abs()
    g = torch.Generator().manual_seed(4)
    kp = torch.cat([torch.rand(B, 19, 2, generator=g) * 1.2 - 0.6, torch.ones(B, 19, 1)], 2).cuda()
    th = torch.from_numpy(synthetic.make_thetas(B * STAGES, seed=9)).cuda()
    outs = []
    for kw in ({}, {"optimizer": "torch"}):
        e = hpe_amd.HpeEngine(device=0, max_batch=B)
        try:
            e.load_smpl(synthetic.make_smpl_model())
            e.load_encoder(weights)
            e.load_regressor(weights)
            e.load_mean_theta(O.load_mean_param(synthetic.make_mean_params()))
            e.finalize()
            e.load_critic(weights)
            gt = hpe_amd.GeneratorTrainer(e, generator=torch.Generator(device="cuda").manual_seed(1), **kw)
            ct = hpe_amd.CriticTrainer(e, generator=torch.Generator(device="cuda").manual_seed(2), **kw)
            assert isinstance(gt.optimizer, torch.optim.Adam) and isinstance(ct.optimizer, torch.optim.Adam)
            with pytest.raises(ValueError):
                hpe_amd.GeneratorTrainer(e, optimizer="sgd")
            with pytest.raises(ValueError):
                hpe_amd.CriticTrainer(e, optimizer="sgd")
            real = hpe_amd.mocap_real(e, th[:, 3:75].contiguous(), th[:, 75:].contiguous())
            for _ in range(2):
                r = gt.step(feats, kp)
                c = ct.step_from_thetas(real, r["thetas"])
            outs.append([gt.params.detach().cpu(), ct.params.detach().cpu(), r["kpr_losses"][-1].cpu(), c["critic_network_loss"].cpu()])
        finally:
            e.close()
    for x, y in zip(*outs):
        assert same(x, y)


def test_keras_mode_refuses_a_second_rate(runs):
    with pytest.raises(ValueError, match="encoder_lr"):
        hpe_amd.GeneratorTrainer(runs["b"].engine, lr=1e-4, train_encoder=True, encoder_lr=1e-3, encoder_bn="batch", optimizer="keras")


def test_train_two_epochs_leaves_the_scheduled_checkpoint(runs, data, tmp_path):
    """4 images, batch 2: two steps per epoch, four steps, one validation step per epoch, a checkpoint after epoch 2 (save_every = 2)"""
    b = runs["b"]
    lines = []
    b.log, b.checkpoint_dir, b.max_epoch = lines.append, str(tmp_path), 2
    b.val_dataset, b.use_validation, b.val_step_size = hpe_amd.RecordDataset(data[0], B), True, 2
    before = b.generator.optimizer.iterations
    out = b.train(save_every=2)
    assert out == {"steps": 4, "epochs": 2, "saved": [2], "validations": 2}
    assert b.generator.optimizer.iterations == before + 4
    assert sorted(os.listdir(str(tmp_path))) == ["checkpoint", "ckpt-2.data-00000-of-00001", "ckpt-2.index"]  # the counter went on from the restored 1
    assert tf_checkpoint.latest_checkpoint(str(tmp_path)) == os.path.join(str(tmp_path), "ckpt-2")
    finished = [l for l in lines if l.startswith("Finished epoch")]
    assert len(finished) == 2 and finished[0].startswith("Finished epoch 0, average losses: kpr=") and " gc=" in finished[0] and " cn=" in finished[0]
    assert " Validation: kpr=" in finished[0] and "nan" not in finished[0] and "nan" not in finished[1]
    assert lines[0] == "started training" and lines[-1].startswith("Finish training on")
    v = b.validate_checkpoint(restore=False)  # one pass over the validation records with the live weights
    assert v["batches"] == 2 and np.isfinite(v["kpr_loss"]) and v["kpr_loss"] > 0 and v["mr_loss"] is None
