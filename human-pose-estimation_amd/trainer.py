"""Trainer -- the reference's training driver (src/trainer.py:40-870): ``train_step`` is
``GeneratorTrainer.step`` (encoder with batch statistics, IEF loop, losses, gradient, update) followed by
``CriticTrainer.step_from_thetas``, both with the reference's optimiser (``KerasAdam``: one for the encoder, the regressor and mean theta,
one for the critic); ``train`` is the reference's loop; ``save`` / ``restore`` write and read the reference's ``tf.train.Checkpoint``
layout (tf_checkpoint.save_checkpoint / load_training_state), optimiser moments and step counts included, so a run resumes with the bits
of one that was never interrupted.

Summaries (DESIGN.md "Training summaries"): with ``config.model_dir`` set and ``config.write_summaries`` (default True), ``train`` writes
the reference's TensorBoard scalars at every step -- a training writer under ``<model_dir>/training``, a validation writer under
``<model_dir>/validation`` (the reference concatenates ``model_dir + 'training'`` without a separator) -- and, every
``config.log_img_step`` steps, the ``draw_results`` panels of the rows ``show_these`` as ``vis_images/<i>`` (summary.py, draw.py,
png_encode.py).  Scalars stay on the device between flushes; a writer is flushed at image steps and when the epoch rolls.  The
bone-length evaluation runs with ``config.do_bone_evaluation`` (default False here so that the result keys stay as they were; the
reference's default is True).

Data-parallel (DESIGN.md "Data-parallel training"): under ``torchrun`` -- a process group is initialised, or ``config.distributed`` asks
for ``distributed.init_from_env`` -- every rank builds the same Trainer on the device ``LOCAL_RANK``.  ``config.batch_size`` stays the
GLOBAL batch G; rank r steps on its ``shard_bounds(G, r, world)`` rows (datasets built with ``RecordDataset(..., shard=(rank, world))``),
BatchNorm statistics and gradients are those of the G rows, the replicas start from rank 0's tensors and stay bit-identical; only
rank 0 saves, summarises and logs.

Guarded optimiser step (DESIGN.md "Guarded optimiser step"; the reference has no gradient clipping, src/trainer.py:84):
``config.generator_clipnorm`` / ``config.critic_clipnorm`` (default None) clip each update's global gradient norm,
``config.skip_nonfinite_steps`` (default False) undoes an update whose gradient holds a NaN or an infinity, ``config.log_grad_norms``
(default False) adds one ``grad_norm/<layer>`` scalar per conv and dense layer.  With any of them set and summaries on, every step also
writes ``optim/<generator|critic>_grad_norm``, ``_clip_scale`` and ``_skipped_steps``, and ``train_step``'s result has them as
``<generator|critic>_grad_norm`` ... (device scalars) and ``layer_grad_norms``.  With none set nothing changes.

Scores (DESIGN.md "Checkpoint scores"): ``score_checkpoint`` gives PCK and the silhouette's IoU / foreground-background accuracy / F1 over
one pass of the validation set, with the best and worst images drawn on request; ``config.score_validation`` (default False) adds four
``metrics/...`` scalars of the batch to every validation step of ``train``.

Not here: ``draw_text`` on the panels.
``generated_verts`` is not among ``train_step``'s result keys: drawing recomputes the vertices of the rows it shows from ``thetas``.
``use_kpr_loss`` decides, as in the reference, only whether the keypoint loss is logged: it is always minimised."""
from __future__ import annotations

import datetime
import os
import time

import numpy as np

from . import critic_spec, regressor_spec, resnet_spec, tf_checkpoint
from .critic_train import CRITIC_LR, CriticTrainer
from .generator_train import GENERATOR_LR, GeneratorTrainer

SAVE_EVERY = 5  # epochs (src/trainer.py:835)
BONE_ENDS = (1, 2, 8, 9, 3, 4, 7, 8, 12, 12, 9, 10, 13)  # precompute_C_matrix (src/models.py:97-112): bone k = joint k - joint BONE_ENDS[k]


def total_bone_length(joints):
    """``reduce_mean(reduce_sum(diag_part(get_kcs(joints, C)), axis=1))`` (src/trainer.py:610-617): the KCS diagonal is the squared
    length of each of the 13 bones B = X C of the first 14 joints; summed over the bones, averaged over the rows.  joints [N, >=14, 3]
    -> a 0-dim float32 tensor.  Plain torch: C has one +1 and one -1 per column, so X C is a difference of two joints; squares and sums
    run in float64 (a few hundred terms, not a hot path) and the result is rounded to float32 once."""
    j = joints[:, :14].double()
    b = j[:, :13] - j[:, list(BONE_ENDS)]
    return (b * b).sum(dim=2).sum(dim=1).mean().float()


def show_rows(batch_size):
    """``show_these`` (src/trainer.py:116-121): half of min(6, batch) rows from the front and three from the back.  Below a batch of
    three the reference's list leaves the batch (tf.gather fails there); such rows are dropped here."""
    num2show = min(6, batch_size)
    rows = np.hstack([np.arange(num2show / 2), batch_size - np.arange(3) - 1]).astype(np.int64)
    return [int(r) for r in rows if 0 <= r < batch_size]


def run_training_loop(batches, train_step, num_images, batch_size, max_epoch, val_step=None, validation_step_size=0, save=None,
                      save_every=SAVE_EVERY, summarize=None, log=print, after_train_step=None, after_val_step=None, after_epoch=None):
    """The bookkeeping of the reference's loop (src/trainer.py:715-868), free of any engine.  batches: an iterable of
    (generator batch, critic batch, validation batch) that normally never ends; train_step(generator batch, critic batch) -> result;
    val_step(validation batch) -> result, called after every ``validation_step_size``-th step when given; save(epoch) when the finished
    epoch count is a multiple of ``save_every``; summarize(epoch, train results, validation results) -> the text of the epoch's line.
    ``num_itr_per_epoch = max(num_images / batch_size, 1)`` is NOT rounded: the epoch rolls at the first step count that reaches it.
    after_train_step(step, result) is called after every train step with the 1-based step count, after_val_step(step, result) after
    every validation step (the places the reference writes its summaries, src/trainer.py:745-809), after_epoch(epoch) when an epoch
    rolls, before its line is logged; all default to None.
    Stops after ``max_epoch`` epochs (or when ``batches`` ends).  -> {"steps", "epochs", "saved": [epochs], "validations"}"""
    num_itr_per_epoch = max(float(num_images) / float(batch_size), 1.0)
    step = itr = epoch = validations = 0
    saved, train_results, val_results = [], [], []
    log("Starting epoch 0")
    start_time = time.time()
    if max_epoch <= 0:
        return {"steps": 0, "epochs": 0, "saved": saved, "validations": 0}
    for gen_batch, critic_batch, val_batch in batches:
        if itr == 0:
            start_time = time.time()
        train_results.append(train_step(gen_batch, critic_batch))
        step += 1
        if after_train_step is not None:
            after_train_step(step, train_results[-1])
        if val_step is not None and validation_step_size > 0 and step % validation_step_size == 0:
            val_results.append(val_step(val_batch))
            validations += 1
            if after_val_step is not None:
                after_val_step(step, val_results[-1])
        itr += 1
        if itr >= num_itr_per_epoch:
            end_time = time.time()
            itr = 0
            epoch += 1
            if save is not None and epoch % save_every == 0:
                save(epoch)
                saved.append(epoch)
            if after_epoch is not None:
                after_epoch(epoch - 1)
            log(summarize(epoch - 1, train_results, val_results) if summarize is not None else "Finished epoch %d" % (epoch - 1))
            train_results, val_results = [], []
            if epoch >= max_epoch:
                break
            log("Starting epoch {}, approx finished in {:04.2f} min".format(epoch, (max_epoch - epoch) * (end_time - start_time) / 60.0))
    return {"steps": step, "epochs": epoch, "saved": saved, "validations": validations}


def rank_zero_only(rank, barrier=None, save=None, log=print, **hooks):
    """The loop's side effects for rank ``rank`` of a data-parallel run, free of any engine: ``save`` runs on rank 0 only and EVERY rank
    then waits at ``barrier()`` (nobody runs ahead of a checkpoint that is being written); the summary hooks (after_train_step,
    after_val_step, after_epoch) and the log exist on rank 0 only.  -> the keyword arguments of ``run_training_loop`` for this rank"""
    out = {"log": log if rank == 0 else (lambda *a, **k: None)}
    if save is not None:
        def save_all(epoch):
            if rank == 0:
                save(epoch)
            if barrier is not None:
                barrier()

        out["save"] = save_all
    if rank == 0:
        out.update({k: v for k, v in hooks.items() if v is not None})
    return out


SCORE_TAGS = ("iou", "fb_f1", "pck_torso_0.2", "pckh_0.5")  # what config.score_validation writes as metrics/<tag>


class BestWorst(object):
    """The ``n`` lowest and ``n`` highest of a stream of (value, record number), ties broken by record order (the earlier record ranks
    first in both lists); NaN values are not ranked."""

    def __init__(self, n):
        self.n, self.low, self.high = int(n), [], []

    def add(self, value, record):
        value = float(value)
        if value != value:
            return
        self.low = sorted(self.low + [(value, record)])[:self.n]
        self.high = sorted(self.high + [(-value, record)])[:self.n]

    def records(self):
        return {r for _v, r in self.low + self.high}


def _repeat(dataset):
    """batches of an iterable dataset, over and over (the reference's ``.repeat()``)"""
    while True:
        empty = True
        for batch in dataset:
            empty = False
            yield batch
        if empty:
            raise ValueError("a dataset yields no batch (fewer records than one batch?)")


class Trainer(object):
    def __init__(self, config, dataset, mocap_dataset, val_dataset=None, validation_only=False, log=print, generator=None,
                 **predictor_args):
        """config: read by attribute like the reference's -- ``batch_size``, ``epoch``, ``generator_lr``, ``critic_lr``,
        ``kpr_loss_weight``, ``mr_loss_weight``, ``critic_loss_weight``, ``use_kpr_loss``, ``use_mesh_repro_loss``, ``encoder_only``,
        ``use_validation``, ``validation_step_size``, ``train_from_checkpoint``, ``checkpoint_dir``, ``encoder_precision`` ("fp32", the
        default, or "mixed": the encoder's walks in bf16 with fp32 master weights, BatchNorm arithmetic in fp32; checkpoints are the
        same either way), ``joints3d_loss_weight`` and ``smpl_loss_weight`` (both 0 by default: no 3-D supervision; above 0 the records'
        ``gt3d`` / ``pose`` / ``shape`` are trained on, DESIGN.md "3-D supervision"), plus what ``Predictor`` reads (the
        SMPL model, the mean parameters and the starting weights: ``predictor_args`` are passed on).  dataset / val_dataset:
        ``RecordDataset``s of image records (batch size ``config.batch_size``) or any iterable of what ``load_training_batch`` takes: the
        reference's image records, whose ``image/encoded`` and ``image/seg_gt`` are JPEG or PNG streams (lsp_train / lsp_val masks and
        mpii frames are PNG, lsp_ext and mpii masks JPEG; one batch may mix them);
        mocap_dataset: a ``RecordDataset(..., parse=parse_mocap_example)`` of ``batch_size * num_stage`` rows or any iterable of lists
        of (pose [72], shape [10]).  ``config.num_images`` (default: counted once from the dataset) sets the epoch length.  generator:
        the torch.Generator (CUDA) of the dropout and interpolation draws; the augmentation draws come from ``config.augment_seed``.
        validation_only: no trainers are built (``validate_checkpoint`` / ``val_step`` only).
        Data-parallel: see the module's text; ``config.seed`` (default 0) + rank seeds the dropout and interpolation draws where no
        generator is given, ``config.augment_seed`` + rank the augmentation; ``config.dist_backend`` / ``config.dist_timeout_s`` go to
        ``Reducer.from_env``."""
        import torch

        from . import distributed as D
        from .predictor import Predictor

        g = lambda name, default: getattr(config, name, default)  # noqa: E731
        self.config, self.log = config, log
        self.reducer, self.rank, self.world, self.sharded = None, 0, 1, None
        dist = D._dist()
        if bool(g("distributed", False)) and not (dist.is_available() and dist.is_initialized()):
            D.init_from_env(g("dist_backend", None), timeout=datetime.timedelta(seconds=float(g("dist_timeout_s", D.DEFAULT_TIMEOUT_S))))
        if dist.is_available() and dist.is_initialized():
            local = int(os.environ.get("LOCAL_RANK", "0"))
            torch.cuda.set_device(local)
            predictor_args.setdefault("device", local)
            red = D.Reducer(device=torch.device("cuda", local))
            if red.active:
                self.reducer, self.rank, self.world = red, red.rank, red.world
                if self.rank != 0:
                    self.log = lambda *a, **k: None
        self.batch_size, self.max_epoch = int(g("batch_size", 8)), int(g("epoch", 125))
        self.generator_lr, self.critic_lr = float(g("generator_lr", GENERATOR_LR)), float(g("critic_lr", CRITIC_LR))
        self.kpr_loss_weight, self.mr_loss_weight = float(g("kpr_loss_weight", 60.0)), float(g("mr_loss_weight", 0.001))
        self.critic_loss_weight = float(g("critic_loss_weight", 0.01))
        # 3-D supervision (DESIGN.md "3-D supervision"): off by default; above 0 the records' gt3d / pose / shape are loaded and trained on
        self.joints3d_loss_weight, self.smpl_loss_weight = float(g("joints3d_loss_weight", 0.0)), float(g("smpl_loss_weight", 0.0))
        self.use_3d_loss = self.joints3d_loss_weight > 0.0 or self.smpl_loss_weight > 0.0
        self.use_kpr_loss, self.use_mesh_repro_loss = bool(g("use_kpr_loss", True)), bool(g("use_mesh_repro_loss", False))
        self.encoder_only, self.use_validation = bool(g("encoder_only", False)), bool(g("use_validation", True))
        self.val_step_size = int(g("validation_step_size", 50))
        self.train_from_checkpoint, self.checkpoint_dir = bool(g("train_from_checkpoint", False)), g("checkpoint_dir", None)
        self.model_dir = g("model_dir", None)
        self.write_summaries = self.model_dir is not None and bool(g("write_summaries", True)) and self.rank == 0
        self.log_img_step, self.do_bone_evaluation = int(g("log_img_step", 1000)), bool(g("do_bone_evaluation", False))
        self.score_validation = bool(g("score_validation", False))
        lo, hi = D.shard_bounds(self.batch_size, self.rank, self.world)
        self.local_batch = hi - lo  # this rank's rows of a step; rank 0 has the largest shard
        if self.local_batch < 1:
            raise ValueError("batch_size %d leaves rank %d of %d without a row" % (self.batch_size, self.rank, self.world))
        self.show_these = show_rows(self.local_batch)
        self.training_writer = self.val_writer = None
        self.dataset, self.mocap_dataset, self.val_dataset = dataset, mocap_dataset, val_dataset
        self.use_validation = self.use_validation and val_dataset is not None
        self.predictor = Predictor(config, **predictor_args)
        self.engine = eng = self.predictor.engine
        self.num_stage = self.predictor.num_stage
        self.inital_theta = np.asarray(self.predictor.load_mean_param(), np.float32).reshape(1, 85)  # the reference's untrained theta_prev
        self.save_counter = 0
        self._aug = torch.Generator().manual_seed(int(g("augment_seed", 0)) + self.rank)
        self.generator = self.critic = None
        if self.reducer is not None:
            self.sharded = D.ShardedPredictor(self.predictor)
            if generator is None:  # every rank its own draws
                generator = torch.Generator(device=eng.tdev).manual_seed(int(g("seed", 0)) + self.rank)
        if validation_only:
            return
        if not self.encoder_only and not eng.has_critic:
            raise RuntimeError("Trainer needs critic weights to start from (critic_params=, config.critic_params, critic/... keys of the "
                               "weights, or a checkpoint with a discriminator) unless config.encoder_only is set")
        dp = {} if self.reducer is None else {"reducer": self.reducer}
        dp_gen = dict(dp, global_batch=self.batch_size) if dp else {}
        self.encoder_precision = g("encoder_precision", "fp32")
        if self.encoder_precision not in ("fp32", "mixed"):
            raise ValueError("config.encoder_precision must be 'fp32' or 'mixed', got %r" % (self.encoder_precision,))
        eng.reserve_encoder_train(D.shard_bounds(self.batch_size, 0, self.world)[1], batch_norm=True,
                                  precision=self.encoder_precision)  # the largest shard
        # the guarded optimiser step (DESIGN.md "Guarded optimiser step"): off unless one of these four is set
        self.generator_clipnorm, self.critic_clipnorm = g("generator_clipnorm", None), g("critic_clipnorm", None)
        self.skip_nonfinite_steps, self.log_grad_norms = bool(g("skip_nonfinite_steps", False)), bool(g("log_grad_norms", False))

        def guard(clipnorm):  # the per-layer norms come from the guard's statistics: logging alone is a guard that never clips
            clipnorm = float("inf") if clipnorm is None and self.log_grad_norms else clipnorm
            return {} if clipnorm is None and not self.skip_nonfinite_steps else {"clipnorm": clipnorm, "skip_nonfinite": self.skip_nonfinite_steps}

        self.generator = GeneratorTrainer(eng, lr=self.generator_lr, kpr_loss_weight=self.kpr_loss_weight, mr_loss_weight=self.mr_loss_weight,
                                          critic_loss_weight=self.critic_loss_weight, generator=generator, train_encoder=True,
                                          encoder_bn="batch", optimizer="keras", encoder_precision=self.encoder_precision,
                                          joints3d_loss_weight=self.joints3d_loss_weight, smpl_loss_weight=self.smpl_loss_weight, **dp_gen,
                                          **guard(self.generator_clipnorm))
        if not self.encoder_only:
            self.critic = CriticTrainer(eng, lr=self.critic_lr, generator=generator, optimizer="keras", **dp, **guard(self.critic_clipnorm))
        self._layer_maps = {}
        self._sync_replicas()

    def _sync_replicas(self):
        """data-parallel: rank 0's flat tensors, moving statistics and optimiser state into every rank, and into the engines"""
        import torch

        red = self.reducer
        if red is None or self.generator is None:
            return
        gen, eng = self.generator, self.engine
        opts = [gen.optimizer] + ([self.critic.optimizer] if self.critic is not None else [])
        with torch.no_grad():
            for t in (gen.params, gen.encoder_params, gen.encoder_stats) + ((self.critic.params,) if self.critic is not None else ()):
                red.broadcast(t.detach())
            for opt in opts:
                for slot in opt.slots.values():
                    red.broadcast(slot["m"])
                    red.broadcast(slot["v"])
                red.broadcast(opt._ensure_state(gen.params))
        eng.set_regressor_params(gen.params)
        eng.set_encoder_params_dev(gen.encoder_params)
        eng.set_encoder_stats_dev(gen.encoder_stats)
        if self.critic is not None:
            eng.set_critic_params(self.critic.params)

    def _guard_results(self, who, trainer, kinds, result):
        """the guard's figures of ``trainer``'s last step into ``result`` as copies on the device: <who>_grad_norm, <who>_clip_scale,
        <who>_skipped_steps and, with ``log_grad_norms``, layer_grad_norms[layer] = sqrt(sum of the sums of squares of the layer's segments)"""
        import torch

        from .optim import layer_segments

        opt = trainer.optimizer
        result[who + "_grad_norm"], result[who + "_step_applied"] = opt.grad_norm.clone(), opt.step_applied.clone()
        result[who + "_clip_scale"], result[who + "_skipped_steps"] = opt.clip_scale.clone(), opt._guard_view("skipped").clone()
        if not self.log_grad_norms:
            return
        norms = result.setdefault("layer_grad_norms", {})
        for kind in kinds:
            if kind not in self._layer_maps:  # [layers, segments] of 0 / 1: which segments make up which layer
                names = layer_segments(kind, self.engine.lib)[1]
                layers = list(dict.fromkeys(names))
                m = torch.zeros((len(layers), len(names)), dtype=torch.float64)
                for j, n in enumerate(names):
                    m[layers.index(n), j] = 1.0
                self._layer_maps[kind] = (layers, m.to(self.engine.tdev))
            layers, m = self._layer_maps[kind]
            per_layer = (m * opt.grad_stats(kind)[:, 0]).sum(1).sqrt()
            for i, n in enumerate(layers):
                norms[n] = per_layer[i]

    # ------------------------------------------------------------------ steps
    def train_step(self, images, seg_gts, kp_gt, joints=None, shapes=None, Rs=None, drop="draw", interp=None, gt3d=None):
        """One update of the generator, then one of the critic on the thetas it produced (src/trainer.py:383-583).  images
        [B,224,224,3], seg_gts [B,224,224(,1)], kp_gt [B,19,3]; joints / shapes / Rs: the real triple of ``mocap_real`` (B * num_stage
        or B rows), unused with ``encoder_only``.  drop / interp: fixed dropout multipliers and interpolation draws (tests).  gt3d: the
        batch's ``ops.Gt3D``; with a 3-D weight above 0 the result gains joints3d_losses and smpl_param_losses.
        -> the reference's result keys: kpr_losses, mr_losses (with ``use_mesh_repro_loss``), pred_keypoints, generated_cams and, unless
        ``encoder_only``, generator_critic_losses, critic_penalty, critic_network_loss; plus ``thetas``; with ``do_bone_evaluation``
        also avg_total_bone_length_pred (all stages' joints) and avg_total_bone_length_gt (``joints``).  Nothing reads the device."""
        if self.generator is None:
            raise RuntimeError("this Trainer was built with validation_only")
        r = self.generator.step(images, kp_gt, seg_gts if self.use_mesh_repro_loss else None, use_critic=not self.encoder_only, drop=drop,
                                gt3d=gt3d if self.use_3d_loss else None)
        result = {"kpr_losses": r["kpr_losses"], "pred_keypoints": r["pred_keypoints"], "generated_cams": r["generated_cams"],
                  "thetas": r["thetas"]}
        if self.use_mesh_repro_loss:
            result["mr_losses"] = r["mr_losses"]
        if "joints3d_losses" in r:
            result["joints3d_losses"], result["smpl_param_losses"] = r["joints3d_losses"], r["smpl_param_losses"]
        if self.generator.guarded:
            self._guard_results("generator", self.generator, ("regressor", "encoder"), result)
        if not self.encoder_only:
            c = self.critic.step_from_thetas((joints, shapes, Rs), r["thetas"], interp=interp,
                                             global_batch=self.batch_size if self.reducer is not None else None)
            if self.critic.guarded:
                self._guard_results("critic", self.critic, ("critic",), result)
            result["generator_critic_losses"] = r["generator_critic_losses"]
            result["critic_penalty"], result["critic_network_loss"] = c["critic_penalty"], c["critic_network_loss"]
        if self.do_bone_evaluation:
            import torch

            if joints is None:
                raise ValueError("do_bone_evaluation needs the mocap joints")
            fake = torch.cat([self.engine.smpl(t, want=("joints",))["joints"] for t in r["thetas"]])
            result["avg_total_bone_length_pred"] = total_bone_length(fake)
            result["avg_total_bone_length_gt"] = total_bone_length(joints)
        return result

    def val_step(self, images, seg_gts, kp2d_gts, gt3d=None):
        """data-parallel: this rank's rows (the validation dataset is sharded like the training one), the losses those of all ranks.
        gt3d: the batch's ``ops.Gt3D``; with a 3-D weight above 0 the result gains the weighted joints3d_losses and smpl_param_losses
        of the last stage (lists of one), from one hpe_loss3d launch on a forward of its own."""
        kw = dict(use_mesh_repro_loss=self.use_mesh_repro_loss, kpr_loss_weight=self.kpr_loss_weight, mr_loss_weight=self.mr_loss_weight)
        if self.sharded is not None:
            r = self.sharded.val_step(images, seg_gts, kp2d_gts, presharded=True, **kw)
        else:
            r = self.predictor.val_step(images, seg_gts, kp2d_gts, **kw)
        if gt3d is not None and self.use_3d_loss:
            r["joints3d_losses"], r["smpl_param_losses"] = self._val_losses_3d(images, gt3d)
        return r

    def _val_losses_3d(self, images, gt3d):
        """the weighted 3-D terms of the last stage's prediction for ``images`` against gt3d -> ([joints3d_loss], [smpl_param_loss]), each
        empty where its weight is 0; data-parallel: the terms of all ranks, numerators and counts summed in one collective before the
        division"""
        import torch

        from .engine import loss3d_parts

        with torch.no_grad():
            o = self.engine.forward(images, all_stages=False, want=("joints", "theta", "Rs"))[0]
        parts = loss3d_parts(o["joints"], o["theta"][:, 75:], o["Rs"], gt3d)[0].clone()
        if self.reducer is not None:
            parts = self.reducer.sum_block(parts)
        den = torch.clamp(parts[3:5], min=1.0)  # a count of 0 has a numerator of 0
        lj, ls = 0.5 * parts[0] / den[0], 0.5 * (parts[1] + parts[2]) / den[1]
        return ([self.joints3d_loss_weight * lj] if self.joints3d_loss_weight > 0.0 else [],
                [self.smpl_loss_weight * ls] if self.smpl_loss_weight > 0.0 else [])

    # ------------------------------------------------------------------ data
    def _load_images(self, records, augment=True, with_3d=False):
        """-> (images, seg_gts, kp_gt); with_3d (the steps of ``train``, and only with a 3-D weight above 0): a fourth element, the
        batch's ``ops.Gt3D`` from ``load_training_batch_3d`` (None for a ready triple, which carries none)"""
        from .augment import draw_augmentation
        from .records import load_training_batch, load_training_batch_3d

        with_3d = with_3d and self.use_3d_loss
        if isinstance(records, (tuple, list)) and len(records) in (3, 4) and hasattr(records[0], "is_cuda"):
            ready = tuple(records)  # an (images, seg_gts, kp_gt[, gt3d]) tuple, ready
            return ready[:3] + ((ready[3] if len(ready) == 4 else None,) if with_3d else ())
        load = (lambda recs, **kw: load_training_batch_3d(recs, self.engine, **kw)) if with_3d else load_training_batch
        if augment:
            return load(records, generator=self._aug)
        draws = draw_augmentation(len(records), trans_max=0, scale_range=(1.0, 1.0))  # validation: centre crop, no jitter, no flip
        draws["flip"][:] = False
        return load(records, draws=draws)

    def _load_mocap(self, rows):
        import torch

        from .augment import mocap_real

        if isinstance(rows, (tuple, list)) and len(rows) == 3 and hasattr(rows[0], "is_cuda"):
            return rows
        poses = torch.from_numpy(np.stack([np.asarray(p, np.float32) for p, _s in rows])).to(self.engine.tdev)
        shapes = torch.from_numpy(np.stack([np.asarray(s, np.float32) for _p, s in rows])).to(self.engine.tdev)
        return mocap_real(self.engine, poses, shapes)

    def _num_images(self):
        n = getattr(self.config, "num_images", None)
        if n is not None:
            return int(n)
        if hasattr(self.dataset, "paths"):
            from .records import read_tfrecords

            return sum(1 for _ in read_tfrecords(self.dataset.paths, False))
        return len(self.dataset) * self.batch_size

    def _batches(self):
        gen = _repeat(self.dataset)
        moc = _repeat(self.mocap_dataset) if not self.encoder_only or self.do_bone_evaluation else None
        val = _repeat(self.val_dataset) if self.use_validation else None
        while True:
            yield next(gen), (next(moc) if moc is not None else None), (next(val) if val is not None else None)

    # ------------------------------------------------------------------ the loop
    def _summarize(self, epoch, train_results, val_results):
        """the reference's line (src/trainer.py:838-852); every device scalar of the epoch is read here, in one transfer"""
        import torch

        cols = []
        if self.use_kpr_loss:
            cols.append(("kpr", "{:04.2f}", [r["kpr_losses"][-1] for r in train_results]))
        if self.use_mesh_repro_loss:
            cols.append(("mr", "{:05.2f}", [r["mr_losses"][-1] for r in train_results]))
        for name, key in (("j3d", "joints3d_losses"), ("smpl", "smpl_param_losses")):  # only with the 3-D terms on
            if any(r.get(key) for r in train_results):
                cols.append((name, "{:06.4f}", [r[key][-1] for r in train_results if r.get(key)]))
        if not self.encoder_only:
            cols.append(("gc", "{:05.2f}", [r["generator_critic_losses"][-1] for r in train_results]))
            cols.append(("cn", "{:05.2f}", [r["critic_network_loss"] for r in train_results]))
        n_train = len(cols)
        if self.use_validation:
            if self.use_kpr_loss:
                cols.append(("kpr", "{:04.2f}", [r["kpr_losses"][-1] for r in val_results]))
            if self.use_mesh_repro_loss:
                cols.append(("mr", "{:05.2f}", [r["mr_losses"][-1] for r in val_results]))
        flat = [t.reshape(()).float() for _n, _f, ts in cols for t in ts]
        host = torch.stack(flat).cpu().numpy() if flat else np.zeros(0, np.float32)
        text, pos = "Finished epoch {}, average losses:".format(epoch), 0
        for i, (name, fmt, ts) in enumerate(cols):
            if i == n_train:
                text += " Validation:"
            mean = float(np.mean(host[pos:pos + len(ts)])) if ts else float("nan")  # no validation step in this epoch: nan, as np.mean([])
            pos += len(ts)
            text += (" %s=" % name) + fmt.format(mean)
        if self.use_validation and n_train == len(cols):
            text += " Validation:"
        return text

    # ------------------------------------------------------------------ summaries
    def draw_rows(self, images, segs, kp_gt, rows, thetas=None, val_result=None):
        """``draw_results`` (src/trainer.py:656-695) for the given rows of a batch -> list of PNG streams, one panel [T*S, 3*S, 3] per
        row.  thetas: the stages' theta [B,85] of a train step -- vertices and keypoints of the rows come from ``engine.smpl`` --, or
        val_result: a ``val_step`` result, which carries them.  Waits for the device (the PNG streams are host bytes)."""
        import torch

        from .draw import draw_results
        from .png_encode import encode_png_batch

        idx = torch.as_tensor(list(rows), dtype=torch.long, device=images.device)
        n = int(idx.numel())
        if thetas is not None:
            th = torch.stack([t.detach()[idx] for t in thetas], 1)  # [n,T,85]
            T, flat, mb = int(th.shape[1]), th.reshape(-1, 85).contiguous(), self.engine.max_batch
            outs = [self.engine.smpl(flat[lo:lo + mb].contiguous(), want=("verts", "kp2d")) for lo in range(0, flat.shape[0], mb)]
            verts = torch.cat([o["verts"] for o in outs]).reshape(n, T, -1, 3)
            kps = torch.cat([o["kp2d"] for o in outs]).reshape(n, T, 19, 2)
            cams = th[:, :, :3]
        else:
            verts, kps, cams = val_result["generated_verts"][idx], val_result["pred_keypoints"][idx], val_result["generated_cams"][idx]
        panels = draw_results(self.predictor.renderer, images[idx], segs[idx], kp_gt[idx], verts, kps, cams)
        return encode_png_batch(panels)

    def _open_writers(self):
        from .summary import SummaryWriter

        if self.log_img_step > 0:
            self.predictor.renderer  # noqa: B018  the panels need the SMPL faces: fail before the first step, not at step log_img_step
        self.training_writer = SummaryWriter(os.path.join(self.model_dir, "training"))
        self.val_writer = SummaryWriter(os.path.join(self.model_dir, "validation")) if self.use_validation else None

    def _write_images(self, writer, step, batch, **source):
        for i, png in enumerate(self.draw_rows(*batch, self.show_these, **source)):
            writer.image("vis_images/%d" % i, png, step)

    def _summarize_train_step(self, step, result, batch):
        """the training writer's block of the reference's loop (src/trainer.py:747-783), same tags, same conditions, same order"""
        w = self.training_writer
        if self.use_kpr_loss:
            w.scalar("generator/kpr_loss", result["kpr_losses"][-1], step)
        if self.use_mesh_repro_loss:
            w.scalar("generator/mr_loss", result["mr_losses"][-1], step)
        self._summarize_3d(w, step, result)
        if self.do_bone_evaluation:
            w.scalar("bones/avg_total_bone_lenth_pred", result["avg_total_bone_length_pred"], step)  # the reference's spelling
            w.scalar("bones/avg_total_bone_lenth_gt", result["avg_total_bone_length_gt"], step)
        image_step = self.log_img_step > 0 and step % self.log_img_step == 0
        if image_step:
            self._write_images(w, step, batch, thetas=result["thetas"])
        if not self.encoder_only:
            w.scalar("critic/critic_network_loss", result["critic_network_loss"], step)
            w.scalar("critic/generator_critic_loss", result["generator_critic_losses"][-1], step)
            w.scalar("critic/penalty", result["critic_penalty"], step)
        for who in ("generator", "critic"):  # the guarded optimiser step: not the reference's tags, and only with a guard configured
            if who + "_grad_norm" in result:
                for what in ("grad_norm", "clip_scale", "skipped_steps"):
                    w.scalar("optim/%s_%s" % (who, what), result["%s_%s" % (who, what)], step)
        for layer, norm in result.get("layer_grad_norms", {}).items():
            w.scalar("grad_norm/" + layer, norm, step)
        if image_step:
            w.flush()

    @staticmethod
    def _summarize_3d(w, step, result):
        """the 3-D supervision terms (not the reference's tags), where the step computed them"""
        for tag, key in (("generator/joints3d_loss", "joints3d_losses"), ("generator/smpl_param_loss", "smpl_param_losses")):
            if result.get(key):
                w.scalar(tag, result[key][-1], step)

    def _summarize_val_step(self, step, result, batch):
        """the validation writer's block (src/trainer.py:798-812)"""
        w = self.val_writer
        if self.use_kpr_loss:
            w.scalar("generator/kpr_loss", result["kpr_losses"][-1], step)
        if self.use_mesh_repro_loss:
            w.scalar("generator/mr_loss", result["mr_losses"][-1], step)
        self._summarize_3d(w, step, result)
        if self.score_validation:
            for tag in SCORE_TAGS:
                w.scalar("metrics/" + tag, result["scores"][tag], step)
        if self.log_img_step > 0 and step % self.log_img_step == 0:
            self._write_images(w, step, batch, val_result=result)
            w.flush()

    def _flush_writers(self):
        for w in (self.training_writer, self.val_writer):
            if w is not None:
                w.flush()

    def train(self, save_every=SAVE_EVERY):
        """the reference's ``train()``: restore when ``train_from_checkpoint``, then epochs of ``num_images / batch_size`` steps with a
        validation step every ``validation_step_size``, a checkpoint every ``save_every`` epochs and one line per epoch -> the loop's
        counts"""
        if self.generator is None:
            raise RuntimeError("this Trainer was built with validation_only")
        self.log("started training")
        if self.train_from_checkpoint:
            self.log("restore checkpoint")
            self.restore()
            self.log("checkpoint restored")
        self.log("Loading Data")

        last = {}  # the loaded batches of the step in flight: what an image step draws over

        def step(gen_batch, critic_batch):
            images, segs, kp, *gt3d = self._load_images(gen_batch, with_3d=True)
            last["train"] = images, segs, kp
            real = self._load_mocap(critic_batch) if not self.encoder_only or self.do_bone_evaluation else (None, None, None)
            return self.train_step(images, segs, kp, *real, gt3d=gt3d[0] if gt3d else None)

        def val(val_batch):
            images, segs, kp, *gt3d = self._load_images(val_batch, augment=False, with_3d=True)
            last["val"] = images, segs, kp
            r = self.val_step(images, segs, kp, gt3d=gt3d[0] if gt3d else None)
            if self.score_validation:  # on every rank: the sums cross the ranks
                r["scores"] = self.score_val_result(r, last["val"][1], last["val"][2])
            return r

        hooks = {}
        if self.score_validation and self.use_validation:
            self.predictor.score_faces()  # fail before the first step, not at the first validation step
        if self.write_summaries:
            self._open_writers()
            hooks = {"after_train_step": lambda s, r: self._summarize_train_step(s, r, last["train"]),
                     "after_val_step": lambda s, r: self._summarize_val_step(s, r, last["val"]),
                     "after_epoch": lambda epoch: self._flush_writers()}
        side = dict(hooks, save=lambda epoch: self.save(), log=self.log)
        if self.reducer is not None:
            side = rank_zero_only(self.rank, barrier=self.reducer.barrier, **side)
        try:
            out = run_training_loop(self._batches(), step, self._num_images(), self.batch_size, self.max_epoch,
                                    val_step=val if self.use_validation else None, validation_step_size=self.val_step_size,
                                    save_every=save_every, summarize=self._summarize, **side)
        finally:
            for w in (self.training_writer, self.val_writer):
                if w is not None:
                    w.close()
            self.training_writer = self.val_writer = None
        self.log("Finish training on %s" % self.model_dir)
        return out

    def validate_checkpoint(self, restore=True, draw_every_image=False):
        """the mean keypoint and mesh reprojection losses (last stage, weighted) of the newest checkpoint over ONE pass of the
        validation set (src/trainer.py:882-960 without the best / worst drawings) -> {"kpr_loss", "mr_loss" (None without the mesh
        loss), "batches"}.  draw_every_image: every image of every batch is drawn (``draw_results``) into an event file under
        ``<model_dir or checkpoint_dir>/checkpoint_validation`` as ``vis_images/<i>`` at step = the batch's 1-based number."""
        import torch

        if self.val_dataset is None:
            raise RuntimeError("validate_checkpoint needs a validation dataset")
        if restore:
            self.restore()
        kpr, mr = [], []
        writer = None
        if draw_every_image:
            from .summary import SummaryWriter

            if not (self.model_dir or self.checkpoint_dir):
                raise RuntimeError("draw_every_image needs config.model_dir or config.checkpoint_dir for its event file")
            writer = SummaryWriter(os.path.join(self.model_dir or self.checkpoint_dir, "checkpoint_validation"))
        try:
            for batch in self.val_dataset:
                loaded = self._load_images(batch, augment=False)
                r = self.val_step(*loaded)
                kpr.append(r["kpr_losses"][-1])
                if self.use_mesh_repro_loss:
                    mr.append(r["mr_losses"][-1])
                if writer is not None:
                    for i, png in enumerate(self.draw_rows(*loaded, range(int(loaded[0].shape[0])), val_result=r)):
                        writer.image("vis_images/%d" % i, png, len(kpr))
                    writer.flush()
        finally:
            if writer is not None:
                writer.close()
        if not kpr:
            raise ValueError("the validation dataset yields no batch")
        host = torch.stack([t.reshape(()).float() for t in kpr + mr]).cpu().numpy()
        return {"kpr_loss": float(host[:len(kpr)].mean()), "mr_loss": float(host[len(kpr):].mean()) if mr else None, "batches": len(kpr)}

    def score_val_result(self, result, seg_gts, kp_gt):
        """the last stage's scores of one validation batch from what ``val_step`` returned (no second forward): one ``hpe_eval_scores``
        launch on the reprojected vertices, the sums reduced over the ranks -> ``Scores.result_tensors()``, device scalars"""
        from .metrics import Scores, eval_scores
        from .projection import reproject_vertices

        S = self.predictor.img_size
        verts2d = reproject_vertices(result["generated_verts"][:, -1].contiguous(), result["generated_cams"][:, -1].contiguous(), (S, S))
        sc = Scores().add(*eval_scores([verts2d], self.predictor.score_faces(), seg_gts, kp_gt, [result["pred_keypoints"][:, -1].contiguous()]))
        if self.reducer is not None:
            sc.reduce(self.reducer)
        return sc.result_tensors()

    def score_checkpoint(self, restore=True, draw_best_worst=0):
        """PCK and silhouette scores of the newest checkpoint over ONE pass of the validation set, loaded as ``validate_checkpoint`` loads
        it (centre crop, no flip) -> ``metrics.Scores.result()`` of the last IEF stage, plus ``"stages"``: the same for every stage, and
        ``"batches"``.  Data-parallel: every rank scores its shard and the sums are added over the ranks in one collective.
        draw_best_worst = n > 0: the images of the pass are ranked by the last stage's mean pixel error of their visible joints and by
        their IoU (ties: the earlier record first; an image with no visible joint / an empty union is not ranked), and the n best and n
        worst of each are drawn (``draw_rows``) into an event file under ``<model_dir or checkpoint_dir>/checkpoint_scores`` as
        ``best_kp/<i>``, ``worst_kp/<i>``, ``best_iou/<i>``, ``worst_iou/<i>`` (i = 0: the best / the worst), at step = the image's
        1-based record number.  Only the batches of the at most 4n current candidates stay on the device; ranking reads two numbers per
        image per batch.  This is the per-image form of the reference's best / worst drawings (src/trainer.py:916-989), which rank whole
        batches by their loss.  Data-parallel: rank 0 draws, from its own shard."""
        import torch

        from .metrics import NUM_LSP_JOINTS, Scores

        if self.val_dataset is None:
            raise RuntimeError("score_checkpoint needs a validation dataset")
        n = int(draw_best_worst)
        draw = n > 0 and self.rank == 0
        if draw and not (self.model_dir or self.checkpoint_dir):
            raise RuntimeError("draw_best_worst needs config.model_dir or config.checkpoint_dir for its event file")
        if restore:
            self.restore()
        scores, batches, seen = Scores(), 0, 0
        by_kp, by_iou, kept = BestWorst(n), BestWorst(n), {}  # kept: first record number of a batch -> its loaded tensors
        for batch in self.val_dataset:
            loaded = self._load_images(batch, augment=False)
            counts, kp_err, norm, iou = self.predictor.score_step(*loaded)
            scores.add(counts, kp_err, norm)
            batches += 1
            if draw:
                e = kp_err[-1, :, :NUM_LSP_JOINTS].double()
                vis = e >= 0
                px = torch.where(vis, e, torch.zeros_like(e)).sum(1) / vis.sum(1)  # NaN where no joint is visible
                host = torch.stack([px, iou[-1]]).cpu().numpy()
                for row in range(host.shape[1]):
                    by_kp.add(host[0, row], seen + row)
                    by_iou.add(host[1, row], seen + row)
                kept[seen] = loaded
                wanted = by_kp.records() | by_iou.records()
                kept = {first: t for first, t in kept.items() if any(first <= r < first + int(t[0].shape[0]) for r in wanted)}
            seen += int(loaded[0].shape[0])
        if not batches:
            raise ValueError("the validation dataset yields no batch")
        if self.reducer is not None:
            scores.reduce(self.reducer)
        out = scores.result()
        out["stages"], out["batches"] = scores.results(), batches
        if draw:
            from .summary import SummaryWriter

            results = {}  # one val_step per kept batch: draw_rows takes the vertices, keypoints and cameras from it
            with SummaryWriter(os.path.join(self.model_dir or self.checkpoint_dir, "checkpoint_scores")) as writer:
                for family, ranked in (("best_kp", by_kp.low), ("worst_kp", by_kp.high), ("best_iou", by_iou.high), ("worst_iou", by_iou.low)):
                    for i, (_value, record) in enumerate(ranked):
                        first = max(f for f in kept if f <= record)
                        if first not in results:
                            results[first] = self.predictor.val_step(*kept[first], use_mesh_repro_loss=False)
                        png = self.draw_rows(*kept[first], [record - first], val_result=results[first])[0]
                        writer.image("%s/%d" % (family, i), png, record + 1)
        return out

    def score_checkpoint_3d(self, dataset, restore=True):
        """MPJPE, PA-MPJPE, PVE and PA-PVE (DESIGN.md "3-D pose scores") of the newest checkpoint over ONE pass of ``dataset``, an iterable
        of ``(images_or_records, gt)``: images [B,224,224,3], or a list of parsed image records, loaded as ``validate_checkpoint`` loads
        them (centre crop, no flip); ``gt`` a dict with ``theta`` [B,85], or with ``joints3d`` [B,19 or 14,3] and optionally ``verts``
        [B,6890,3] and ``joint_weights``.  -> ``metrics.Scores3D.result()`` of the last IEF stage, plus ``"stages"``: the same for every
        stage, and ``"batches"``.  Data-parallel: every rank scores its shard and the sums are added over the ranks in one collective;
        rank 0 logs."""
        from .metrics import Scores3D

        if restore:
            self.restore()
        scores, batches = Scores3D(), 0
        for images, gt in dataset:
            if isinstance(images, (tuple, list)):
                images = self._load_images(images, augment=False)[0]
            joint_err, summary, _ = self.predictor.score_step_3d(images, theta_gt=gt.get("theta"), joints3d_gt=gt.get("joints3d"),
                                                                 verts_gt=gt.get("verts"), joint_weights=gt.get("joint_weights"))
            scores.add(joint_err, summary)
            batches += 1
        if not batches:
            raise ValueError("the dataset yields no batch")
        if self.reducer is not None:
            scores.reduce(self.reducer)
        out = scores.result()
        out["stages"], out["batches"] = scores.results(), batches
        self.log("3-D scores over %d images: mpjpe=%.1f mm pa_mpjpe=%.1f mm pve=%.1f mm pa_pve=%.1f mm pck3d_150=%.3f auc3d=%.3f"
                 % (out["images"], out["mpjpe_mm"], out["pa_mpjpe_mm"], out["pve_mm"], out["pa_pve_mm"], out["pck3d_150"], out["auc3d"]))
        return out

    # ------------------------------------------------------------------ checkpoints
    def weights(self):
        """the live networks as the Keras-layout dict (host arrays): encoder with its moving statistics, regressor, critic, and
        ``mean_theta``"""
        gen = self.generator
        w = resnet_spec.flat_to_params(gen.encoder_params, resnet_spec.stats_to_params(gen.encoder_stats))
        w.update(regressor_spec.flat_to_params(gen.params))
        if self.critic is not None:
            w.update(critic_spec.flat_to_params(self.critic.params))
        return w

    def save(self):
        """``checkpoint.save(checkpoint_prefix)``: ``<checkpoint_dir>/ckpt-N`` with N = the save counter -> the prefix"""
        if self.generator is None:
            raise RuntimeError("this Trainer was built with validation_only")
        if not self.checkpoint_dir:
            raise RuntimeError("config.checkpoint_dir is not set")
        w = self.weights()
        mean = w.pop("mean_theta")
        sd = self.generator.optimizer.state_dict()
        slots = tf_checkpoint.flat_slots("encoder", sd["slots"]["encoder"]["m"], sd["slots"]["encoder"]["v"])
        slots.update(tf_checkpoint.flat_slots("regressor", sd["slots"]["regressor"]["m"], sd["slots"]["regressor"]["v"]))
        opts = {"generator_optimizer": dict(sd, slots=slots)}
        if self.critic is not None:
            sd = self.critic.optimizer.state_dict()
            opts["discriminator_optimizer"] = dict(sd, slots=tf_checkpoint.flat_slots("critic", sd["slots"]["critic"]["m"], sd["slots"]["critic"]["v"]))
        self.save_counter += 1
        os.makedirs(self.checkpoint_dir, exist_ok=True)
        return tf_checkpoint.save_checkpoint(os.path.join(self.checkpoint_dir, "ckpt-%d" % self.save_counter), w, inital_theta=self.inital_theta,
                                             mean_var=mean, optimizers=opts, save_counter=self.save_counter)

    def restore(self, prefix_or_dir=None, verify=True):
        """``checkpoint.restore(latest_checkpoint(checkpoint_dir))``: weights, moving statistics, mean theta, optimiser moments and step
        counts into the live engine and trainers, on the device.  The learning rates stay the configuration's.  A checkpoint without
        optimiser state restores the weights and keeps fresh moments (the reference's ``expect_partial()``).  -> the prefix"""
        import torch

        src = prefix_or_dir if prefix_or_dir is not None else self.checkpoint_dir
        w, info = tf_checkpoint.load_hmr_weights(src, verify=verify)
        prefix = info["prefix"]
        eng, dev = self.engine, self.engine.tdev
        mean = np.asarray(w["mean_var"], np.float32).reshape(-1) if "mean_var" in w else self.inital_theta.reshape(-1)
        reg_flat = torch.from_numpy(regressor_spec.params_to_flat(w, mean)).to(dev)
        enc_flat = torch.from_numpy(resnet_spec.params_to_flat(w)).to(dev)
        stats = torch.from_numpy(resnet_spec.params_to_stats(w)).to(dev)
        try:
            cw = tf_checkpoint.load_critic_weights(prefix, verify=verify)[0]
        except tf_checkpoint.NoCriticError:
            cw = None
        if self.generator is None:  # validation only: no trainers to fill, the engine alone
            eng.set_encoder_params(enc_flat)
            eng.set_regressor_params(reg_flat)
            if cw is not None:
                eng.load_critic(cw)
            if not torch.equal(stats, eng.encoder_stats()):
                raise RuntimeError("validation_only: the checkpoint's moving statistics differ from the ones this engine was built with; "
                                   "build the Trainer with config.checkpoint_dir naming the checkpoint")
            return prefix
        gen = self.generator
        with torch.no_grad():
            gen.params.copy_(reg_flat)
            gen.encoder_params.copy_(enc_flat)
            gen.encoder_stats.copy_(stats)
        eng.set_regressor_params(gen.params)
        eng.set_encoder_params_dev(gen.encoder_params)
        eng.set_encoder_stats_dev(gen.encoder_stats)
        if self.critic is not None:
            if cw is None:
                raise tf_checkpoint.NoCriticError("%s has no discriminator to resume the critic from" % prefix)
            with torch.no_grad():
                self.critic.params.copy_(torch.from_numpy(critic_spec.params_to_flat(cw)).to(dev))
            eng.set_critic_params(self.critic.params)
        try:
            st = tf_checkpoint.load_training_state(prefix, verify=verify)
        except tf_checkpoint.CheckpointError as e:
            if "no optimiser state" not in str(e):
                raise
            self.log("no optimiser state in %s: starting fresh moments" % prefix)
            self._sync_replicas()
            return prefix
        go = st.get("generator_optimizer")
        if go is not None and go["encoder"] is not None and go["regressor"] is not None:
            gen.optimizer.load_state_dict({"iterations": go["iter"], "slots": {"encoder": go["encoder"], "regressor": go["regressor"]}}, hyper=False)
        do = st.get("discriminator_optimizer")
        if self.critic is not None and do is not None and do["critic"] is not None:
            self.critic.optimizer.load_state_dict({"iterations": do["iter"], "slots": {"critic": do["critic"]}}, hyper=False)
        if st["save_counter"] is not None:
            self.save_counter = int(st["save_counter"])
        self._sync_replicas()
        return prefix
