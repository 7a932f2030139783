"""GeneratorTrainer: the generator half of the reference's Trainer.train_step (src/trainer.py:383-505) after the encoder -- the IEF loop
with dropout at the last stage, SMPL, the keypoint / mesh reprojection losses and the critic term on the last stage, their gradient with
respect to the RegressionNetwork and mean theta (hpe_smpl_backward, hpe_kp_loss_backward, hpe_mesh_loss_grad, hpe_critic_backward,
hpe_regressor_backward), an Adam step and the new weights back into the engine on the device (hpe_regressor_set_params_dev).  Adam is
torch.optim.Adam on ONE flat tensor; everything else runs in libhpe_hip.so.  With ``train_encoder=True`` the encoder (BatchNorm statistics
fixed, fp32) is in the same step, as in the reference (src/trainer.py:481): features come from ``encoder_features``, the one
``.backward()`` fills both flat gradients, a second Adam steps the encoder's flat tensor and ``set_encoder_params_dev`` installs it on the device, in stream order
(hpe_encoder_set_params_dev).  ``encoder_bn="batch"`` is the reference's own mode (src/trainer.py:386, training=True): every BatchNorm
normalises with the statistics of the batch, the gradient flows through them, and after the Adam steps the moving statistics follow the
batch (hpe_encoder_update_stats on ``encoder_stats``, installed by hpe_encoder_set_stats_dev).
``grad_features`` is returned either way.

Data-parallel (DESIGN.md "Data-parallel training"): with ``reducer=`` (distributed.Reducer) and ``global_batch=`` G, ``step`` takes this
rank's rows of a batch of G spread across the ranks.  Every loss term is the rank's SHARE of the global loss -- the keypoint numerator over
the visible count of all ranks (all-reduced on the device before the forward), the mesh sum as it is, the critic's column sums over G --
so that after ``loss.backward()`` ONE sum per flat gradient over the ranks is the gradient of the global batch, which every rank then
steps with; BatchNorm takes its statistics over the G images (``HpeEngine.set_encoder_reduce``) and the moving statistics follow
those.  The reported losses are the global values, from one packed all-reduce per step.

3-D supervision (DESIGN.md "3-D supervision"): ``step(..., gt3d=)`` with ``joints3d_loss_weight`` / ``smpl_loss_weight`` above 0 adds the
L2 loss on the pelvis-aligned 3-D joints and the L2 loss on the rotations and the shape (hpe_loss3d: one launch for all stages;
hpe_loss3d_backward for the last), masked per row; data-parallel, their two counts travel with the keypoint count."""
from __future__ import annotations

from . import engine as _engine
from .ops import (encoder_features, generator_critic_loss, kp_reprojection_loss, kp_reprojection_loss_share, kp_visible_count, loss3d,
                  loss3d_counts, mesh_reprojection_loss, regressor_thetas)

GENERATOR_LR = 0.0001  # the reference's generator_lr (src/config.py:64-69)
ADAM_EPS = 1e-7  # tf.keras.optimizers.Adam's epsilon


class GeneratorTrainer(object):
    def __init__(self, engine, lr=GENERATOR_LR, betas=(0.9, 0.999), eps=ADAM_EPS, kpr_loss_weight=60.0, mr_loss_weight=0.001,
                 critic_loss_weight=0.01, dropout=0.5, generator=None, train_encoder=False, encoder_lr=None, encoder_bn="frozen",
                 bn_momentum=0.99, bn_unbiased=True, optimizer="torch", reducer=None, global_batch=None, encoder_precision="fp32",
                 clipnorm=None, skip_nonfinite=False, joints3d_loss_weight=0.0, smpl_loss_weight=0.0):
        """engine: a finalized HpeEngine with a regressor, mean theta and SMPL (and a critic, for the critic term).  ``params`` is the
        flat parameter tensor (regressor_spec.flat_layout) the optimiser owns; ``regressor_spec.flat_to_params(params)`` gives the
        dict ``load_regressor`` / ``load_mean_theta`` take.  generator: the torch.Generator of the dropout draws.  train_encoder: also
        step the encoder's flat tensor ``encoder_params`` (needs ``engine.reserve_encoder_train(B)``; Adam with the same
        hyper-parameters, lr ``encoder_lr``, default the generator's) whenever ``step`` is given images.  encoder_bn: "frozen" (the
        moving statistics stay fixed) or "batch" (needs ``engine.reserve_encoder_train(B, batch_norm=True)``): batch statistics in the
        forward and the backward, and ``encoder_stats``, the flat statistics tensor (resnet_spec.stats_to_params), moves with momentum
        ``bn_momentum`` after every step (``bn_unbiased``: the batch variance times M / (M - 1)).  optimizer: "torch"
        (torch.optim.Adam, one per flat tensor) or "keras": ONE ``KerasAdam`` (optim.py: the reference's fused update in HIP) that owns
        the regressor's and, with ``train_encoder``, the encoder's tensor under one step count, as the reference's
        ``generator_optimizer`` does; it has one rate, so an ``encoder_lr`` other than ``lr`` is refused.  reducer / global_batch:
        data-parallel training (the module's text); with ``encoder_bn="batch"`` the reducer's callback is installed as the engine's
        reduce hook.  ``reducer=None`` is the single-process trainer, unchanged.  encoder_precision: "fp32", or "bf16" for the
        mixed-precision encoder walks (needs ``engine.reserve_encoder_train(B, precision="bf16")``; ``encoder_bn="frozen"`` only): the
        fp32 master tensor ``encoder_params``, the optimiser and ``set_encoder_params_dev`` are as in fp32.  "mixed": those walks with
        either ``encoder_bn`` (with "batch": ``engine.reserve_encoder_train(B, batch_norm=True, precision="mixed")``); the moving
        statistics, ``update_encoder_stats``, ``set_encoder_stats_dev`` and the reduce hook are as in fp32.  clipnorm / skip_nonfinite
        (``optimizer="keras"`` only): the guarded step of ``KerasAdam`` (global-norm clipping over the tensors stepped; a step with a
        non-finite gradient is undone as a whole: both flat tensors, the moments, the step count and ``encoder_stats`` keep their
        bits), decided on the device from per-layer statistics taken after the data-parallel sum, so every rank decides alike.  The
        result of ``step`` then has ``grad_norm`` and ``step_applied`` (0-dim device tensors).  joints3d_loss_weight /
        smpl_loss_weight: the weights of the two 3-D supervision terms of ``step(..., gt3d=)``; 0, the default, leaves a term out."""
        import torch

        if not 0.0 <= dropout < 1.0:
            raise ValueError("dropout must be in [0, 1)")
        self.engine = engine
        self.reducer, self.global_batch = reducer, None
        if reducer is not None:
            if global_batch is None or int(global_batch) < 1:
                raise ValueError("reducer= needs global_batch, the rows of all ranks together")
            self.global_batch = int(global_batch)
        self.kpr_loss_weight, self.mr_loss_weight, self.critic_loss_weight = float(kpr_loss_weight), float(mr_loss_weight), float(critic_loss_weight)
        self.joints3d_loss_weight, self.smpl_loss_weight = float(joints3d_loss_weight), float(smpl_loss_weight)
        if self.joints3d_loss_weight < 0.0 or self.smpl_loss_weight < 0.0:
            raise ValueError("joints3d_loss_weight and smpl_loss_weight must be >= 0")
        self.dropout = float(dropout)
        self.generator = generator
        self.params = engine.regressor_params().requires_grad_(True)
        if optimizer not in ("torch", "keras"):
            raise ValueError("optimizer must be 'torch' or 'keras'")
        self.keras = optimizer == "keras"
        self.guarded = clipnorm is not None or bool(skip_nonfinite)
        if self.guarded and not self.keras:
            raise ValueError("clipnorm / skip_nonfinite need optimizer='keras' (the guarded step is KerasAdam's)")
        if self.keras:
            from .optim import KerasAdam, layer_segments

            if train_encoder and encoder_lr is not None and float(encoder_lr) != float(lr):
                raise ValueError("optimizer='keras' steps the encoder and the regressor with one optimiser: encoder_lr must equal lr")
            self.optimizer = KerasAdam(lr, betas[0], betas[1], eps, global_clipnorm=clipnorm, skip_nonfinite=skip_nonfinite)
            self.optimizer.add("regressor", self.params, segments=layer_segments("regressor", engine.lib)[0] if self.guarded else None)
        else:
            self.optimizer = torch.optim.Adam([self.params], lr=lr, betas=betas, eps=eps)
        self.train_encoder = bool(train_encoder)
        if encoder_bn not in ("frozen", "batch"):
            raise ValueError("encoder_bn must be 'frozen' or 'batch'")
        if not 0.0 <= bn_momentum <= 1.0:
            raise ValueError("bn_momentum must be in [0, 1]")
        self.encoder_bn, self.bn_momentum, self.bn_unbiased = encoder_bn, float(bn_momentum), bool(bn_unbiased)
        from .engine import HpeEngine

        HpeEngine._mixed(encoder_precision, encoder_bn)  # "bf16" with batch statistics is refused ("mixed" is its spelling): ValueError
        self.encoder_precision = encoder_precision
        self.encoder_params = self.encoder_optimizer = self.encoder_stats = None
        if self.train_encoder and encoder_bn == "batch":
            self.encoder_stats = engine.encoder_stats()
        if self.train_encoder:
            self.encoder_params = engine.encoder_params().requires_grad_(True)
            if self.keras:
                self.optimizer.add("encoder", self.encoder_params, segments=layer_segments("encoder", engine.lib)[0] if self.guarded else None)
            else:
                self.encoder_optimizer = torch.optim.Adam([self.encoder_params], lr=lr if encoder_lr is None else encoder_lr, betas=betas, eps=eps)
        if reducer is not None and self.train_encoder and encoder_bn == "batch":
            engine.set_encoder_reduce(reducer.callback, self.global_batch, owner=reducer)

    def draw_masks(self, B):
        """the dropout multipliers [2,B,1024] of one step: 0 with probability ``dropout``, else 1 / (1 - dropout); None without dropout"""
        import torch

        if self.dropout == 0.0:
            return None
        u = torch.rand((2, B, 1024), generator=self.generator, device=self.engine.tdev, dtype=torch.float32)
        return (u >= self.dropout).to(torch.float32) * (1.0 / (1.0 - self.dropout))

    def _smpl(self, theta, want):
        """engine.smpl in chunks of max_batch rows (with gradient where theta carries one)"""
        import torch

        mb = self.engine.max_batch
        if theta.shape[0] <= mb:
            return self.engine.smpl(theta, want=want)
        parts = [self.engine.smpl(theta[lo : lo + mb], want=want) for lo in range(0, theta.shape[0], mb)]
        return {k: torch.cat([p[k] for p in parts]) for k in want}

    def _sum_grads(self, enc):
        """data-parallel: each flat gradient summed over the ranks, one all-reduce per tensor, before the optimiser reads it"""
        if self.reducer is None:
            return
        self.reducer.sum_grad(self.params.grad)
        if enc:
            self.reducer.sum_grad(self.encoder_params.grad)

    def step(self, images_or_features, kp_gt, seg_gts=None, use_critic=None, drop="draw", gt3d=None):
        """One generator update.  images_or_features: images [B,224,224,3] (the encoder runs without gradient) or features [B,2048];
        kp_gt [B,K,3] (x, y, visibility); seg_gts [B,H,W(,1)] adds the mesh reprojection loss; use_critic (default: the engine has a
        critic) adds the critic term.  drop: the multipliers [2,B,1024] of this step, None for none, "draw" to draw them.  gt3d: the
        batch's ``ops.Gt3D`` (``augment.gt3d_real``); each 3-D term whose weight is above 0 then joins the loss, and the result gains
        joints3d_losses / smpl_param_losses (lists over the stages, weighted).  None, or both weights 0: the step without them.
        -> the reference's result keys: kpr_losses, mr_losses, generator_critic_losses (lists over the stages, already weighted, 0-dim
        device tensors; the LAST stage's terms are what is minimised, src/trainer.py:487-496), pred_keypoints, generated_cams (last
        stage), thetas (list over the stages: what CriticTrainer.step_from_thetas takes), and grad_features [B,2048].  Nothing reads
        the device."""
        import torch

        eng = self.engine
        x = images_or_features
        if use_critic is None:
            use_critic = eng.has_critic
        enc = self.train_encoder and x.dim() == 4
        if enc:
            features = encoder_features(eng, x, self.encoder_params, self.encoder_bn, self.encoder_precision)
            features.retain_grad()
        else:
            with torch.no_grad():
                features = x if x.dim() == 2 else torch.cat([eng.encoder(x[lo : lo + eng.max_batch]) for lo in range(0, x.shape[0], eng.max_batch)])
        B = features.shape[0]
        if isinstance(drop, str):
            drop = self.draw_masks(B)
        if not enc:
            features = features.detach().clone().requires_grad_(True)
        thetas = regressor_thetas(eng, features, self.params, drop)
        S = thetas.shape[0]
        red, G = self.reducer, self.global_batch
        if red is not None:
            if B > G:
                raise ValueError("this rank's %d rows exceed global_batch %d" % (B, G))
        use3d = gt3d is not None and (self.joints3d_loss_weight > 0.0 or self.smpl_loss_weight > 0.0)
        if use3d and gt3d.joints.shape[0] != B:
            raise ValueError("gt3d holds %d rows, the batch %d" % (gt3d.joints.shape[0], B))
        counts3d = None
        if red is not None:
            if use3d:  # the two 3-D counts travel with the keypoint count: one collective, three numbers
                block = red.sum_block(torch.cat([kp_visible_count(kp_gt), loss3d_counts(gt3d)]))
                count, counts3d = block[:1], block[1:3]
            else:
                count = red.sum_block(kp_visible_count(kp_gt))  # 2 * #visible of all ranks, before the forward; stays on the device
        kpr, mr, gc, j3, sp = [], [], [], [], []
        # kp2d / verts2d: batch_orth_proj_idrot / reproject_vertices of the stage, as outputs of the one hpe_smpl call (and of its backward)
        want = ("kp2d", "joints", "Rs") + (("verts2d",) if seg_gts is not None else ())
        loss = pred_kp = None
        outs = []
        for i in range(S):
            last = i == S - 1
            with torch.set_grad_enabled(last):
                th = thetas[i] if last else thetas[i].detach()
                o = self._smpl(th, want)
                outs.append((o["joints"], th[:, 75:], o["Rs"]))
                kp = o["kp2d"]
                kpr.append(self.kpr_loss_weight * (kp_reprojection_loss(kp_gt, kp) if red is None else kp_reprojection_loss_share(kp_gt, kp, count)))
                if seg_gts is not None:
                    mr.append(self.mr_loss_weight * mesh_reprojection_loss(eng, seg_gts, o["verts2d"]))
                if use_critic:
                    gc.append(self.critic_loss_weight * generator_critic_loss(eng, o["joints"], th[:, 75:], o["Rs"], global_rows=G))
                if last:
                    pred_kp = kp.detach()
                    loss = kpr[-1] + (mr[-1] if mr else 0.0) + (gc[-1] if gc else 0.0)
        if use3d:  # ONE forward launch for all stages; the last stage's row carries the gradient (hpe_loss3d_backward)
            parts = _engine.loss3d_parts(*[[o[k] for o in outs] for k in range(3)], gt3d)
            for i in range(S):
                with torch.set_grad_enabled(i == S - 1):
                    lj, ls = loss3d(*outs[i], gt3d, counts3d, parts[i])
                if self.joints3d_loss_weight > 0.0:
                    j3.append(self.joints3d_loss_weight * lj)
                if self.smpl_loss_weight > 0.0:
                    sp.append(self.smpl_loss_weight * ls)
            loss = loss + (j3[-1] if j3 else 0.0) + (sp[-1] if sp else 0.0)
        if self.keras:
            self.optimizer.zero_grad()
            loss.backward()
            self._sum_grads(enc)
            self.optimizer.step(only=None if enc or not self.train_encoder else ("regressor",))
        else:
            self.optimizer.zero_grad(set_to_none=True)
            if enc:
                self.encoder_optimizer.zero_grad(set_to_none=True)
            loss.backward()
            self._sum_grads(enc)
            self.optimizer.step()
        eng.set_regressor_params(self.params)
        if enc:
            if not self.keras:
                self.encoder_optimizer.step()
            eng.set_encoder_params_dev(self.encoder_params)
            if self.encoder_bn == "batch":
                if self.guarded:  # a skipped step leaves the moving statistics alone too: chosen on the device, from the guard's flag
                    before = self.encoder_stats.clone()
                    eng.update_encoder_stats(self.encoder_stats, self.bn_momentum, self.bn_unbiased)
                    self.encoder_stats.copy_(torch.where(self.optimizer.step_applied != 0, self.encoder_stats, before))
                else:
                    eng.update_encoder_stats(self.encoder_stats, self.bn_momentum, self.bn_unbiased)
                eng.set_encoder_stats_dev(self.encoder_stats)
        det = lambda ts: [t.detach() for t in ts]  # noqa: E731
        if red is not None:  # the ranks' shares into the losses of the global batch: one packed all-reduce for all of them
            block = red.sum_block(torch.stack([t.detach().reshape(()) for t in kpr + mr + gc + j3 + sp]))
            cut = [0]
            for ts in (kpr, mr, gc, j3, sp):
                cut.append(cut[-1] + len(ts))
            kpr, mr, gc, j3, sp = (list(block[lo:hi]) for lo, hi in zip(cut, cut[1:]))
        out = {"kpr_losses": det(kpr), "mr_losses": det(mr), "generator_critic_losses": det(gc), "pred_keypoints": pred_kp,
               "generated_cams": thetas[S - 1, :, :3].detach(), "thetas": [thetas[i].detach() for i in range(S)],
               "grad_features": features.grad}
        if use3d:
            out["joints3d_losses"], out["smpl_param_losses"] = det(j3), det(sp)
        if self.guarded:  # copies: the guard block is the next step's too
            out["grad_norm"], out["step_applied"] = self.optimizer.grad_norm.clone(), self.optimizer.step_applied.clone()
        return out
