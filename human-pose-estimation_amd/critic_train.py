"""CriticTrainer: the critic half of the reference's Trainer.train_step (src/trainer.py:508-583) -- the WGAN loss with the gradient
penalty, its gradient with respect to the critic's weights (hpe_critic_weight_grad), an Adam step and the new weights back into the
engine on the device (hpe_critic_set_params_dev).  Adam is torch.optim.Adam on ONE flat tensor; everything else runs in
libhpe_hip.so.  The generator update and the data loader are not part of it.

Data-parallel: with ``reducer=`` (distributed.Reducer) ``step`` takes this rank's rows and ``global_rows``, the rows of all ranks: the
plain sums and N cross the ranks in ONE packed all-reduce before the norms, the tangents and grad_scores divide by the global row count,
the flat gradient is summed over the ranks, and the reported losses are those of the global batch."""
from __future__ import annotations

from .ops import critic_wgan_loss

CRITIC_LR = 0.0005  # the reference's critic_lr (src/config.py:65)
ADAM_EPS = 1e-7  # tf.keras.optimizers.Adam's epsilon (src/trainer.py:184)


class CriticTrainer(object):
    def __init__(self, engine, lr=CRITIC_LR, betas=(0.9, 0.999), eps=ADAM_EPS, gp_weight=10.0, generator=None, optimizer="torch", reducer=None,
                 clipnorm=None, skip_nonfinite=False):
        """engine: an HpeEngine with a loaded critic (the starting point: a checkpoint's discriminator or a fresh initialisation).
        ``params`` is the flat parameter tensor (critic_spec.flat_layout) the optimiser owns; ``critic_spec.flat_to_params(params)``
        gives the dict ``load_critic`` / ``weights.npz`` take.  generator: the torch.Generator of the interpolation draws.  optimizer:
        "torch" (torch.optim.Adam) or "keras" (``KerasAdam``, optim.py: the reference's fused update in HIP).  clipnorm /
        skip_nonfinite (``optimizer="keras"`` only): its guarded step -- global-norm clipping, and a step with a non-finite gradient
        leaves the weights, the moments and the step count as they were -- decided on the device from per-layer statistics of the
        gradient summed over the ranks; ``step`` then also returns ``grad_norm`` and ``step_applied`` (0-dim device tensors)."""
        import torch

        if not engine.has_critic:
            raise RuntimeError("CriticTrainer needs an engine with a loaded critic (HpeEngine.load_critic)")
        self.engine = engine
        self.gp_weight = float(gp_weight)
        self.generator = generator
        self.reducer = reducer
        self.params = engine.critic_params()
        if optimizer not in ("torch", "keras"):
            raise ValueError("optimizer must be 'torch' or 'keras'")
        self.guarded = clipnorm is not None or bool(skip_nonfinite)
        if self.guarded and optimizer != "keras":
            raise ValueError("clipnorm / skip_nonfinite need optimizer='keras' (the guarded step is KerasAdam's)")
        if optimizer == "keras":
            from .optim import KerasAdam, layer_segments

            self.optimizer = KerasAdam(lr, betas[0], betas[1], eps, global_clipnorm=clipnorm, skip_nonfinite=skip_nonfinite)
            self.optimizer.add("critic", self.params, segments=layer_segments("critic", engine.lib)[0] if self.guarded else None)
        else:
            self.optimizer = torch.optim.Adam([self.params], lr=lr, betas=betas, eps=eps)

    def step(self, real, fake, interp=None, global_rows=None):
        """One critic update on (joints, shapes, Rs) triples of equal row count -> {'critic_network_loss', 'critic_penalty'} as in
        the reference's result (src/trainer.py:605-608): the loss INCLUDING the weighted penalty, and the penalty, both before the
        step, as 0-dim device tensors.  Nothing reads the device."""
        if self.reducer is None:
            r = critic_wgan_loss(self.engine, real, fake, gp_weight=self.gp_weight, interp=interp, generator=self.generator)
        else:
            r = critic_wgan_loss(self.engine, real, fake, gp_weight=self.gp_weight, interp=interp, generator=self.generator,
                                 reduce=self.reducer.sum_block, global_rows=global_rows)
            self.reducer.sum_grad(r["grad"])
        self.params.grad = r["grad"]
        self.optimizer.step()
        self.engine.set_critic_params(self.params)
        out = {"critic_network_loss": r["loss"], "critic_penalty": r["penalty"], "critic_wgan": r["wgan"]}
        if self.guarded:  # copies: the guard block is the next step's too
            out["grad_norm"], out["step_applied"] = self.optimizer.grad_norm.clone(), self.optimizer.step_applied.clone()
        return out

    def step_from_thetas(self, real, thetas, interp=None, global_batch=None):
        """The same with the fake rows taken from the generator's thetas: ``thetas`` is the list of the IEF stages' theta [B,85]; their
        joints and rotations come from hpe_smpl, and all stages are concatenated as src/trainer.py:511-516 does.  ``real`` has either
        as many rows as the concatenation or B rows, which then serve every stage.  global_batch (with a reducer): the rows of one
        stage over all ranks."""
        import torch

        thetas = [t.detach() for t in thetas]
        joints, Rs = [], []
        mb = self.engine.max_batch
        with torch.no_grad():
            for t in thetas:
                for lo in range(0, t.shape[0], mb):
                    o = self.engine.smpl(t[lo : lo + mb], want=("joints", "Rs"))
                    joints.append(o["joints"])
                    Rs.append(o["Rs"])
        theta = torch.cat(thetas)
        fake = (torch.cat(joints), theta[:, 75:], torch.cat(Rs))
        if real[0].shape[0] != theta.shape[0]:
            if real[0].shape[0] * len(thetas) != theta.shape[0]:
                raise ValueError("real must have as many rows as one stage or as all stages together")
            real = tuple(torch.cat([t] * len(thetas)) for t in real)
        return self.step(real, fake, interp=interp, global_rows=None if global_batch is None else int(global_batch) * len(thetas))
