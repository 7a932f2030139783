"""KerasAdam: the reference's ``tf.keras.optimizers.Adam`` (src/trainer.py:183-184) on flat CUDA parameter tensors, i.e. TensorFlow's
fused ResourceApplyAdam

    alpha = lr * sqrt(1 - beta_2^t) / (1 - beta_1^t)
    m += (g - m) * (1 - beta_1);  v += (g * g - v) * (1 - beta_2);  var -= (m * alpha) / (sqrt(v) + eps)

run by libhpe_hip.so (hpe_adam_advance, hpe_adam_apply; csrc/adam.hip).  ``torch.optim.Adam`` computes
``lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)``: epsilon sits elsewhere, so the two differ by more than rounding and a
checkpoint's moments fit only this form.  All registered tensors share ONE step count, as the variables of one Keras optimiser do
(the reference's ``generator_optimizer`` steps the encoder and the regressor).  The step count, the powers and alpha live on the
device: ``step()`` reads nothing on the host and can be captured in a graph on one stream."""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict

import numpy as np

from . import _lib


def _f32(x):
    return float(np.float32(x))


class KerasAdam(object):
    def __init__(self, lr, beta_1=0.9, beta_2=0.999, eps=1e-7):
        if not (0.0 <= beta_1 < 1.0 and 0.0 <= beta_2 < 1.0):
            raise ValueError("beta_1 and beta_2 must be in [0, 1)")
        if not eps >= 0.0:
            raise ValueError("eps must be >= 0")
        self.lr, self.beta_1, self.beta_2, self.eps = float(lr), float(beta_1), float(beta_2), float(eps)
        self.lib = _lib.load()
        self.params = OrderedDict()  # name -> the registered tensor
        self.slots = OrderedDict()  # name -> {"m": tensor, "v": tensor}
        self._state = None  # 4 doubles on the device: t, beta_1^t, beta_2^t, alpha
        self._pending_t = 0

    # Keras computes 1 - beta in the variable's dtype: the float32 nearest to beta, subtracted from 1 in float32
    @property
    def one_minus_beta_1(self):
        return _f32(np.float32(1.0) - np.float32(self.beta_1))

    @property
    def one_minus_beta_2(self):
        return _f32(np.float32(1.0) - np.float32(self.beta_2))

    def _stream(self, t):
        import torch

        return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)

    def _ensure_state(self, like):
        import torch

        if self._state is None:
            self._state = torch.tensor([0.0, 1.0, 1.0, 0.0], dtype=torch.float64, device=like.device)
            if self._pending_t:
                self._set_step(self._pending_t)
        return self._state

    def _set_step(self, t):
        _lib.check(self.lib.hpe_adam_set_step(self._state.data_ptr(), int(t), self.beta_1, self.beta_2, self._stream(self._state)))

    def add(self, name, flat_tensor):
        """register a flat (1-D, contiguous, float32) CUDA parameter tensor; its moments ``m`` and ``v`` start as zeros"""
        import torch

        t = flat_tensor
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 1 or not t.is_contiguous():
            raise ValueError("%s must be a flat contiguous float32 CUDA tensor" % name)
        if name in self.params:
            raise ValueError("%s is registered already" % name)
        self.params[name] = t
        self.slots[name] = {"m": torch.zeros_like(t, requires_grad=False), "v": torch.zeros_like(t, requires_grad=False)}
        self._ensure_state(t)
        return t

    def zero_grad(self):
        for p in self.params.values():
            p.grad = None

    def step(self, only=None):
        """one hpe_adam_advance, then one hpe_adam_apply per registered tensor on its ``.grad``; a tensor without a gradient is an error.
        only: names of the tensors this step applies to (Keras' ``apply_gradients`` on a subset: the step count still moves once)"""
        if not self.params:
            raise RuntimeError("KerasAdam.step: no tensor registered")
        todo = [(n, p) for n, p in self.params.items() if only is None or n in only]
        if only is not None and len(todo) != len(set(only)):
            raise KeyError("KerasAdam.step: unknown tensor among %s" % (tuple(only),))
        grads = []
        for name, p in todo:
            g = p.grad
            if g is None:
                raise RuntimeError("KerasAdam.step: %s has no gradient" % name)
            if g.dtype != p.dtype or g.shape != p.shape or not g.is_cuda:
                raise ValueError("KerasAdam.step: the gradient of %s does not match it" % name)
            grads.append(g if g.is_contiguous() else g.contiguous())
        st = self._state
        stream = self._stream(st)
        _lib.check(self.lib.hpe_adam_advance(st.data_ptr(), self.lr, self.beta_1, self.beta_2, stream))
        omb1, omb2, eps = self.one_minus_beta_1, self.one_minus_beta_2, _f32(self.eps)
        for (name, p), g in zip(todo, grads):
            s = self.slots[name]
            _lib.check(self.lib.hpe_adam_apply(p.data_ptr(), s["m"].data_ptr(), s["v"].data_ptr(), g.data_ptr(), p.numel(), st.data_ptr(),
                                               omb1, omb2, eps, stream))

    @property
    def iterations(self):
        """the shared step count; reads the device (synchronises): not for use inside a step"""
        return self._pending_t if self._state is None else int(self._state[0].item())

    def state_dict(self):
        """{'iterations', 'learning_rate', 'beta_1', 'beta_2', 'epsilon', 'slots': {name: {'m', 'v'}}} with the slots as CPU tensors:
        what the checkpoint writer stores"""
        return {"iterations": self.iterations, "learning_rate": self.lr, "beta_1": self.beta_1, "beta_2": self.beta_2, "epsilon": self.eps,
                "slots": {n: {k: t.detach().cpu().clone() for k, t in s.items()} for n, s in self.slots.items()}}

    def load_state_dict(self, state, hyper=True):
        """the step count, the slots of every registered tensor (all must be there, with the tensor's size) and, with ``hyper``, the
        hyper-parameters.  The powers are recomputed from the step count (hpe_adam_set_step): the next step has the bits of a run that
        was never interrupted."""
        import torch

        t = int(state["iterations"])
        if t < 0:
            raise ValueError("iterations must be >= 0")
        slots = state.get("slots", {})
        new = {}
        for name, p in self.params.items():
            if name not in slots:
                raise KeyError("no optimiser slots for %s" % name)
            for k in ("m", "v"):
                src = slots[name][k]
                src = src if isinstance(src, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(src, dtype=np.float32))
                if src.numel() != p.numel():
                    raise ValueError("slot %s of %s holds %d values, the tensor %d" % (k, name, src.numel(), p.numel()))
                new[name, k] = src.reshape(-1).to(torch.float32)
        if hyper:
            self.lr = float(state.get("learning_rate", self.lr))
            self.beta_1 = float(state.get("beta_1", self.beta_1))
            self.beta_2 = float(state.get("beta_2", self.beta_2))
            self.eps = float(state.get("epsilon", self.eps))
        for (name, k), src in new.items():
            self.slots[name][k].copy_(src)
        self._pending_t = t
        if self._state is not None:
            self._set_step(t)
