"""KerasAdam: the reference's ``tf.keras.optimizers.Adam`` (src/trainer.py:183-184) on flat CUDA parameter tensors, i.e. TensorFlow's
fused ResourceApplyAdam

    alpha = lr * sqrt(1 - beta_2^t) / (1 - beta_1^t)
    m += (g - m) * (1 - beta_1);  v += (g * g - v) * (1 - beta_2);  var -= (m * alpha) / (sqrt(v) + eps)

run by libhpe_hip.so (hpe_adam_advance, hpe_adam_apply; csrc/adam.hip).  ``torch.optim.Adam`` computes
``lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)``: epsilon sits elsewhere, so the two differ by more than rounding and a
checkpoint's moments fit only this form.  All registered tensors share ONE step count, as the variables of one Keras optimiser do
(the reference's ``generator_optimizer`` steps the encoder and the regressor).  The step count, the powers and alpha live on the
device: ``step()`` reads nothing on the host and can be captured in a graph on one stream.

``global_clipnorm=`` and ``skip_nonfinite=`` make the step a guarded one (DESIGN.md "Guarded optimiser step"; the reference has neither,
src/trainer.py:84): hpe_grad_stats reduces every stepped gradient to records of (sum of squares, max |g|, non-finite count) per
registered segment, ONE hpe_adam_guard in the place of hpe_adam_advance takes their global norm and decides, and hpe_adam_apply_guarded
steps with g * scale, or stores nothing when a non-finite gradient is to be skipped: the tensors, the moments and the step count then keep
their bits.  All of it on the device, still capturable.  The scale is ``clip / max(norm, clip)`` from a float64 norm summed in a fixed
order; TensorFlow's ``clip_by_global_norm`` takes ``clip * min(1 / norm, 1 / clip)`` in float32 from a float32 reduction of unspecified
order, so bit parity with a Keras ``global_clipnorm`` is not available and not claimed.  A guarded step that neither clips nor skips has
the bits of the unguarded one.  With both options at their defaults ``step()`` is the unguarded code path, launch for launch."""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict

import numpy as np

from . import _lib


def _f32(x):
    return float(np.float32(x))


def layer_segments(kind, lib=None):
    """the per-layer statistics table of one of the trainers' flat tensors, from the library's own layout calls: kind "regressor"
    (hpe_regressor_param_offset: kernel and bias of the three Dense layers, then mean theta), "encoder" (hpe_encoder_param_offset: kernel,
    bias, gamma, beta of the 53 conv layers) or "critic" (hpe_critic_param_offset: kernel and bias of the nine Dense layers).
    -> (offsets, layers): S + 1 ascending offsets covering the whole tensor, and the layer name of each of the S segments"""
    from .critic_spec import CRITIC_LAYERS
    from .resnet_spec import CONV_SPECS

    lib = lib or _lib.load()
    if kind == "regressor":
        parts = [("dense_%d" % i, lib.hpe_regressor_param_offset(i, b)) for i in range(3) for b in (0, 1)]
        parts.append(("mean_theta", lib.hpe_regressor_param_offset(3, 0)))
        total = lib.hpe_regressor_param_floats()
    elif kind == "encoder":
        parts = [(s.name, lib.hpe_encoder_param_offset(i, w)) for i, s in enumerate(CONV_SPECS) for w in range(4)]
        total = lib.hpe_encoder_param_floats()
    elif kind == "critic":
        parts = [(name, lib.hpe_critic_param_offset(i, b)) for i, (name, _fi, _fo) in enumerate(CRITIC_LAYERS) for b in (0, 1)]
        total = lib.hpe_critic_param_floats()
    else:
        raise ValueError("kind must be 'regressor', 'encoder' or 'critic'")
    offsets = [o for _n, o in parts] + [total]
    if offsets[0] != 0 or any(b < a for a, b in zip(offsets[:-1], offsets[1:])):
        raise RuntimeError("layer_segments: the library's %s offsets do not ascend from 0" % kind)
    return offsets, [n for n, _o in parts]


class KerasAdam(object):
    GUARD_FIELDS = ("norm", "scale", "applied", "skipped", "clipped", "nonfinite", "maxabs", "sumsq")  # the guard block (include/hpe.h)
    MAX_GUARDED_TENSORS = 16  # record lists one hpe_adam_guard takes

    def __init__(self, lr, beta_1=0.9, beta_2=0.999, eps=1e-7, global_clipnorm=None, skip_nonfinite=False):
        if not (0.0 <= beta_1 < 1.0 and 0.0 <= beta_2 < 1.0):
            raise ValueError("beta_1 and beta_2 must be in [0, 1)")
        if not eps >= 0.0:
            raise ValueError("eps must be >= 0")
        if global_clipnorm is not None and not float(global_clipnorm) >= 0.0:
            raise ValueError("global_clipnorm must be >= 0")
        self.lr, self.beta_1, self.beta_2, self.eps = float(lr), float(beta_1), float(beta_2), float(eps)
        self.global_clipnorm = None if global_clipnorm is None else float(global_clipnorm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.guarded = self.global_clipnorm is not None or self.skip_nonfinite
        self.segments = OrderedDict()  # name -> the S + 1 offsets (numpy int64) of its statistics records
        self._stats = {}  # name -> (offsets on the device, records [S,3], workspace, its bytes): guarded optimisers only
        self._guard = None  # 8 doubles on the device, GUARD_FIELDS
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
            if self.guarded:
                self._guard = torch.zeros(len(self.GUARD_FIELDS), dtype=torch.float64, device=like.device)
            if self._pending_t:
                self._set_step(self._pending_t)
        return self._state

    def _set_step(self, t):
        _lib.check(self.lib.hpe_adam_set_step(self._state.data_ptr(), int(t), self.beta_1, self.beta_2, self._stream(self._state)))

    def add(self, name, flat_tensor, segments=None):
        """register a flat (1-D, contiguous, float32) CUDA parameter tensor; its moments ``m`` and ``v`` start as zeros.  segments: S + 1
        ascending offsets into it, the table of the gradient statistics a guarded step takes (``grad_stats``); default: one segment,
        the whole tensor.  The global norm is that of the elements the table covers."""
        import torch

        t = flat_tensor
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 1 or not t.is_contiguous():
            raise ValueError("%s must be a flat contiguous float32 CUDA tensor" % name)
        if name in self.params:
            raise ValueError("%s is registered already" % name)
        off = np.array([0, t.numel()] if segments is None else [int(o) for o in segments], dtype=np.int64)
        if off.ndim != 1 or off.size < 2 or off[0] < 0 or off[-1] > t.numel() or (np.diff(off) < 0).any():
            raise ValueError("segments of %s must be S + 1 >= 2 ascending offsets in [0, %d]" % (name, t.numel()))
        self.segments[name] = off
        if self.guarded:
            S = off.size - 1
            nbytes = int(self.lib.hpe_grad_stats_workspace_bytes(t.numel(), S))
            if nbytes < 0:
                _lib.check(1)  # HPE_ERR_INVALID: hpe_last_error() says why
            self._stats[name] = (torch.from_numpy(off).to(t.device), torch.zeros((S, 3), dtype=torch.float64, device=t.device),
                                 torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=t.device), nbytes)
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
        omb1, omb2, eps = self.one_minus_beta_1, self.one_minus_beta_2, _f32(self.eps)
        if self.guarded:
            return self._guarded_step(todo, grads, stream, omb1, omb2, eps)
        _lib.check(self.lib.hpe_adam_advance(st.data_ptr(), self.lr, self.beta_1, self.beta_2, stream))
        for (name, p), g in zip(todo, grads):
            s = self.slots[name]
            _lib.check(self.lib.hpe_adam_apply(p.data_ptr(), s["m"].data_ptr(), s["v"].data_ptr(), g.data_ptr(), p.numel(), st.data_ptr(),
                                               omb1, omb2, eps, stream))

    def _guarded_step(self, todo, grads, stream, omb1, omb2, eps):
        """hpe_grad_stats per stepped tensor, one hpe_adam_guard on their records (in the order of registration), hpe_adam_apply_guarded
        per tensor"""
        if len(todo) > self.MAX_GUARDED_TENSORS:
            raise ValueError("a guarded step takes at most %d tensors" % self.MAX_GUARDED_TENSORS)
        st, gd = self._state, self._guard
        recs, counts = (C.c_void_p * len(todo))(), (C.c_int * len(todo))()
        for i, ((name, p), g) in enumerate(zip(todo, grads)):
            off_dev, rec, ws, nbytes = self._stats[name]
            off = self.segments[name]
            _lib.check(self.lib.hpe_grad_stats(g.data_ptr(), g.numel(), off.ctypes.data, off_dev.data_ptr(), off.size - 1, rec.data_ptr(),
                                               ws.data_ptr(), nbytes, stream))
            recs[i], counts[i] = rec.data_ptr(), off.size - 1
        clip = float("inf") if self.global_clipnorm is None else self.global_clipnorm
        _lib.check(self.lib.hpe_adam_guard(st.data_ptr(), gd.data_ptr(), recs, counts, len(todo), self.lr, self.beta_1, self.beta_2, clip,
                                           int(self.skip_nonfinite), stream))
        for (name, p), g in zip(todo, grads):
            s = self.slots[name]
            _lib.check(self.lib.hpe_adam_apply_guarded(p.data_ptr(), s["m"].data_ptr(), s["v"].data_ptr(), g.data_ptr(), p.numel(), st.data_ptr(),
                                                       gd.data_ptr(), omb1, omb2, eps, stream))

    def _guard_view(self, field):
        if self._guard is None:
            raise RuntimeError("KerasAdam: not a guarded optimiser (global_clipnorm= / skip_nonfinite=), or no tensor registered yet")
        return self._guard[self.GUARD_FIELDS.index(field)]

    def grad_stats(self, name):
        """the device records [S,3] float64 of ``name``'s last guarded step, one per registered segment: (sum of squares, largest |g|
        over the finite elements, number of non-finite elements).  A view: the next step overwrites it.  A record's bits depend on its
        segment's values alone, but two segmentations of one tensor add in different orders: their sums agree to rounding, not in bits."""
        if name not in self._stats:
            raise KeyError("no gradient statistics for %s (a guarded optimiser keeps them per registered tensor)" % name)
        return self._stats[name][1]

    @property
    def grad_norm(self):
        """0-dim float64 device view: the global gradient norm of the last guarded step, before clipping"""
        return self._guard_view("norm")

    @property
    def clip_scale(self):
        """0-dim float64 device view: the float32 factor the last guarded step multiplied its gradients by (0 on a skipped step)"""
        return self._guard_view("scale")

    @property
    def step_applied(self):
        """0-dim float64 device view: 1 if the last guarded step was applied, 0 if it was skipped"""
        return self._guard_view("applied")

    @property
    def skipped_steps(self):
        """steps skipped for a non-finite gradient in this run; reads the device (synchronises), as ``iterations`` does"""
        return 0 if self._guard is None else int(self._guard_view("skipped").item())

    @property
    def clipped_steps(self):
        """steps whose gradients were scaled down in this run; reads the device (synchronises)"""
        return 0 if self._guard is None else int(self._guard_view("clipped").item())

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
