"""HpeEngine: thin owner of one ``hpe_ctx`` (include/hpe.h) -- asset ingestion from Keras-layout dicts and
torch-tensor plumbing around the C-ABI calls.  PyTorch is used for device memory, streams and (in
``distributed.py``) the RCCL process group only; every numerical stage runs in libhpe_hip.so.
"""
from __future__ import annotations

import collections
import ctypes as C

import numpy as np

from . import _lib
from .critic_spec import PARAM_FLOATS
from .regressor_spec import PARAM_FLOATS as REGRESSOR_PARAM_FLOATS
from .resnet_spec import CONV_SPECS, ENCODER_PARAM_FLOATS, ENCODER_STAT_FLOATS

NUM_VERTS = _lib.NUM_VERTS


def _torch():
    import torch

    return torch


def _require_cuda_tensor(t, name, shape_tail=None):
    torch = _torch()
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor on the GPU" % name)
    if not t.is_cuda:
        raise ValueError("%s must live on the GPU (got %s); there is no CPU path" % (name, t.device))
    if t.dtype != torch.float32:
        raise TypeError("%s must be float32 (got %s)" % (name, t.dtype))
    if shape_tail is not None and tuple(t.shape[1:]) != tuple(shape_tail):
        raise ValueError("%s must have shape [B,%s], got %s" % (name, ",".join(map(str, shape_tail)), tuple(t.shape)))
    return t.contiguous()


def _require_bf16_tensor(t, name):
    torch = _torch()
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError("%s must be a torch.Tensor on the GPU" % name)
    if t.dtype != torch.bfloat16:
        raise TypeError("%s must be bfloat16 (got %s)" % (name, t.dtype))
    return t.contiguous()


def _ptr(t):
    """device address of an optional tensor: None crosses the ABI as a null pointer"""
    return t.data_ptr() if t is not None else None


def _flat_arg(t, n, name):
    """-> t as a flat float32 CUDA tensor of exactly n elements"""
    t = _require_cuda_tensor(t.detach(), name)
    if tuple(t.shape) != (n,):
        raise ValueError("%s must be [%d], got %s" % (name, n, tuple(t.shape)))
    return t


class _Prec(collections.namedtuple("_Prec", "suffix dtype check forward")):
    """What differs between the encoder's fp32 and mixed-precision training calls, the counterpart of Prec<T> in csrc/encoder_train.hip:
    the suffix of the C symbols (_lib.ENCODER_ENTRY), the torch dtype of activations and cotangents (by name), the checker of such an
    argument and the words the "no ... has run" errors use for the forward.  Everything else is float32 in both precisions: the images
    (so layer 0's x), features, statistics, grad_layer, grad_flat, and the pooled cotangent ``dy`` of ``debug_avgpool_backward``."""
    __slots__ = ()

    def act(self, t, name, idx=None, optional=False):
        """an activation or cotangent argument (optional: or None) checked; ``x`` of layer idx 0 is the float32 images"""
        if t is None and optional:
            return None
        return _require_cuda_tensor(t, name) if idx == 0 else self.check(t, name)

    def new(self, engine, *shape):
        """an uninitialised activation or cotangent tensor on the engine's device"""
        return engine._new(*shape, dtype=self.dtype)


_FP32 = _Prec("", "float32", _require_cuda_tensor, "training forward")
_MIXED = _Prec("_mixed", "bfloat16", _require_bf16_tensor, "mixed-precision training forward")


class HpeEngine(object):
    def __init__(self, device=0, max_batch=8, num_stage=3, bn_eps=1e-3, encoder_dtype="fp32", **plan_options):
        """plan_options: the HpeConfig plan fields of include/hpe.h (n_streams, dual_gemm, stem_fused, wino_min_c, wino_min_items,
        wino_fused, wino_fused_min_hw, mesh_a2b, wino_f4, wino4_fused, bf16_p8, wino4_ksplit, chain_fuse, halo3, f32_split); unset = -1 = the library default (environment variable, else built-in).
        They select WHICH kernels run, per context -- two engines with different options can coexist in one process."""
        self.lib = _lib.load()
        torch = _torch()
        if not torch.cuda.is_available():
            raise _lib.HpeError("no GPU visible: the HIP path is the only path (no CPU fallback)")
        self.device = int(device)
        self.max_batch = int(max_batch)
        self.num_stage = int(num_stage)
        self.num_kp = 19
        if encoder_dtype not in ("fp32", "bf16"):
            raise ValueError("encoder_dtype must be 'fp32' or 'bf16'")
        self.encoder_dtype = encoder_dtype
        cfg = _lib.HpeConfig()
        self.lib.hpe_config_init(C.byref(cfg))
        cfg.device, cfg.max_batch, cfg.num_stage, cfg.bn_eps = self.device, self.max_batch, self.num_stage, float(bn_eps)
        cfg.encoder_dtype = 1 if encoder_dtype == "bf16" else 0
        for k, v in plan_options.items():
            if k not in _lib.PLAN_OPTIONS:
                raise TypeError("unknown plan option %r (known: %s)" % (k, ", ".join(_lib.PLAN_OPTIONS)))
            if k == "mesh_a2b" and isinstance(v, str):
                v = {"grid": 0, "valu": 1, "mfma": 2}[v]
            setattr(cfg, k, int(v))
        self.plan_options = dict(plan_options)
        self._cfg = cfg
        h = C.c_void_p()
        _lib.check(self.lib.hpe_create(C.byref(cfg), C.byref(h)))
        self._h = h
        self._finalized = False
        self._has_critic = False
        self.tdev = torch.device("cuda", self.device)

    # ------------------------------------------------------------------ ingestion
    def load_smpl(self, model, joint_type="cocoplus"):
        """model: dict with the reference pickle's keys (src/tf_smpl/batch_smpl.py:31-81); scipy-sparse
        regressors and chumpy-like objects (``.r``) are densified here exactly as the reference does."""

        def dense(x):
            if hasattr(x, "todense"):
                x = np.asarray(x.todense())
            elif hasattr(x, "r") and not isinstance(x, np.ndarray):
                x = np.asarray(x.r)
            return np.asarray(x)

        if joint_type not in ("cocoplus", "lsp"):
            raise ValueError('BAD!! Unknown joint type: %s, it must be either "cocoplus" or "lsp"' % joint_type)
        kp = dense(model["cocoplus_regressor"])
        if joint_type == "lsp":
            kp = kp[:14]
        parents = np.ascontiguousarray(np.asarray(model["kintree_table"])[0].astype(np.int64).astype(np.int32))
        parents[parents < 0] = -1
        parents[0] = -1  # uint32(-1) -> int32 (batch_smpl.py:65)
        keep = [_lib.f32(dense(model[k])) for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "weights")]
        keep.append(_lib.f32(kp))
        if keep[0][0].shape != (NUM_VERTS, 3) or keep[1][0].shape != (NUM_VERTS, 3, 10) or keep[2][0].shape != (NUM_VERTS, 3, 207):
            raise ValueError("SMPL arrays have unexpected shapes")
        if keep[3][0].shape != (24, NUM_VERTS) or keep[4][0].shape != (NUM_VERTS, 24) or keep[5][0].shape[1] != NUM_VERTS:
            raise ValueError("SMPL regressor/weight arrays have unexpected shapes")
        m = _lib.HpeSmplModel(*[k[1] for k in keep], parents.ctypes.data_as(C.c_void_p), int(kp.shape[0]))
        _lib.check(self.lib.hpe_load_smpl(self._h, C.byref(m)))
        self.num_kp = int(kp.shape[0])

    def load_encoder(self, params):
        """params: {'<layer>/kernel' HWIO, '<layer>/bias', '<bn>/gamma|beta|moving_mean|moving_variance'}"""
        for i, s in enumerate(CONV_SPECS):
            arrs = [
                _lib.f32(params[s.name + "/kernel"]),
                _lib.f32(params[s.name + "/bias"]),
                _lib.f32(params[s.bn_name + "/gamma"]),
                _lib.f32(params[s.bn_name + "/beta"]),
                _lib.f32(params[s.bn_name + "/moving_mean"]),
                _lib.f32(params[s.bn_name + "/moving_variance"]),
            ]
            if arrs[0][0].shape != (s.kh, s.kw, s.cin, s.cout):
                raise ValueError("%s/kernel must be HWIO %s, got %s" % (s.name, (s.kh, s.kw, s.cin, s.cout), arrs[0][0].shape))
            _lib.check(self.lib.hpe_load_conv(self._h, i, *[a[1] for a in arrs]))

    def load_regressor(self, params):
        dims = [(2133, 1024), (1024, 1024), (1024, 85)]
        for i, d in enumerate(dims):
            k = _lib.f32(params["dense_%d/kernel" % i])
            b = _lib.f32(params["dense_%d/bias" % i])
            if k[0].shape != d:
                raise ValueError("dense_%d/kernel must be %s" % (i, d))
            _lib.check(self.lib.hpe_load_dense(self._h, i, k[1], b[1]))

    def load_mean_theta(self, mean85):
        m = _lib.f32(np.asarray(mean85).reshape(-1))
        if m[0].shape != (85,):
            raise ValueError("mean theta must have 85 entries")
        _lib.check(self.lib.hpe_load_mean_theta(self._h, m[1]))

    def load_critic(self, params):
        """params: {'critic/<layer name>/kernel' [in,out], 'critic/<layer name>/bias' [out]} for the nine Dense layers of
        CriticNetwork (hpe_critic_layer_name); valid before or after ``finalize``, loading again replaces the weights."""
        m = _lib.HpeCriticModel()
        keep = []
        shape = (C.c_int * 2)()
        for i in range(_lib.NUM_CRITIC_DENSE):
            name = self.lib.hpe_critic_layer_name(i).decode()
            _lib.check(self.lib.hpe_critic_layer_shape(i, shape))
            try:
                k = _lib.f32(params["critic/%s/kernel" % name])
                b = _lib.f32(params["critic/%s/bias" % name])
            except KeyError as e:
                raise KeyError("critic weights lack %s" % e) from None
            if k[0].shape != (shape[0], shape[1]) or b[0].shape != (shape[1],):
                raise ValueError("critic/%s: kernel must be %s and bias (%d,), got %s and %s" % (name, (shape[0], shape[1]), shape[1], k[0].shape, b[0].shape))
            keep += [k, b]
            m.kernel[i], m.bias[i] = k[1].value, b[1].value
        _lib.check(self.lib.hpe_load_critic(self._h, C.byref(m)))
        self._has_critic = True

    @property
    def has_critic(self):
        """a critic is loaded in the live ctx (a failed ``finalize`` releases it with the rest of the device state; ``close`` ends it)"""
        return self._has_critic

    def finalize(self):
        rc = self.lib.hpe_finalize(self._h)
        if rc not in (0, 3):  # a device-side failure leaves the ctx dead, the critic's device copy released (3 = call order: nothing touched)
            self._has_critic = False
        _lib.check(rc)
        self._finalized = True

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.hpe_destroy(self._h)
            self._h = C.c_void_p()
            self._has_critic = False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ helpers
    def _stream(self):
        return C.c_void_p(_torch().cuda.current_stream(self.tdev).cuda_stream)

    def _new(self, *shape, dtype="float32"):
        return _torch().empty(shape, dtype=getattr(_torch(), dtype), device=self.tdev)

    def _output_shapes(self, B):
        return {
            "verts": (B, NUM_VERTS, 3),
            "joints": (B, self.num_kp, 3),
            "cams": (B, 3),
            "theta": (B, 85),
            "J_transformed": (B, 24, 3),
            "kp2d": (B, self.num_kp, 2),
            "verts2d": (B, NUM_VERTS, 2),
            "Rs": (B, 24, 3, 3),
        }

    def _alloc_outputs(self, B, want):
        shapes = self._output_shapes(B)
        tensors = {k: self._new(*shapes[k]) for k in want}
        o = _lib.HpeOutputs(*[_ptr(tensors.get(k)) for k in _lib.OUTPUT_FIELDS])
        return tensors, o

    def _output_sets(self, B, want, n_outs):
        """-> (outs, arr): n_outs freshly allocated output dicts and the HpeOutputs array that names their buffers"""
        outs, arr = [], (_lib.HpeOutputs * n_outs)()
        for i in range(n_outs):
            t, arr[i] = self._alloc_outputs(B, want)
            outs.append(t)
        return outs, arr

    # ------------------------------------------------------------------ compute
    DEFAULT_OUTPUTS = ("verts", "joints", "cams", "theta", "J_transformed", "kp2d")

    def forward(self, images, all_stages=False, want=DEFAULT_OUTPUTS, pipelined=False):
        """images [B,224,224,3] cuda float32 -> list (one dict per returned stage) of output tensors.
        pipelined=True: hpe_forward_pipelined (the outputs are complete after ``join()``); used by Predictor.predict for inputs
        larger than config.batch_size, whose chunks then overlap tail and encoder.  The ctx's tail stream writes the outputs and
        torch's caching allocator does not know that stream: keep the returned tensors alive until ``join()`` has been called
        (they are also marked with ``record_stream`` for the tail stream, so a tensor dropped early is not recycled under it)."""
        images = _require_cuda_tensor(images, "images", (224, 224, 3))
        B = images.shape[0]
        n_outs = self.num_stage if all_stages else 1
        outs, arr = self._output_sets(B, want, n_outs)
        fwd = self.lib.hpe_forward_pipelined if pipelined else self.lib.hpe_forward
        if pipelined:
            ts = self.tail_stream()
            for t in outs:
                for v in t.values():
                    v.record_stream(ts)
        _lib.check(fwd(self._h, images.data_ptr(), B, arr, n_outs, self._stream()))
        return outs

    def tail(self, features, all_stages=False, want=DEFAULT_OUTPUTS):
        """The regressor + SMPL half alone (hpe_tail): features [B,2048] from ``encoder()`` -> list of per-stage output dicts."""
        features = _require_cuda_tensor(features, "features", (2048,))
        B = features.shape[0]
        n_outs = self.num_stage if all_stages else 1
        outs, arr = self._output_sets(B, want, n_outs)
        _lib.check(self.lib.hpe_tail(self._h, features.data_ptr(), B, arr, n_outs, self._stream()))
        return outs

    def make_overlapped_plan(self, B, all_stages=False, want=DEFAULT_OUTPUTS, graph=False, tail_extra=None, n_sets=2):
        """Steady-state serving as ONE stream-ordered, hipGraph-capturable step per batch (hpe_encoder + hpe_tail):

            step(images_k)  =  fork;  side stream: tail(features of batch k-1) [+ tail_extra(outs)]  ||  encoder(images_k);  join

        i.e. the software pipeline of ``hpe_forward_pipelined`` with the overlap INSIDE the step instead of across calls, so that
        the whole step (every launch of both branches, the fork / join of the encoder's chunk streams and of the side stream) can
        be captured once and replayed with one host call.  ``step(images)`` returns the output set of the PREVIOUS batch (None
        on the first call); ``flush()`` runs the tail of the last batch alone and returns its outputs.  Features alternate
        between two buffers and outputs between ``n_sets`` sets; ``tail_extra(outs, set_index)`` (e.g. the loss call) is enqueued
        on the side stream after the tail, inside the capture.  graph=True: two graphs (one per feature buffer parity) per output
        set rotation are captured after an eager warm-up; images are copied into a static input buffer."""
        torch = _torch()
        n_outs = self.num_stage if all_stages else 1
        sets = [self._output_sets(B, want, n_outs) for _ in range(n_sets)]
        feats = [self._new(B, 2048) for _ in range(2)]
        # the side branch runs on the ctx's own tail stream: a process should keep <= 4 busy HIP streams ("hardware queues")
        side = self.tail_stream()
        lib, h = self.lib, self._h
        state = {"k": 0}

        def enqueue(images, k, with_tail, with_enc):
            cur = torch.cuda.current_stream(self.tdev)
            if with_tail:
                side.wait_stream(cur)
                with torch.cuda.stream(side):
                    outs, arr = sets[(k - 1) % n_sets]
                    _lib.check(lib.hpe_tail(h, feats[(k - 1) & 1].data_ptr(), B, arr, n_outs, C.c_void_p(side.cuda_stream)))
                    if tail_extra is not None:
                        tail_extra(outs, (k - 1) % n_sets)
            if with_enc:
                _lib.check(lib.hpe_encoder(h, images.data_ptr(), B, feats[k & 1].data_ptr(), self._stream()))
            if with_tail:
                cur.wait_stream(side)

        run = enqueue  # run(images, k, with_tail, with_enc): step k of the pipeline, eagerly or (below) as the replay of its graph
        if graph:
            static_in = torch.zeros((B, 224, 224, 3), dtype=torch.float32, device=self.tdev)
            self.enable_timing(0)  # event timing cannot be captured
            # eager warm-up of every launch shape (lazy module loading, workspace growth) before capture
            enqueue(static_in, 0, False, True)
            enqueue(static_in, 1, True, True)
            enqueue(None, 2, True, False)
            torch.cuda.synchronize(self.tdev)
            period = 2 * n_sets // (2 if n_sets % 2 == 0 else 1)  # lcm(2, n_sets): (feature parity, output set) repeats with this period

            def capture(k, with_tail, with_enc):
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    enqueue(static_in, k, with_tail, with_enc)
                return g

            g_first = capture(0, False, True)
            g_steady = [capture(period + r, True, True) for r in range(period)]  # index r == k % period, k >= 1
            g_flush = [capture(period + r, True, False) for r in range(period)]

            def replay(images, k, with_tail, with_enc):
                if with_enc:
                    static_in.copy_(images, non_blocking=True)
                (g_first if not with_tail else g_steady[k % period] if with_enc else g_flush[k % period]).replay()

            run = replay

        def step(images):
            k = state["k"]
            run(images, k, k > 0, True)
            state["k"] = k + 1
            if k > 0:
                step.last = (k - 1) % n_sets
            return sets[(k - 1) % n_sets][0] if k > 0 else None

        def flush():
            k = state["k"]
            if k == 0:
                return None
            run(None, k, True, False)
            state["k"] = 0
            step.last = (k - 1) % n_sets
            return sets[(k - 1) % n_sets][0]

        step.flush = flush
        step.last = None  # index (into step.sets) of the output set of the most recently completed batch
        step.sets = [s_[0] for s_ in sets]
        if graph:
            step.graphs = (g_first, g_steady, g_flush)  # keep alive
        return step

    def tail_stream(self):
        """torch view of the ctx's tail stream (hpe_tail_stream): consumers of a pipelined plan's outputs enqueue there."""
        torch = _torch()
        ptr = self.lib.hpe_tail_stream(self._h)
        if not ptr:
            raise _lib.HpeError("no tail stream (ctx not finalized)")
        return torch.cuda.ExternalStream(ptr, device=self.tdev)

    def join(self):
        """Make the current stream wait for the tail of the last pipelined forward (hpe_join)."""
        _lib.check(self.lib.hpe_join(self._h, self._stream()))

    def make_forward_plan(self, B, all_stages=False, want=DEFAULT_OUTPUTS, graph=False, pipelined=False):
        """Pre-allocate outputs once; returns (callable(images), outputs) -- the steady-state serving path.
        graph=True captures the whole forward (all kernel launches, including the fork/join of the batch-chunk streams)
        into a hipGraph through torch.cuda.CUDAGraph: the callable then copies `images` into a static input buffer and
        replays the graph -- one host call per batch instead of ~75 launches (what matters for small batches).
        pipelined=True uses hpe_forward_pipelined (steady-state throughput: the tail of batch k overlaps the encoder of batch
        k+1); the caller reads the outputs after ``join()`` or from work enqueued on ``tail_stream()``."""
        torch = _torch()
        n_outs = self.num_stage if all_stages else 1
        outs, arr = self._output_sets(B, want, n_outs)
        lib, h = self.lib, self._h
        fwd = lib.hpe_forward_pipelined if pipelined else lib.hpe_forward
        if pipelined and graph:
            raise ValueError("a pipelined plan cannot be captured into a graph")

        def launch(images):
            # pipelined: encoder on the current stream, regressor + SMPL tail on the ctx's tail stream (outputs valid after
            # join(), or for work enqueued on tail_stream()); the next call's encoder overlaps this call's tail
            _lib.check(fwd(h, images.data_ptr(), B, arr, n_outs, self._stream()))

        if not graph:

            def run(images):
                launch(images)
                return outs

            return run, outs

        static_in = torch.zeros((B, 224, 224, 3), dtype=torch.float32, device=self.tdev)
        self.enable_timing(0)  # event timing cannot be captured
        side = torch.cuda.Stream(device=self.tdev)
        side.wait_stream(torch.cuda.current_stream(self.tdev))
        with torch.cuda.stream(side):  # warm-up outside capture (lazy allocations such as module loading)
            launch(static_in)
        torch.cuda.current_stream(self.tdev).wait_stream(side)
        torch.cuda.synchronize(self.tdev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            launch(static_in)

        def run_graph(images):
            static_in.copy_(images, non_blocking=True)
            g.replay()
            return outs

        run_graph.graph = g  # keep alive
        return run_graph, outs

    def encoder(self, images):
        images = _require_cuda_tensor(images, "images", (224, 224, 3))
        feat = self._new(images.shape[0], 2048)
        _lib.check(self.lib.hpe_encoder(self._h, images.data_ptr(), images.shape[0], feat.data_ptr(), self._stream()))
        return feat

    def regress_stage(self, features, theta_prev=None):
        features = _require_cuda_tensor(features, "features", (2048,))
        B = features.shape[0]
        if theta_prev is not None:
            theta_prev = _require_cuda_tensor(theta_prev, "theta_prev", (85,))
        out = self._new(B, 85)
        _lib.check(self.lib.hpe_regress_stage(self._h, features.data_ptr(), _ptr(theta_prev), B, out.data_ptr(), self._stream()))
        return out

    def smpl(self, theta, want=("verts", "joints", "J_transformed", "kp2d", "Rs")):
        """hpe_smpl on theta rows [B,85].  A theta that requires grad goes through ``autograd.SmplFunction`` (the outputs then
        backpropagate through hpe_smpl_backward); any other theta takes the plain call below."""
        if _torch().is_grad_enabled() and isinstance(theta, _torch().Tensor) and theta.requires_grad:
            from .autograd import smpl_with_grad

            return smpl_with_grad(self, theta, tuple(want))
        theta = _require_cuda_tensor(theta, "theta", (85,))
        B = theta.shape[0]
        t, o = self._alloc_outputs(B, want)
        _lib.check(self.lib.hpe_smpl(self._h, theta.data_ptr(), B, C.byref(o), self._stream()))
        return t

    def smpl_backward(self, theta, grads):
        """Gradient of ``smpl`` (hpe_smpl_backward): theta [B,85], grads {output name: cotangent tensor of that output's shape}
        (a missing name or None = zero) -> grad_theta [B,85].  Any B: chunks of max_batch images, as SMPL.__call__ does."""
        torch = _torch()
        theta = _require_cuda_tensor(theta.detach(), "theta", (85,))
        B = theta.shape[0]
        shapes = self._output_shapes(B)
        g = {}
        for k, v in grads.items():
            if k not in shapes:
                raise KeyError("unknown output %r (known: %s)" % (k, ", ".join(_lib.OUTPUT_FIELDS)))
            if v is None:
                continue
            v = _require_cuda_tensor(v.detach(), "grads[%r]" % k)
            if tuple(v.shape) != shapes[k]:
                raise ValueError("grads[%r] must have shape %s, got %s" % (k, shapes[k], tuple(v.shape)))
            g[k] = v
        out = self._new(B, 85)
        mb = self.max_batch
        for lo in range(0, B, mb):
            n = min(mb, B - lo)
            o = _lib.HpeOutputs(*[_ptr(g[k][lo : lo + n] if k in g else None) for k in _lib.OUTPUT_FIELDS])
            _lib.check(self.lib.hpe_smpl_backward(self._h, theta[lo : lo + n].data_ptr(), n, C.byref(o), out[lo : lo + n].data_ptr(), self._stream()))
        return out

    def _critic_inputs(self, joints, betas, Rs):
        """-> (joints, betas, Rs, N, K, betas_stride): joints [N,K,3] and Rs [N,24,3,3] contiguous; betas [N,10] with unit column
        stride is used in place whatever its row stride (theta[:, 75:] is not copied)."""
        joints = _require_cuda_tensor(joints.detach(), "joints")
        Rs = _require_cuda_tensor(Rs.detach(), "Rs", (24, 3, 3))
        betas = betas.detach()
        if not betas.is_cuda or betas.dtype != _torch().float32 or betas.dim() != 2 or betas.shape[1] != 10:
            raise ValueError("betas must be a float32 CUDA tensor [N,10]")
        N = joints.shape[0]
        if joints.dim() != 3 or joints.shape[2] != 3 or not 14 <= joints.shape[1] <= 24:
            raise ValueError("joints must be [N,K,3] with 14 <= K <= 24, got %s" % (tuple(joints.shape),))
        if betas.shape[0] != N or Rs.shape[0] != N or N < 1:
            raise ValueError("joints, betas and Rs must have the same number (>= 1) of rows")
        if betas.stride(1) != 1 or (N > 1 and betas.stride(0) < 10):
            betas = betas.contiguous()
        stride = betas.stride(0) if N > 1 else 10
        return joints, betas, Rs, N, joints.shape[1], stride

    @staticmethod
    def _grad_scores(grad_scores, N):
        """-> grad_scores as a float32 CUDA tensor [N,3], or None"""
        if grad_scores is None:
            return None
        gs = _require_cuda_tensor(grad_scores.detach(), "grad_scores", (3,))
        if gs.shape[0] != N:
            raise ValueError("grad_scores must be [N,3]")
        return gs

    def critic(self, joints, betas, Rs, want_kcs=False):
        """hpe_critic: joints [N,K,3] (the first 14 are read), betas [N,10], Rs [N,24,3,3] (the root is skipped) -> scores [N,3]
        = (joints + KCS, shapes, rotations); want_kcs=True returns (scores, kcs [N,13,13]).  Any N."""
        joints, betas, Rs, N, K, stride = self._critic_inputs(joints, betas, Rs)
        scores = self._new(N, 3)
        kcs = self._new(N, 13, 13) if want_kcs else None
        _lib.check(self.lib.hpe_critic(self._h, joints.data_ptr(), K, betas.data_ptr(), stride, Rs.data_ptr(), N, scores.data_ptr(), _ptr(kcs),
                                       self._stream()))
        return (scores, kcs) if want_kcs else scores

    def critic_backward(self, joints, betas, Rs, grad_scores=None, want=("joints", "betas", "Rs")):
        """hpe_critic_backward: the gradient of sum(grad_scores * scores) (grad_scores [N,3]; None = ones) with respect to the inputs
        named in ``want`` (among joints [N,K,3], betas [N,10], Rs [N,24,3,3], kcs [N,13,13]) -> dict.  'joints' is the total
        derivative, 'kcs' the partial one with KCS held as an independent input."""
        shapes_of = {"joints": None, "betas": (10,), "Rs": (24, 3, 3), "kcs": (13, 13)}
        unknown = [k for k in want if k not in shapes_of]
        if unknown or not want:
            raise ValueError("want must name some of %s, got %r" % (sorted(shapes_of), tuple(want)))
        joints, betas, Rs, N, K, stride = self._critic_inputs(joints, betas, Rs)
        shapes_of["joints"] = (K, 3)
        gs = self._grad_scores(grad_scores, N)
        out = {k: self._new(N, *shapes_of[k]) for k in want}
        ptr = [_ptr(out.get(k)) for k in ("joints", "betas", "Rs", "kcs")]
        _lib.check(self.lib.hpe_critic_backward(self._h, joints.data_ptr(), K, betas.data_ptr(), stride, Rs.data_ptr(), N, _ptr(gs), *ptr,
                                                self._stream()))
        return out

    _TANGENT_SHAPES = {"kcs": (13, 13), "joints": (14, 3), "betas": (10,), "Rs": (23, 3, 3)}

    def critic_weight_grad(self, joints, betas, Rs, grad_scores=None, tangents=None):
        """hpe_critic_weight_grad: the gradient with respect to the critic's weights of

            F = sum_n [ sum_c grad_scores[n,c] * scores[n,c] + < t_n , d(sum_c scores[n,c]) / d x_n > ]

        as one flat tensor [critic_spec.PARAM_FLOATS] (kernel 0, bias 0, kernel 1, ...).  grad_scores [N,3] or None (no first-order
        term); tangents: {name: tensor} for some of kcs (13,13), joints (14,3), betas (10,), Rs (23,3,3) -- the root is left out --
        either all of exactly that shape (one tangent shared by all rows: the reference's gradient penalty) or all with a leading N
        (one per row).  The result is a sum over the rows in a fixed order: same inputs, same bits."""
        joints, betas, Rs, N, K, stride = self._critic_inputs(joints, betas, Rs)
        gs = self._grad_scores(grad_scores, N)
        tangents = {k: v for k, v in (tangents or {}).items() if v is not None}
        unknown = [k for k in tangents if k not in self._TANGENT_SHAPES]
        if unknown:
            raise ValueError("tangents must name some of %s, got %r" % (sorted(self._TANGENT_SHAPES), unknown))
        if gs is None and not tangents:
            raise ValueError("critic_weight_grad needs grad_scores or a tangent")
        per_row, keep = None, {}
        for k, v in tangents.items():
            base = self._TANGENT_SHAPES[k]
            v = _require_cuda_tensor(v.detach(), "tangents[%r]" % k)
            if tuple(v.shape) == base:
                row = False
            elif tuple(v.shape) == (N,) + base:
                row = True
            else:
                raise ValueError("tangents[%r] must be %s or %s, got %s" % (k, base, (N,) + base, tuple(v.shape)))
            if per_row is not None and row != per_row:
                raise ValueError("tangents must be all shared or all per row")
            per_row = row
            keep[k] = v
        out = self._new(PARAM_FLOATS)
        ptr = [_ptr(keep.get(k)) for k in ("kcs", "joints", "betas", "Rs")]
        _lib.check(self.lib.hpe_critic_weight_grad(self._h, joints.data_ptr(), K, betas.data_ptr(), stride, Rs.data_ptr(), N, _ptr(gs), *ptr,
                                                   1 if per_row else 0, out.data_ptr(), self._stream()))
        return out

    def critic_reserve(self, N):
        """size the workspace of ``critic_weight_grad`` for N rows ahead of time (a call that needs more grows it itself, which
        synchronises and cannot happen inside a graph capture)"""
        _lib.check(self.lib.hpe_critic_reserve(self._h, int(N)))

    def critic_params(self):
        """hpe_critic_get_params: the live critic weights as one flat CUDA tensor [critic_spec.PARAM_FLOATS] (a copy)"""
        out = self._new(PARAM_FLOATS)
        _lib.check(self.lib.hpe_critic_get_params(self._h, out.data_ptr(), self._stream()))
        return out

    def set_critic_params(self, flat):
        """hpe_critic_set_params_dev: replace the live critic weights by ``flat`` on the device, in stream order, without a host round
        trip (``load_critic`` comes first, once; ``critic_spec.flat_to_params`` turns a flat tensor back into its dict)"""
        _lib.check(self.lib.hpe_critic_set_params_dev(self._h, _flat_arg(flat, PARAM_FLOATS, "flat").data_ptr(), self._stream()))

    # ------------------------------------------------------------------ regressor training
    def regressor_params(self):
        """hpe_regressor_get_params: the live regressor (three Dense layers + mean theta) as one flat CUDA tensor
        [regressor_spec.PARAM_FLOATS] (a copy)"""
        out = self._new(REGRESSOR_PARAM_FLOATS)
        _lib.check(self.lib.hpe_regressor_get_params(self._h, out.data_ptr(), self._stream()))
        return out

    def set_regressor_params(self, flat):
        """hpe_regressor_set_params_dev: replace the live regressor and mean theta by ``flat`` on the device, in stream order, without
        a host round trip (``regressor_spec.flat_to_params`` turns a flat tensor back into its dict)"""
        _lib.check(self.lib.hpe_regressor_set_params_dev(self._h, _flat_arg(flat, REGRESSOR_PARAM_FLOATS, "flat").data_ptr(), self._stream()))

    def _drop(self, drop, B):
        if drop is None:
            return None
        drop = _require_cuda_tensor(drop.detach(), "drop")
        if tuple(drop.shape) != (2, B, 1024):
            raise ValueError("drop must be [2,%d,1024] (the multipliers of the two hidden layers at the last stage), got %s" % (B, tuple(drop.shape)))
        return drop

    def regressor_forward_train(self, features, drop=None):
        """hpe_regressor_forward_train: features [B,2048] -> thetas [num_stage,B,85], the IEF loop with the dropout multipliers
        ``drop`` [2,B,1024] (0 or 1 / keep) on the two hidden layers of the LAST stage; None: no dropout, the bits of ``tail``."""
        features = _require_cuda_tensor(features.detach(), "features", (2048,))
        B = features.shape[0]
        drop = self._drop(drop, B)
        out = self._new(self.num_stage, B, 85)
        _lib.check(self.lib.hpe_regressor_forward_train(self._h, features.data_ptr(), B, _ptr(drop), out.data_ptr(), self._stream()))
        return out

    def regressor_backward(self, features, grad_thetas, drop=None, want_grad_features=True):
        """hpe_regressor_backward: the gradient of sum(grad_thetas * thetas) (grad_thetas [num_stage,B,85]; None = zeros) with respect
        to the flat parameters -> (grad_flat [regressor_spec.PARAM_FLOATS], grad_features [B,2048] or None).  Stateless: the forward
        is recomputed, pass the same ``drop``.  Same inputs, same bits."""
        features = _require_cuda_tensor(features.detach(), "features", (2048,))
        B = features.shape[0]
        drop = self._drop(drop, B)
        if grad_thetas is not None:
            grad_thetas = _require_cuda_tensor(grad_thetas.detach(), "grad_thetas")
            if tuple(grad_thetas.shape) != (self.num_stage, B, 85):
                raise ValueError("grad_thetas must be [%d,%d,85], got %s" % (self.num_stage, B, tuple(grad_thetas.shape)))
        gflat = self._new(REGRESSOR_PARAM_FLOATS)
        gfeat = self._new(B, 2048) if want_grad_features else None
        _lib.check(self.lib.hpe_regressor_backward(self._h, features.data_ptr(), B, _ptr(drop), _ptr(grad_thetas), gflat.data_ptr(), _ptr(gfeat),
                                                   self._stream()))
        return gflat, gfeat

    # ------------------------------------------------------------------ encoder training (fp32 contexts; BatchNorm statistics frozen or of the batch)
    def reserve_encoder_train(self, B, batch_norm=False, precision="fp32"):
        """hpe_encoder_train_reserve: allocate the stash, cotangent buffers, partial sums and data-gradient packings for batches up to B.
        batch_norm=True (hpe_encoder_train_reserve_batchnorm): also the raw-output stash and the statistics buffers that ``bn="batch"``,
        ``encoder_stats``, ``update_encoder_stats`` and ``set_encoder_stats_dev`` need.  precision="bf16"
        (hpe_encoder_train_reserve_mixed): also the bf16 stash, cotangent buffers and weight operands of the mixed-precision walks.
        precision="mixed": the same with batch_norm=False; with batch_norm=True (hpe_encoder_train_reserve_batchnorm_mixed) both of
        those reserves and the bf16 raw-output stash of the mixed-precision walks with batch statistics."""
        fn, _ = self._entry("reserve", "batch" if batch_norm else "frozen", precision)
        _lib.check(fn(self._h, int(B)))

    @staticmethod
    def _entry_symbol(role, bn="frozen", precision="fp32"):
        """-> (name of the C entry point of ``role`` in this BatchNorm mode and precision (_lib.ENCODER_ENTRY), the precision's _Prec)"""
        batch = HpeEngine._bn_mode(bn)
        prec = _MIXED if HpeEngine._mixed(precision, bn) else _FP32
        return _lib.encoder_symbol(role, batch, prec.suffix), prec

    def _entry(self, role, bn="frozen", precision="fp32"):
        """``_entry_symbol`` with the library's function in place of its name"""
        name, prec = self._entry_symbol(role, bn, precision)
        return getattr(self.lib, name), prec

    @staticmethod
    def _bn_mode(bn):
        if bn not in ("frozen", "batch"):
            raise ValueError("bn must be 'frozen' or 'batch', got %r" % (bn,))
        return bn == "batch"

    @staticmethod
    def _mixed(precision, bn="frozen"):
        """True for precision="bf16" or "mixed": the mixed-precision walks (bf16 activations and cotangents on this fp32 context).
        "bf16" is the frozen-statistics spelling only; "mixed" runs with both BatchNorm modes (bn="frozen": the walks of "bf16", the
        same bits; bn="batch": BatchNorm arithmetic in fp32, its reductions in float64)"""
        if precision not in ("fp32", "bf16", "mixed"):
            raise ValueError("precision must be 'fp32', 'bf16' or 'mixed', got %r" % (precision,))
        batch = HpeEngine._bn_mode(bn)
        if precision == "bf16" and batch:
            raise ValueError("precision='bf16' runs with frozen BatchNorm statistics only: batch statistics in bf16 are the follow-up")
        return precision != "fp32"

    def encoder_stats(self):
        """hpe_encoder_get_stats: the installed moving statistics as one flat CUDA tensor [resnet_spec.ENCODER_STAT_FLOATS] (moving_mean of
        every layer, then moving_variance of every layer)"""
        out = self._new(ENCODER_STAT_FLOATS)
        _lib.check(self.lib.hpe_encoder_get_stats(self._h, out.data_ptr(), self._stream()))
        return out

    def update_encoder_stats(self, stats, momentum=0.99, unbiased=True):
        """hpe_encoder_update_stats: stats <- momentum * stats + (1 - momentum) * (the batch statistics of the last ``bn="batch"`` forward
        or backward), in place on the CUDA tensor ``stats``; unbiased multiplies each batch variance by M / (M - 1).  Returns ``stats``.
        It installs nothing: ``set_encoder_stats_dev`` does."""
        _lib.check(self.lib.hpe_encoder_update_stats(self._h, _flat_arg(stats, ENCODER_STAT_FLOATS, "stats").data_ptr(), float(momentum),
                                                     int(bool(unbiased)), self._stream()))
        return stats

    def set_encoder_stats_dev(self, stats):
        """hpe_encoder_set_stats_dev: install the CUDA tensor ``stats`` as the moving statistics, in stream order: the folded BatchNorm
        scale / shift and the dual-source weights are rewritten from them and the live parameters.  Capturable."""
        _lib.check(self.lib.hpe_encoder_set_stats_dev(self._h, _flat_arg(stats, ENCODER_STAT_FLOATS, "stats").data_ptr(), self._stream()))

    def encoder_batch_stats(self):
        """hpe_debug_encoder_batch_stats: mu | var of every layer of the last ``bn="batch"`` forward, in the statistics layout"""
        out = self._new(ENCODER_STAT_FLOATS)
        _lib.check(self.lib.hpe_debug_encoder_batch_stats(self._h, out.data_ptr(), self._stream()))
        return out

    def _stash(self, role, what, idx, bn, precision):
        """one stashed map of the last training forward of this precision, over that call's batch (idx -1: the max-pooled map)"""
        stash_batch, prec = self._entry("stash_batch", bn, precision)
        fn, _ = self._entry(role, bn, precision)
        B = stash_batch(self._h)
        if B < 1:
            raise _lib.HpeError("%s: no %s has run" % (what, prec.forward))
        s = CONV_SPECS[idx] if idx >= 0 else None
        out = prec.new(self, B, s.hout, s.hout, s.cout) if s else prec.new(self, B, 56, 56, 64)
        _lib.check(fn(self._h, idx, out.data_ptr(), self._stream()))
        return out

    def encoder_stash_raw(self, idx, precision="fp32"):
        """hpe_debug_encoder_stash_raw: layer idx's raw output conv(x, W) + b of the last ``bn="batch"`` forward, over that call's batch.
        precision="mixed" (hpe_debug_encoder_stash_raw_mixed): of the last mixed-precision one, as torch.bfloat16"""
        return self._stash("stash_raw", "encoder_stash_raw", idx, "batch", precision)

    def debug_conv_batchnorm(self, idx, x, residual=None, relu=True, precision="fp32"):
        """hpe_debug_conv_batchnorm: one layer with batch statistics -> (y, z, stats [2 * cout] = mu | var).  precision="mixed"
        (hpe_debug_conv_batchnorm_mixed): x, residual, y and z are torch.bfloat16 (x of idx 0: the float32 images), stats float32"""
        fn, prec = self._entry("conv_batchnorm", "batch", precision)
        s = CONV_SPECS[idx]
        x = prec.act(x, "x", idx)
        B = x.shape[0]
        y, z, st = prec.new(self, B, s.hout, s.hout, s.cout), prec.new(self, B, s.hout, s.hout, s.cout), self._new(2 * s.cout)
        residual = prec.act(residual, "residual", optional=True)
        _lib.check(fn(self._h, idx, x.data_ptr(), B, _ptr(residual), int(relu), y.data_ptr(), z.data_ptr(), st.data_ptr(), self._stream()))
        return y, z, st

    def _conv_backward(self, bn, precision, idx, x, z, y, dy, want_dx):
        """one layer's backward in either BatchNorm mode (z: the raw output, read with batch statistics only) and either precision"""
        fn, prec = self._entry("conv_backward", bn, precision)
        s = CONV_SPECS[idx]
        x = prec.act(x, "x", idx)
        z = prec.act(z, "z") if bn == "batch" else None
        dy = prec.act(dy, "dy")
        y = prec.act(y, "y", optional=True)  # None: a layer without activation (dz = dy)
        B = x.shape[0]
        dx = prec.new(self, B, s.hin, s.hin, s.cin) if want_dx and idx != 0 else None
        gl = self._new(s.kh * s.kw * s.cin * s.cout + 3 * s.cout)
        acts = [x.data_ptr()] + ([z.data_ptr()] if bn == "batch" else []) + [_ptr(y), dy.data_ptr()]
        _lib.check(fn(self._h, idx, *acts, B, _ptr(dx), gl.data_ptr(), self._stream()))
        return dx, gl

    def debug_conv_backward_batchnorm(self, idx, x, z, y, dy, want_dx=True, precision="fp32"):
        """hpe_debug_conv_backward_batchnorm: one layer's gate, BatchNorm backward, weight and data gradient from its raw output z and
        its activated output y (None: no activation) -> (dx or None, grad_layer = [kernel | bias = 0 | gamma | beta] flat).
        precision="mixed" (hpe_debug_conv_backward_batchnorm_mixed): x, z, y, dy and dx are torch.bfloat16 (x of idx 0: the float32
        images); grad_layer is float32"""
        return self._conv_backward("batch", precision, idx, x, z, y, dy, want_dx)

    # ------------------------------------------------------------------ data-parallel training: statistics over the batch of all ranks
    def set_encoder_reduce(self, callback, global_batch=0, owner=None):
        """hpe_encoder_set_reduce: from now on ``bn="batch"`` takes every layer's statistics over ``global_batch`` images: per layer the
        local column sums [2, cout] (float64, on the device) go through ``callback(user, dev_ptr, count, stream) -> 0 or nonzero``, which
        adds the other ranks' to them in place, ordered on the stream (``distributed.Reducer.callback``).  ``encoder_backward`` then
        returns this rank's PARTIAL gradient in every entry: the sum over the ranks is the gradient of the global batch.  None clears
        the hook.  owner: an object whose ``reraise()`` runs after every hooked library call, so that an exception the callback caught
        surfaces once the call has returned.  The callback object is kept alive here."""
        if callback is None:
            _lib.check(self.lib.hpe_encoder_set_reduce(self._h, _lib.REDUCE_FN(), None, 0))
            self._reduce_cb = self._reduce_owner = None
            return
        if not isinstance(callback, _lib.REDUCE_FN):
            callback = _lib.REDUCE_FN(callback)
        _lib.check(self.lib.hpe_encoder_set_reduce(self._h, callback, None, int(global_batch)))
        self._reduce_cb, self._reduce_owner = callback, owner

    def _check_hooked(self, rc):
        """the result of a library call that may have run the reduce hook: the callback's own exception first"""
        owner = getattr(self, "_reduce_owner", None)
        if owner is not None:
            owner.reraise()
        _lib.check(rc)

    def debug_bn_sums(self, idx, z):
        """hpe_debug_bn_sums: z [B,hout,hout,cout] -> the column sums [2, cout] float64 = (sum z | sum z^2), in the library's order"""
        torch = _torch()
        z = _require_cuda_tensor(z, "z")
        out = torch.empty((2, CONV_SPECS[idx].cout), dtype=torch.float64, device=self.tdev)
        _lib.check(self.lib.hpe_debug_bn_sums(self._h, idx, z.data_ptr(), z.shape[0], out.data_ptr(), self._stream()))
        return out

    @staticmethod
    def _sums_arg(sums, idx, name):
        torch = _torch()
        if not (isinstance(sums, torch.Tensor) and sums.is_cuda and sums.dtype == torch.float64 and sums.is_contiguous()
                and tuple(sums.shape) == (2, CONV_SPECS[idx].cout)):
            raise ValueError("%s must be a contiguous CUDA float64 tensor [2, %d]" % (name, CONV_SPECS[idx].cout))
        return sums

    def debug_bn_finish(self, idx, sums, M, z, residual=None, relu=True):
        """hpe_debug_bn_finish: the statistics of ``sums`` over M rows applied to the images of z -> (y, stats [2 * cout] = mu | var)"""
        s = CONV_SPECS[idx]
        z, sums = _require_cuda_tensor(z, "z"), self._sums_arg(sums, idx, "sums")
        y, st = self._new(*z.shape), self._new(2 * s.cout)
        residual = _FP32.act(residual, "residual", optional=True)
        _lib.check(self.lib.hpe_debug_bn_finish(self._h, idx, sums.data_ptr(), int(M), z.data_ptr(), z.shape[0], _ptr(residual), int(relu),
                                                y.data_ptr(), st.data_ptr(), self._stream()))
        return y, st

    def debug_bn_backward_sums(self, idx, z, y, dy, sums, M):
        """hpe_debug_bn_backward_sums: -> [2, cout] float64 = (sum dz | sum dz * xhat) over the rows given, xhat from (sums, M)"""
        torch = _torch()
        z, dy, sums = _require_cuda_tensor(z, "z"), _require_cuda_tensor(dy, "dy"), self._sums_arg(sums, idx, "sums")
        y = _FP32.act(y, "y", optional=True)
        out = torch.empty((2, CONV_SPECS[idx].cout), dtype=torch.float64, device=self.tdev)
        _lib.check(self.lib.hpe_debug_bn_backward_sums(self._h, idx, z.data_ptr(), _ptr(y), dy.data_ptr(), z.shape[0], sums.data_ptr(), int(M),
                                                       out.data_ptr(), self._stream()))
        return out

    def debug_bn_backward_finish(self, idx, x, z, y, dy, sums, bwd_sums, M, want_dx=True):
        """hpe_debug_bn_backward_finish: the layer's backward on the rows given with the statistics of (sums, M) and the reduced
        ``bwd_sums`` -> (dx or None, grad_layer = [kernel | bias = 0 | gamma | beta], each the partial of these rows)"""
        s = CONV_SPECS[idx]
        x, z, dy = _require_cuda_tensor(x, "x"), _require_cuda_tensor(z, "z"), _require_cuda_tensor(dy, "dy")
        y = _FP32.act(y, "y", optional=True)
        sums, bwd_sums = self._sums_arg(sums, idx, "sums"), self._sums_arg(bwd_sums, idx, "bwd_sums")
        B = x.shape[0]
        dx = self._new(B, s.hin, s.hin, s.cin) if want_dx and idx != 0 else None
        gl = self._new(s.kh * s.kw * s.cin * s.cout + 3 * s.cout)
        _lib.check(self.lib.hpe_debug_bn_backward_finish(self._h, idx, x.data_ptr(), z.data_ptr(), _ptr(y), dy.data_ptr(), B, sums.data_ptr(),
                                                         bwd_sums.data_ptr(), int(M), _ptr(dx), gl.data_ptr(), self._stream()))
        return dx, gl

    def encoder_params(self):
        """hpe_encoder_get_params: the live kernels, biases, gammas and betas as one flat CUDA tensor [resnet_spec.ENCODER_PARAM_FLOATS]"""
        out = self._new(ENCODER_PARAM_FLOATS)
        _lib.check(self.lib.hpe_encoder_get_params(self._h, out.data_ptr(), self._stream()))
        return out

    def set_encoder_params(self, flat):
        """hpe_encoder_set_params: replace the encoder's trainable parameters by ``flat`` (a tensor on any device or an array).  The host
        packing runs again and is copied into the existing device buffers; synchronous, not capturable."""
        torch = _torch()
        if isinstance(flat, torch.Tensor):
            flat = flat.detach().to("cpu", torch.float32).numpy()
        arr, ptr = _lib.f32(np.asarray(flat).reshape(-1))
        if arr.shape != (ENCODER_PARAM_FLOATS,):
            raise ValueError("flat must be [%d], got %s" % (ENCODER_PARAM_FLOATS, arr.shape))
        _lib.check(self.lib.hpe_encoder_set_params(self._h, ptr))

    def set_encoder_params_dev(self, flat):
        """hpe_encoder_set_params_dev: replace the encoder's trainable parameters by the CUDA tensor ``flat`` on the device, in stream
        order: every packing the context holds is rewritten by gather kernels, bit for bit what a fresh context would hold.  No host
        round trip, no synchronisation, capturable."""
        _lib.check(self.lib.hpe_encoder_set_params_dev(self._h, _flat_arg(flat, ENCODER_PARAM_FLOATS, "flat").data_ptr(), self._stream()))

    def encoder_packing(self, idx, which):
        """hpe_debug_encoder_packing: the bytes of one packing of layer idx (``which``: a name of _lib.ENCODER_PACKINGS or its index)
        as a CUDA uint8 tensor; None if this context does not hold that form of that layer"""
        torch = _torch()
        if isinstance(which, str):
            which = _lib.ENCODER_PACKINGS.index(which)
        n = self.lib.hpe_debug_encoder_packing_bytes(self._h, int(idx), int(which))
        if n == 0:
            return None
        out = torch.empty(n, dtype=torch.uint8, device=self.tdev)
        _lib.check(self.lib.hpe_debug_encoder_packing(self._h, int(idx), int(which), out.data_ptr(), self._stream()))
        return out

    def encoder_forward_train(self, images, bn="frozen", precision="fp32"):
        """hpe_encoder_forward_train: images [B,224,224,3] -> features [B,2048], layer by layer, every activation kept in the stash.
        bn="batch" (hpe_encoder_forward_batchnorm): every BatchNorm normalises with the statistics of this batch.  precision="bf16"
        (hpe_encoder_forward_train_mixed): bf16 activations and matrix products, fp32 accumulation; images and features stay fp32.
        precision="mixed": the same with bn="frozen"; with bn="batch" (hpe_encoder_forward_batchnorm_mixed) the statistics of this
        batch, taken of the bf16 raw outputs in float64."""
        fn, _ = self._entry("forward", bn, precision)
        images = _require_cuda_tensor(images.detach(), "images", (224, 224, 3))
        B = images.shape[0]
        out = self._new(B, 2048)
        self._check_hooked(fn(self._h, images.data_ptr(), B, out.data_ptr(), self._stream()))
        return out

    def encoder_backward(self, images, grad_features, bn="frozen", precision="fp32"):
        """hpe_encoder_backward: the gradient of sum(grad_features * features) with respect to the flat encoder parameters.  Stateless
        (the training forward runs again); same inputs, same bits.  bn="batch" (hpe_encoder_backward_batchnorm): through the batch
        statistics; the bias slots are 0.  precision="bf16" (hpe_encoder_backward_mixed): the mixed-precision walk; the flat gradient
        is fp32.  precision="mixed": that walk with bn="frozen", hpe_encoder_backward_batchnorm_mixed with bn="batch"."""
        fn, _ = self._entry("backward", bn, precision)
        images = _require_cuda_tensor(images.detach(), "images", (224, 224, 3))
        B = images.shape[0]
        grad_features = _require_cuda_tensor(grad_features.detach(), "grad_features")
        if tuple(grad_features.shape) != (B, 2048):
            raise ValueError("grad_features must be [%d,2048], got %s" % (B, tuple(grad_features.shape)))
        g = self._new(ENCODER_PARAM_FLOATS)
        self._check_hooked(fn(self._h, images.data_ptr(), B, grad_features.data_ptr(), g.data_ptr(), self._stream()))
        return g

    def debug_conv_backward(self, idx, x, y, dy, want_dx=True, precision="fp32"):
        """hpe_debug_conv_backward: one layer's gate, weight gradient and data gradient -> (dx or None, grad_layer = [kernel | bias |
        gamma | beta] flat).  precision="bf16" (hpe_debug_conv_backward_mixed): x, y, dy and dx are torch.bfloat16 (x of idx 0: the
        float32 images); grad_layer is float32"""
        return self._conv_backward("frozen", precision, idx, x, None, y, dy, want_dx)

    def debug_maxpool_backward(self, x, dy, precision="fp32"):
        fn, prec = self._entry("maxpool_backward", "frozen", precision)
        x, dy = prec.act(x, "x"), prec.act(dy, "dy")
        dx = prec.new(self, *x.shape)
        _lib.check(fn(x.data_ptr(), dy.data_ptr(), x.shape[0], x.shape[1], x.shape[3], dx.data_ptr(), self._stream()))
        return dx

    def debug_avgpool_backward(self, dy, HW, precision="fp32"):
        dy = _require_cuda_tensor(dy, "dy")  # the cotangent of the features: float32 in both precisions
        fn, prec = self._entry("avgpool_backward", "frozen", precision)
        dx = prec.new(self, dy.shape[0], HW, dy.shape[1])
        _lib.check(fn(dy.data_ptr(), dy.shape[0], HW, dy.shape[1], dx.data_ptr(), self._stream()))
        return dx

    def encoder_stash(self, idx, precision="fp32"):
        """hpe_debug_encoder_stash: layer idx's output of the last training forward, over that call's batch (idx -1: the max-pooled map).
        precision="bf16" (hpe_debug_encoder_stash_mixed): of the last mixed-precision forward, as torch.bfloat16"""
        return self._stash("stash", "encoder_stash", idx, "frozen", precision)

    def mesh_loss(self, seg, verts2d):
        torch = _torch()
        seg = _require_cuda_tensor(seg, "seg")
        verts2d = _require_cuda_tensor(verts2d, "verts2d")
        B, H, W = seg.shape[0], seg.shape[1], seg.shape[2]
        P = verts2d.shape[1]
        out = torch.zeros(4, dtype=torch.float32, device=self.tdev)
        _lib.check(self.lib.hpe_mesh_loss(self._h, seg.data_ptr(), verts2d.data_ptr(), B, H, W, P, out.data_ptr(), self._stream()))
        return out[0]

    def mesh_loss_grad(self, seg, verts2d, want_neighbours=False):
        """hpe_mesh_loss_grad: seg [B,H,W] (> 0 = silhouette), verts2d [B,P,2] -> (loss, grad [B,P,2] = d loss / d verts2d) from one
        pair of nearest-neighbour searches; want_neighbours=True appends (nn_pix [B,H,W] int32: nearest vertex of every silhouette
        pixel, -1 elsewhere; nn_vert [B,P] int32: y * W + x of every vertex' nearest silhouette pixel, -1 if there is none)."""
        torch = _torch()
        seg = _require_cuda_tensor(seg, "seg")
        verts2d = _require_cuda_tensor(verts2d, "verts2d")
        if seg.dim() != 3 or verts2d.dim() != 3 or verts2d.shape[2] != 2 or verts2d.shape[0] != seg.shape[0]:
            raise ValueError("seg must be [B,H,W] and verts2d [B,P,2], got %s and %s" % (tuple(seg.shape), tuple(verts2d.shape)))
        B, H, W = seg.shape[0], seg.shape[1], seg.shape[2]
        P = verts2d.shape[1]
        out = torch.zeros(4, dtype=torch.float32, device=self.tdev)
        grad = torch.empty((B, P, 2), dtype=torch.float32, device=self.tdev)
        nn_pix = nn_vert = None
        if want_neighbours:
            nn_pix = torch.empty((B, H, W), dtype=torch.int32, device=self.tdev)
            nn_vert = torch.empty((B, P), dtype=torch.int32, device=self.tdev)
        _lib.check(self.lib.hpe_mesh_loss_grad(self._h, seg.data_ptr(), verts2d.data_ptr(), B, H, W, P, out.data_ptr(), grad.data_ptr(),
                                               _ptr(nn_pix), _ptr(nn_vert), self._stream()))
        return (out[0], grad, nn_pix, nn_vert) if want_neighbours else (out[0], grad)

    def val_losses(self, kp_gt, kp2d_stages, seg=None, verts2d_stages=None, out=None):
        """Both reprojection losses of every IEF stage in one call (hpe_val_losses): -> tensor [n_stage, 4] =
        (kp numerator, kp count, kp loss, mesh loss sum) per stage.  The silhouette-only work is done once per call."""
        torch = _torch()
        kp_gt = _require_cuda_tensor(kp_gt, "kp_gt")
        n = len(kp2d_stages)
        kp2d = [_require_cuda_tensor(t, "kp2d") for t in kp2d_stages]
        B, K = kp_gt.shape[0], kp_gt.shape[1]
        kp_ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in kp2d])
        H = W = P = 0
        seg_ptr, v_ptrs, keep = None, None, None
        if seg is not None and verts2d_stages is not None:
            seg = _require_cuda_tensor(seg, "seg")
            keep = [_require_cuda_tensor(t, "verts2d") for t in verts2d_stages]
            if len(keep) != n or seg.shape[0] != B:
                raise ValueError("one verts2d tensor per stage and one silhouette per image are needed")
            H, W, P = seg.shape[1], seg.shape[2], keep[0].shape[1]
            seg_ptr = seg.data_ptr()
            v_ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in keep])
        if out is None:
            out = torch.empty((n, 4), dtype=torch.float32, device=self.tdev)
        _lib.check(self.lib.hpe_val_losses(self._h, seg_ptr, kp_gt.data_ptr(), kp_ptrs, v_ptrs, n, B, K, H, W, P, out.data_ptr(), self._stream()))
        return out

    def check_device(self):
        """Synchronise the current stream and raise if a kernel flagged an invalid result (hpe_device_status)."""
        _lib.check(self.lib.hpe_device_status(self._h, self._stream()))

    def debug_conv(self, idx, x, residual=None, relu=True):
        s = CONV_SPECS[idx]
        x = _require_cuda_tensor(x, "x")
        B = x.shape[0]
        y = self._new(B, s.hout, s.hout, s.cout)
        residual = _FP32.act(residual, "residual", optional=True)
        _lib.check(self.lib.hpe_debug_conv(self._h, idx, x.data_ptr(), B, _ptr(residual), int(relu), y.data_ptr(), self._stream()))
        return y

    def conv_route(self, idx, B, concurrent=False, residual=False, workspace=True):
        """hpe_debug_conv_route with this engine's own config: which kernel layer idx takes at batch B (_lib.HpeConvRoute)"""
        return _lib.conv_route(self.lib, self._cfg, idx, B, concurrent, residual, workspace)

    def debug_dual(self, idx2c, t2, x):
        """hpe_debug_dual: the dual-source launch of the conv_block whose branch2c is idx2c, t2 [B,ho,ho,cin2c] and the block input x"""
        s = CONV_SPECS[idx2c]
        t2 = _require_cuda_tensor(t2, "t2")
        x = _require_cuda_tensor(x, "x")
        B = t2.shape[0]
        y = self._new(B, s.hout, s.hout, s.cout)
        _lib.check(self.lib.hpe_debug_dual(self._h, int(idx2c), t2.data_ptr(), x.data_ptr(), B, y.data_ptr(), self._stream()))
        return y

    def conv_stream1x1(self, idx, B, concurrent=False, residual=True):
        """hpe_debug_conv_stream1x1 with this engine's own config and the environment as it is now: bit 0 = the launch runs on
        conv_stream_f32s.hip, bit 1 = the layer is one of that kernel's"""
        return int(self.lib.hpe_debug_conv_stream1x1(C.byref(self._cfg), int(idx), int(B), int(concurrent), int(residual)))

    def _debug_gemm(self, call, what, mode, tile, x, wt, y, M, N, K, kw):
        g = _lib.HpeDebugGemm()
        g.struct_size = C.sizeof(_lib.HpeDebugGemm)
        fields = dict(lda=K, ldw=K, ldy=N, ldres=N, mode=mode, tile=tile, x=x, wt=wt, y=y, M=M, N=N, K=K)
        fields.update(kw)
        for k, v in fields.items():
            if k in ("x", "x2", "wt", "residual", "scale", "shift", "y"):
                v = v.data_ptr() if hasattr(v, "data_ptr") else v
            elif k in ("struct_size", "split_k") or not hasattr(g, k):
                raise TypeError("%s: unknown argument %r" % (what, k))
            setattr(g, k, v)
        sk = C.c_int(-1)
        g.split_k = C.pointer(sk)
        _lib.check(call(g))
        return sk.value

    def debug_gemm_ex(self, mode, tile, x, wt, y, M, N, K, **kw):
        """hpe_debug_gemm_ex: the fp32 implicit-GEMM kernel with every launch argument given (HpeDebugGemm of include/hpe.h).  x, wt, y
        and the optional x2 / residual / scale / shift are CUDA tensors or device addresses, y is written in place; the other
        HpeDebugGemm fields are keywords (default 0, pitches default to the dense ones).  Returns the split_k the launcher chose."""
        return self._debug_gemm(lambda g: self.lib.hpe_debug_gemm_ex(self._h, C.byref(g), self._stream()), "debug_gemm_ex", mode, tile, x, wt, y, M, N, K, kw)

    def debug_gemm_launch(self, kernel, mode, tile, x, wt, y, M, N, K, w_piece=0, **kw):
        """hpe_debug_gemm_launch: debug_gemm_ex for any of the four implicit-GEMM kernels -- 0 fp32, 1 f32s (wt: three bf16 pieces per
        row, w_piece elements apart), 2 bf16, 3 bf16 256x256 (x, x2, wt, residual, y in bf16; pitches in bf16 elements).  Returns the
        split_k the launcher chose."""
        return self._debug_gemm(lambda g: self.lib.hpe_debug_gemm_launch(self._h, C.byref(g), int(kernel), int(w_piece), self._stream()),
                                "debug_gemm_launch", mode, tile, x, wt, y, M, N, K, kw)

    def debug_chain(self, idx2c, t2, residual):
        """bf16 contexts: res*_branch2c (+ residual + ReLU) and the next block's res*_branch2a (+ ReLU) as the one launch of
        conv_chain_bf16.hip.  Returns (t3 [B,H,H,4C], u1 [B,H,H,C], resident workgroups per CU of the two instantiations)."""
        s = CONV_SPECS[idx2c]
        first = CONV_SPECS[idx2c + 1].name.endswith("branch1")  # conv_block form: `residual` is the block input
        sn = CONV_SPECS[idx2c + (2 if first else 1)]
        t2 = _require_cuda_tensor(t2, "t2", (s.hin, s.hin, s.cin))
        residual = _require_cuda_tensor(residual, "residual", (s.hout, s.hout, CONV_SPECS[idx2c + 1].cin if first else s.cout))
        B = t2.shape[0]
        t3 = self._new(B, s.hout, s.hout, s.cout)
        u1 = self._new(B, sn.hout, sn.hout, sn.cout)
        occ = (C.c_int * 3)()
        _lib.check(self.lib.hpe_debug_chain(self._h, idx2c, t2.data_ptr(), residual.data_ptr(), B, t3.data_ptr(), u1.data_ptr(), occ, self._stream()))
        return t3, u1, (occ[0], occ[1], occ[2])

    def debug_stream_chain(self, idx2c, t2, x, slab8=False, rows=0):
        """hpe_debug_stream_chain: the chained launch of conv_stream_chain_f32s.hip alone (fp32 contexts).  idx2c = res2b_branch2c with x the
        residual [B,56,56,256], or res2a_branch2c with x the block input [B,56,56,64].  Returns (t3 [B,56,56,256], u1): u1 [B,56,56,64]
        row-major, or the flat channel-slab major buffer [8, M, 8] when slab8.  rows: ask the launcher for the first `rows` rows only (zero
        filled outputs beyond them); a count it refuses raises and launches nothing."""
        s = CONV_SPECS[idx2c]
        first = CONV_SPECS[idx2c + 1].name.endswith("branch1")
        sn = CONV_SPECS[idx2c + (2 if first else 1)]
        t2 = _require_cuda_tensor(t2, "t2", (s.hin, s.hin, s.cin))
        x = _require_cuda_tensor(x, "x", (s.hout, s.hout, CONV_SPECS[idx2c + 1].cin if first else s.cout))
        B = t2.shape[0]
        t3 = self._new(B, s.hout, s.hout, s.cout)
        M = int(rows) if rows else B * sn.hout * sn.hout
        u1 = self._new(sn.cout // 8, M, 8) if slab8 else self._new(B, sn.hout, sn.hout, sn.cout)
        if rows:
            t3.zero_()
            u1.zero_()
        _lib.check(self.lib.hpe_debug_stream_chain(self._h, int(idx2c), t2.data_ptr(), x.data_ptr(), B, t3.data_ptr(), u1.data_ptr(), int(bool(slab8)),
                                                   int(rows), self._stream()))
        return t3, u1

    def debug_stem(self, images, rows_per_strip=0):
        images = _require_cuda_tensor(images, "images", (224, 224, 3))
        y = self._new(images.shape[0], 56, 56, 64)
        _lib.check(self.lib.hpe_debug_stem(self._h, images.data_ptr(), images.shape[0], int(rows_per_strip), y.data_ptr(), self._stream()))
        return y

    def joint_regress(self, X, use_kp_regressor=True):
        X = _require_cuda_tensor(X, "X", (NUM_VERTS, 3))
        K = self.num_kp if use_kp_regressor else 24
        out = self._new(X.shape[0], K, 3)
        _lib.check(self.lib.hpe_debug_joint_regress(self._h, X.data_ptr(), X.shape[0], int(use_kp_regressor), out.data_ptr(), self._stream()))
        return out

    def encoder_kernel_description(self):
        """The kernel family bench.py's `roofline` block prices (one string per encoder dtype, kept next to the dispatch)."""
        if self.encoder_dtype == "fp32":
            return ("conv_gemm_f32s_dma_kernel (the 1x1 / strided / dual-source layers of stages 3-5 on the bf16 matrix cores, operands split "
                    "exactly into three bf16 pieces) + conv_gemm_f32_dma_kernel (the other 1x1 layers) + w4_input_kernel + w4_gemm_kernel / w4_gemm32_kernel "
                    "(the 13 3x3 layers on the 28x28 / 14x14 / 7x7 maps as fp32 Winograd F(4x4,3x3); F(2x2,3x3) / direct below 64 work "
                    "items) + wino_fused_split_kernel (the three 56x56 3x3 layers, F(2x2,3x3) on the bf16 matrix cores through the same exact split) + stem_fused_f32s_kernel (image and weights split like the 1x1 layers) -- the 53 conv layers of one "
                    "step, priced at their direct-convolution FLOPs")
        return ("conv_gemm_bf16_dma_kernel (1x1 / strided / dual-source layers) + chain_expand_reduce_bf16_kernel (branch2c + next branch2a of "
                "stages 2-3 as one launch) + conv3_halo_bf16_kernel (the sixteen 3x3 layers, tile + halo resident in LDS) + stem_fused_bf16_kernel "
                "-- the 53 conv layers of one step, priced at their algorithmic HBM bytes")

    def enable_timing(self, level=1):
        _lib.check(self.lib.hpe_enable_timing(self._h, int(level)))

    def timings(self):
        ms = (C.c_float * 5)()
        _lib.check(self.lib.hpe_get_timings(self._h, ms))
        return dict(encoder_ms=ms[0], conv_ms=ms[1], regress_smpl_ms=ms[2], total_ms=ms[4])

    def span_stats(self):
        """Encoder span over all timed calls since enable_timing (hpe_get_span_stats): dict(mean_ms, min_ms, max_ms, calls)."""
        ms = (C.c_float * 3)()
        n = C.c_int()
        _lib.check(self.lib.hpe_get_span_stats(self._h, ms, C.byref(n)))
        return dict(mean_ms=ms[0], min_ms=ms[1], max_ms=ms[2], calls=n.value)

    def set_loss_counter(self, counter=None):
        """counter: int64 CUDA tensor of 2 elements (zeroed by the caller) that the pixel -> vertex searches add their MFMA counts
        to ([0] cell-grid search, [1] full search; 1024 (pixel, vertex) pairs per MFMA); None disables."""
        _lib.check(self.lib.hpe_debug_set_loss_counter(self._h, None if counter is None else counter.data_ptr()))
        self._loss_counter = counter  # keep alive

    def loss_timings(self):
        ms = (C.c_float * 2)()
        _lib.check(self.lib.hpe_get_loss_timings(self._h, ms))
        return dict(val_losses_ms=ms[0], a2b_search_ms=ms[1])

    def conv_timings(self):
        ms = (C.c_float * _lib.NUM_CONV)()
        _lib.check(self.lib.hpe_get_conv_timings(self._h, ms))
        return list(ms)


# ---------------------------------------------------------------------- context-free operators
def _cur_stream(t):
    return C.c_void_p(_torch().cuda.current_stream(t.device).cuda_stream)


def orth_proj(X, camera):
    X = _require_cuda_tensor(X, "X")
    camera = _require_cuda_tensor(camera, "camera").reshape(-1, 3)
    B, P = X.shape[0], X.shape[1]
    out = _torch().empty((B, P, 2), dtype=_torch().float32, device=X.device)
    with _torch().cuda.device(X.device):
        _lib.check(_lib.load().hpe_orth_proj(X.data_ptr(), camera.data_ptr(), B, P, out.data_ptr(), _cur_stream(X)))
    return out


def reproject(verts, cam, im_w, im_h):
    verts = _require_cuda_tensor(verts, "verts")
    cam = _require_cuda_tensor(cam, "cam").reshape(-1, 3)
    B, P = verts.shape[0], verts.shape[1]
    out = _torch().empty((B, P, 2), dtype=_torch().float32, device=verts.device)
    with _torch().cuda.device(verts.device):
        _lib.check(
            _lib.load().hpe_reproject_vertices(verts.data_ptr(), cam.data_ptr(), B, P, float(im_w), float(im_h), out.data_ptr(), _cur_stream(verts))
        )
    return out


def kp_loss_backward(kp_gt, kp_pred, grad_loss=None):
    """d kp_reprojection_loss / d kp_pred (hpe_kp_loss_backward): grad_loss = one-element CUDA float tensor or None (= 1)"""
    kp_gt = _require_cuda_tensor(kp_gt, "kp_gt")
    kp_pred = _require_cuda_tensor(kp_pred, "kp_pred")
    B, K = kp_gt.shape[0], kp_gt.shape[1]
    if grad_loss is not None:
        grad_loss = _require_cuda_tensor(grad_loss.reshape(1), "grad_loss")
    out = _torch().empty((B, K, 2), dtype=_torch().float32, device=kp_gt.device)
    with _torch().cuda.device(kp_gt.device):
        _lib.check(_lib.load().hpe_kp_loss_backward(kp_gt.data_ptr(), kp_pred.data_ptr(), B, K, _ptr(grad_loss), out.data_ptr(), _cur_stream(kp_gt)))
    return out


def kp_loss_parts(kp_gt, kp_pred):
    """-> tensor [3]: (sum vis*|d|, 2*#visible, loss)"""
    kp_gt = _require_cuda_tensor(kp_gt, "kp_gt")
    kp_pred = _require_cuda_tensor(kp_pred, "kp_pred")
    B, K = kp_gt.shape[0], kp_gt.shape[1]
    out = _torch().zeros(4, dtype=_torch().float32, device=kp_gt.device)
    with _torch().cuda.device(kp_gt.device):
        _lib.check(_lib.load().hpe_kp_loss(kp_gt.data_ptr(), kp_pred.data_ptr(), B, K, out.data_ptr(), _cur_stream(kp_gt)))
    return out[:3]


def _loss3d_call(symbol, joints, betas, Rs, gt, tail):
    """The one body of the two 3-D loss calls (hpe_loss3d, hpe_loss3d_backward): the predictions, per-stage lists of joints [B,K,3],
    betas [B,10] (a ``theta[:, 75:]`` view is read in place) and Rs [B,24,3,3] (a single tensor each: one stage), and the ground
    truth ``gt`` (``ops.Gt3D``) checked once; ``tail(n, B, K, dev)`` -> (what to return, the call's trailing arguments)."""
    torch = _torch()
    as_list = lambda x: [x] if isinstance(x, torch.Tensor) else list(x)  # noqa: E731
    joints, betas, Rs = as_list(joints), as_list(betas), as_list(Rs)
    n = len(joints)
    if not 1 <= n <= 16 or len(betas) != n or len(Rs) != n:
        raise ValueError("joints, betas and Rs must be one tensor each or lists of the same length in [1, 16]")
    gj = _require_cuda_tensor(gt.joints, "gt.joints", (14, 3))
    gR = _require_cuda_tensor(gt.Rs, "gt.Rs", (24, 3, 3))
    gs = _require_cuda_tensor(gt.shape, "gt.shape", (10,))
    wj, ws = _require_cuda_tensor(gt.w_joints, "gt.w_joints"), _require_cuda_tensor(gt.w_smpl, "gt.w_smpl")
    B, dev = gj.shape[0], gj.device
    flip = gt.flip
    if flip is not None:
        if not isinstance(flip, torch.Tensor) or not flip.is_cuda or flip.dtype not in (torch.uint8, torch.bool) or tuple(flip.shape) != (B,):
            raise ValueError("gt.flip must be a uint8 or bool CUDA tensor [%d], or None" % B)
        flip = flip.to(torch.uint8).contiguous()
    if B < 1 or gR.shape[0] != B or gs.shape[0] != B or tuple(wj.shape) != (B,) or tuple(ws.shape) != (B,):
        raise ValueError("gt must hold joints [B,14,3], Rs [B,24,3,3], shape [B,10], w_joints [B] and w_smpl [B] with one B >= 1")
    joints = [_require_cuda_tensor(t.detach(), "joints") for t in joints]
    Rs = [_require_cuda_tensor(t.detach(), "Rs", (24, 3, 3)) for t in Rs]
    K = joints[0].shape[1] if joints[0].dim() == 3 else 0
    if any(t.dim() != 3 or tuple(t.shape) != (B, K, 3) for t in joints) or not 14 <= K <= 24:
        raise ValueError("every stage's joints must be [%d,K,3] with one 14 <= K <= 24" % B)
    if any(t.shape[0] != B for t in Rs):
        raise ValueError("every stage's Rs must be [%d,24,3,3]" % B)
    bs = [b.detach() for b in betas]
    if any(not b.is_cuda or b.dtype != torch.float32 or tuple(b.shape) != (B, 10) for b in bs):
        raise ValueError("every stage's betas must be a float32 CUDA tensor [%d,10]" % B)
    strides = {b.stride(0) for b in bs} if B > 1 else {10}
    if any(b.stride(1) != 1 for b in bs) or len(strides) != 1 or min(strides) < 10:  # the call has one row stride for all stages
        bs, strides = [b.contiguous() for b in bs], {10}
    stride = strides.pop()
    if any(t.device != dev for t in joints + Rs + bs + [gR, gs, wj, ws] + ([flip] if flip is not None else [])):
        raise ValueError("the predictions and gt must live on one device")
    ptrs = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])  # noqa: E731
    with torch.cuda.device(dev):
        result, args = tail(n, B, K, dev)
        _lib.check(getattr(_lib.load(), symbol)(ptrs(joints), ptrs(Rs), ptrs(bs), stride, gj.data_ptr(), gR.data_ptr(), gs.data_ptr(), wj.data_ptr(),
                                                ws.data_ptr(), _ptr(flip), n, B, K, *args, _cur_stream(gj)))
    return result


def loss3d_parts(joints, betas, Rs, gt, want_per_image=False):
    """hpe_loss3d for all the stages given in ONE launch -> parts [n_stage,5] = (num_j, num_pose, num_shape, cnt_j, cnt_s), the
    numerators and counts of the joint and the SMPL-parameter loss (DESIGN.md "3-D supervision"); want_per_image=True returns (parts,
    per_image [n_stage,B,3], each row's unweighted sums of squares: joints, rotations, shape; 0 where the term's weight is 0)."""

    def tail(n, B, K, dev):
        parts = _torch().empty((n, 5), dtype=_torch().float32, device=dev)
        per = _torch().empty((n, B, 3), dtype=_torch().float32, device=dev) if want_per_image else None
        return ((parts, per) if want_per_image else parts), (parts.data_ptr(), _ptr(per))

    return _loss3d_call("hpe_loss3d", joints, betas, Rs, gt, tail)


def loss3d_backward(joints, betas, Rs, gt, scale_j=None, scale_s=None, want=("joints", "betas", "Rs")):
    """hpe_loss3d_backward: the gradient of the two losses with respect to the predictions named in ``want`` (among joints, betas, Rs)
    -> dict of per-stage lists (of tensors, where the predictions were single tensors).  scale_j / scale_s: CUDA float tensors of one
    element per stage, grad_loss * 0.5 / count with the local or the global count; scale_j is needed for 'joints', scale_s for the
    other two.  Nothing reads the device."""
    torch = _torch()
    names = ("joints", "Rs", "betas")  # the ABI's order
    if not want or any(k not in names for k in want):
        raise ValueError("want must name some of %s, got %r" % (sorted(names), tuple(want)))
    single = isinstance(joints, torch.Tensor)

    def tail(n, B, K, dev):
        def scale(t, name, needed):
            if not needed:
                return None
            if t is None:
                raise ValueError("%s is needed for %s" % (name, "'joints'" if name == "scale_j" else "'betas' and 'Rs'"))
            t = _require_cuda_tensor(t.detach().reshape(-1), name)
            if t.numel() != n or t.device != dev:
                raise ValueError("%s must hold one float per stage (%d) on %s" % (name, n, dev))
            return t

        sj, ss = scale(scale_j, "scale_j", "joints" in want), scale(scale_s, "scale_s", "betas" in want or "Rs" in want)
        shapes = {"joints": (B, K, 3), "Rs": (B, 24, 3, 3), "betas": (B, 10)}
        out = {k: [torch.empty(shapes[k], dtype=torch.float32, device=dev) for _ in range(n)] for k in want}
        arrs = [(C.c_void_p * n)(*[t.data_ptr() for t in out[k]]) if k in out else None for k in names]
        return ({k: v[0] if single else v for k, v in out.items()}), (_ptr(sj), _ptr(ss), *arrs)

    return _loss3d_call("hpe_loss3d_backward", joints, betas, Rs, gt, tail)
