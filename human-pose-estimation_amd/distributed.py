"""Batch-sharded multi-GPU driver: one process per GPU, ``torch.distributed`` (backend "nccl" == RCCL over
xGMI on ROCm; "gloo" for the CPU rehearsal tests).

The path shards naturally: images are independent units, weights and SMPL constants are
replicated, and the ONLY data-path collective is one all-gather of the predicted theta rows
([B_local, 85] fp32 = 87 KB per rank at B_local = 256 -- latency-bound, one call, no bucketing).
For the config-5 losses ``kp_reprojection_loss`` normalises by the GLOBAL visible count, so ranks all-reduce
(numerator, count) and divide afterwards; the mesh loss is a plain sum over images.
"""
from __future__ import annotations

import os


def _dist():
    import torch.distributed as dist

    return dist


def init_from_env(backend=None, timeout=None):
    """Initialise the default process group from RANK / WORLD_SIZE / LOCAL_RANK / MASTER_* (torchrun contract).
    Returns (rank, world, local_rank).  world == 1 needs no process group.  timeout: a
    datetime.timedelta for the group's collectives (None: torch's default)."""
    import torch

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1 and not _dist().is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend is None:
            backend = "nccl" if torch.cuda.is_available() else "gloo"
        kw = {} if timeout is None else {"timeout": timeout}
        if backend == "nccl":
            torch.cuda.set_device(local_rank)
            kw["device_id"] = torch.device("cuda", local_rank)
        _dist().init_process_group(backend, rank=rank, world_size=world, **kw)
    return rank, world, local_rank


def shard_bounds(n, rank, world):
    """Contiguous shard [lo, hi) of n items for `rank`; the first n % world ranks get one extra item."""
    base, rem = divmod(n, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def all_gather_theta(theta_local, world=None):
    """theta_local [B_local, 85] (same B_local on every rank) -> [world * B_local, 85], rank-major."""
    import torch

    dist = _dist()
    if not dist.is_available() or not dist.is_initialized() or (dist.get_world_size() == 1 and not _force_collectives()):
        return theta_local
    world = dist.get_world_size() if world is None else world
    out = torch.empty((world * theta_local.shape[0],) + tuple(theta_local.shape[1:]), dtype=theta_local.dtype,
                      device=theta_local.device)
    dist.all_gather_into_tensor(out, theta_local.contiguous())
    return out


def all_gather_theta_ragged(theta_local, counts):
    """Ragged variant (shards of different sizes, e.g. a global batch that does not divide by the world size):
    pads to max(counts), gathers once, and strips the padding."""
    import torch

    dist = _dist()
    if not dist.is_initialized() or dist.get_world_size() == 1:
        return theta_local
    world = dist.get_world_size()
    mx = max(counts)
    pad = torch.zeros((mx,) + tuple(theta_local.shape[1:]), dtype=theta_local.dtype, device=theta_local.device)
    pad[: theta_local.shape[0]] = theta_local
    out = torch.empty((world * mx,) + tuple(theta_local.shape[1:]), dtype=theta_local.dtype, device=theta_local.device)
    dist.all_gather_into_tensor(out, pad)
    return torch.cat([out[r * mx : r * mx + counts[r]] for r in range(world)], 0)


def reduce_kp_loss(parts_local):
    """parts_local = tensor [numerator, count, ...] from kp_reprojection_loss(return_parts=True) on the local
    shard -> global loss sum(num) / sum(count) (0 if nothing is visible anywhere)."""
    import torch

    dist = _dist()
    nc = parts_local[:2].clone()
    if dist.is_initialized() and dist.get_world_size() > 1:
        dist.all_reduce(nc, op=dist.ReduceOp.SUM)
    return torch.where(nc[1] > 0, nc[0] / torch.clamp(nc[1], min=1.0), torch.zeros_like(nc[0]))


def reduce_losses(packed_local):
    """reduce_fn for Predictor.val_step -- the ONE collective of the config-5 losses: `packed_local`
    [n_stage, 4] holds (kp numerator, kp count, kp loss, mesh loss sum) of the local shard for every IEF stage; the whole
    block is summed over the ranks in a single all-reduce (12 floats at 3 stages).  kp_reprojection_loss normalises by the
    GLOBAL visible count, so column 2 is recomputed from the reduced numerator / count (0 if nothing is visible anywhere);
    the mesh loss is a plain sum over images.  Columns past the fourth (val_step(critic_loss_weight=...) appends the critic's three
    score sums and N) are plain sums too and ride in the same all-reduce: only column 2 is recomputed."""
    import torch

    dist = _dist()
    packed = packed_local.clone()
    if dist.is_initialized() and (dist.get_world_size() > 1 or _force_collectives()):
        dist.all_reduce(packed, op=dist.ReduceOp.SUM)
    num, cnt = packed[:, 0], packed[:, 1]
    packed[:, 2] = torch.where(cnt > 0, num / torch.clamp(cnt, min=1.0), torch.zeros_like(num))
    return packed


def _force_collectives():
    """HPE_FORCE_DIST=1: issue the collectives even in a world of one rank (rehearses the RCCL calls on a 1-GPU box)."""
    return bool(os.environ.get("HPE_FORCE_DIST"))


def reduce_sum(x):
    dist = _dist()
    x = x.clone()
    if dist.is_initialized() and dist.get_world_size() > 1:
        dist.all_reduce(x, op=dist.ReduceOp.SUM)
    return x


class _DevicePointer(object):
    """what ``torch.as_tensor`` needs to see device memory it does not own: the CUDA array interface (version 2) of ``count`` float64"""

    def __init__(self, ptr, count):
        self.__cuda_array_interface__ = {"shape": (int(count),), "typestr": "<f8", "data": (int(ptr), False), "strides": None, "version": 2}


def device_doubles(ptr, count, device):
    """the ``count`` float64 at address ``ptr`` of ``device`` as a 1-D tensor: a view, no copy; valid while the memory is.  A CPU device
    takes a host address (the gloo rehearsal of the callback on a host without a GPU)."""
    import torch

    if torch.device(device).type == "cpu":
        import ctypes

        import numpy as np

        return torch.from_numpy(np.ctypeslib.as_array((ctypes.c_double * int(count)).from_address(int(ptr))))
    return torch.as_tensor(_DevicePointer(ptr, count), device=device)


DEFAULT_TIMEOUT_S = 300.0  # of a process group made here: a rank that never arrives raises on the others instead of hanging them


class Reducer(object):
    """The sums that join the ranks of data-parallel training (DESIGN.md "Data-parallel training"), over one process group.

    ``nccl`` (RCCL): the all-reduce runs on the device tensor, on the current stream.  ``gloo``: the tensor is staged through ONE
    reused pinned host buffer -- device to host (which waits for the stream), the host all-reduce, host to device on the stream --
    gloo's own device support is not relied on.  A world of one rank is the identity unless ``HPE_FORCE_DIST`` is set
    (``active``).  CPU tensors go straight to the group.

    ``callback`` is the ``hpe_reduce_fn`` of ``HpeEngine.set_encoder_reduce``: it wraps the library's device buffer as a tensor
    without a copy and sums it over the ranks.  An exception inside it is caught and kept, the callback returns nonzero (the library
    call then fails with the layer's name), and ``reraise()`` -- which the engine calls once the library call has returned -- raises it.
    ``counts`` tallies the collectives issued, by kind: "hook", "grad", "block", "broadcast"."""

    def __init__(self, group=None, device=None):
        import torch

        from . import _lib

        dist = _dist()
        self.group = group
        self.initialized = dist.is_available() and dist.is_initialized()
        self.world = dist.get_world_size(group) if self.initialized else 1
        self.rank = dist.get_rank(group) if self.initialized else 0
        self.backend = dist.get_backend(group) if self.initialized else None
        self.active = self.initialized and (self.world > 1 or _force_collectives())
        self.device = torch.device(device) if device is not None else None
        self.counts = {"hook": 0, "grad": 0, "block": 0, "broadcast": 0}
        self._host = None
        self._exc = None
        self.callback = _lib.REDUCE_FN(self._hook)

    @classmethod
    def from_env(cls, backend=None, timeout_s=DEFAULT_TIMEOUT_S, device=None):
        """``init_from_env`` with a finite timeout on the group it creates -> a Reducer on the default group"""
        import datetime

        init_from_env(backend, timeout=datetime.timedelta(seconds=float(timeout_s)))
        return cls(device=device)

    # ------------------------------------------------------------------ transport
    def _staging(self, nbytes):
        """the first ``nbytes`` of the pinned host buffer (grown, never shrunk), as uint8"""
        import torch

        if self._host is None or self._host.numel() < nbytes:
            self._host = torch.empty(max(int(nbytes), 1 << 16), dtype=torch.uint8, pin_memory=torch.cuda.is_available())
        return self._host[:nbytes]

    def _collective(self, t, fn):
        """fn(tensor) on ``t`` in place: directly (CPU tensors, nccl) or through the staging buffer (a device tensor over gloo)"""
        if not t.is_contiguous():
            raise ValueError("Reducer: the tensor must be contiguous")
        if not t.is_cuda or self.backend == "nccl":
            fn(t)
            return t
        host = self._staging(t.numel() * t.element_size()).view(t.dtype).reshape(t.shape)
        host.copy_(t)  # a blocking copy: waits for what the stream holds
        fn(host)
        t.copy_(host, non_blocking=True)  # stream-ordered; the next staging copy is ordered behind it on the same stream
        return t

    def _sum(self, t):
        if self.active:
            dist = _dist()
            self._collective(t, lambda x: dist.all_reduce(x, op=dist.ReduceOp.SUM, group=self.group))
        return t

    # ------------------------------------------------------------------ the four uses
    def sum_grad(self, flat):
        """the flat gradient of one network, summed over the ranks in place: ONE all-reduce"""
        self.counts["grad"] += 1
        return self._sum(flat)

    def sum_block(self, block):
        """a small packed block of loss terms or counts, summed over the ranks in place: ONE all-reduce"""
        self.counts["block"] += 1
        return self._sum(block)

    def broadcast(self, t, src=0):
        """rank ``src``'s tensor into every rank's, in place"""
        self.counts["broadcast"] += 1
        if self.active:
            dist = _dist()
            src_global = dist.get_global_rank(self.group, src) if self.group is not None else src
            self._collective(t, lambda x: dist.broadcast(x, src=src_global, group=self.group))
        return t

    def barrier(self):
        if self.active:
            _dist().barrier(group=self.group)

    def _hook(self, user, ptr, count, stream):
        import torch

        try:
            self.counts["hook"] += 1
            if not self.active:
                return 0
            dev = self.device if self.device is not None else torch.device("cuda", torch.cuda.current_device())
            t = device_doubles(ptr, count, dev)
            if not t.is_cuda or (stream or 0) == torch.cuda.current_stream(dev).cuda_stream:
                self._sum(t)
            else:
                with torch.cuda.stream(torch.cuda.ExternalStream(stream or 0, device=dev)):
                    self._sum(t)
            return 0
        except BaseException as e:  # noqa: B902  nothing may unwind through the C frames of the library
            self._exc = e
            return 1

    def reraise(self):
        """raise, once, what the callback caught"""
        e, self._exc = self._exc, None
        if e is not None:
            raise e


class ShardedPredictor(object):
    """Wraps a per-rank ``Predictor``: every rank calls ``predict(global_images)`` (or passes only its shard with
    ``presharded=True``); returns the rank-local result dict plus ``theta_all`` = the all-gathered theta of the
    whole global batch.  Verts/joints stay rank-local (21 MB/rank at B = 256) unless a caller gathers them."""

    def __init__(self, predictor):
        self.predictor = predictor
        dist = _dist()
        self.world = dist.get_world_size() if dist.is_initialized() else 1
        self.rank = dist.get_rank() if dist.is_initialized() else 0

    def predict(self, images, presharded=False, all_stages=False):
        if not presharded:
            n = images.shape[0]
            lo, hi = shard_bounds(n, self.rank, self.world)
            counts = [shard_bounds(n, r, self.world)[1] - shard_bounds(n, r, self.world)[0] for r in range(self.world)]
            images = images[lo:hi]
        else:
            counts = None
        res = self.predictor.predict(images, all_stages=all_stages)
        if counts is not None and len(set(counts)) > 1:
            res["theta_all"] = all_gather_theta_ragged(res["theta"], counts)
        else:
            res["theta_all"] = all_gather_theta(res["theta"])
        return res

    def val_step(self, images, seg_gts, kp2d_gts, presharded=False, **kw):
        """Predictor.val_step on this rank's shard with the losses reduced over the ranks (one all-reduce per step)."""
        if not presharded:
            lo, hi = shard_bounds(images.shape[0], self.rank, self.world)
            images, seg_gts, kp2d_gts = images[lo:hi], seg_gts[lo:hi], kp2d_gts[lo:hi]
        return self.predictor.val_step(images, seg_gts, kp2d_gts, reduce_fn=reduce_losses, **kw)
