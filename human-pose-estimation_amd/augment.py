"""Training-batch augmentation on the GPU: the reference's ``DataLoader.image_preprocessing`` (src/data_loader.py:160-213) with
``jitter_center``, ``jitter_scale``, ``pad_image_edge``, ``random_flip`` and ``flip_image`` (src/util/data_utils.py:144-238) for a whole
batch in ONE launch (hpe_augment_batch, csrc/augment.hip), and ``mocap_real`` = ``preprocess_poses`` (src/data_loader.py:139-143).
The random draws are inputs (``draw_augmentation``), the way ``drop`` is an input to ``GeneratorTrainer.step``.  What is computed is
defined in DESIGN.md "Training-batch augmentation".  HIP-backed through include/hpe.h; no CPU fallback."""
from __future__ import annotations

import numpy as np

from . import _lib
from .batch_io import DecodedBatch, frame_offsets as packed_offsets, pinned, ptr as _p, stream_ptr, upload

IMG_SIZE = 224
NUM_KP = 19
TRANS_MAX = 20  # src/config.py:72
SCALE_RANGE = (0.8, 1.23)  # src/config.py:73-74
SWAP_INDS = (5, 4, 3, 2, 1, 0, 11, 10, 9, 8, 7, 6, 12, 13, 14, 16, 15, 18, 17)  # flip_image, src/util/data_utils.py:234-235
SWAP14 = SWAP_INDS[:14]  # the same swap on the 14 joints of the 3-D labels
PERM24 = (0, 2, 1, 3, 5, 4, 6, 8, 7, 9, 11, 10, 12, 14, 13, 15, 17, 16, 19, 18, 21, 20, 23, 22)  # the SMPL joints' left/right swap
# HpeAugmentFrame (include/hpe.h) as a numpy record
TABLE_DTYPE = _lib.record_dtype(_lib.HpeAugmentFrame)


def draw_augmentation(B, generator=None, trans_max=TRANS_MAX, scale_range=SCALE_RANGE):
    """The random draws of one batch as CPU tensors: ``trans`` int32 [B,2] in [-trans_max, trans_max) (jitter_center), ``scale``
    float32 [B] in [scale_range[0], scale_range[1]) (jitter_scale), ``flip`` bool [B] with probability 1/2 (random_flip)."""
    import torch

    B, trans_max = int(B), int(trans_max)
    lo, hi = float(scale_range[0]), float(scale_range[1])
    if B < 1 or trans_max < 0 or not 0.0 < lo <= hi:
        raise ValueError("need B >= 1, trans_max >= 0 and 0 < scale_range[0] <= scale_range[1]")
    if trans_max > 0:
        trans = torch.randint(-trans_max, trans_max, (B, 2), generator=generator, dtype=torch.int32)
    else:
        trans = torch.zeros((B, 2), dtype=torch.int32)
    scale = torch.rand(B, generator=generator, dtype=torch.float32) * (hi - lo) + lo
    flip = torch.rand(B, generator=generator, dtype=torch.float32) < 0.5
    return {"trans": trans, "scale": scale, "flip": flip}


def _host(x, dtype, shape, name):
    """a host value as a contiguous numpy array of ``shape`` (a device tensor is refused: nothing here reads the device)"""
    if hasattr(x, "is_cuda"):
        if x.is_cuda:
            raise ValueError("%s must live on the host" % name)
        x = x.detach().numpy()
    a = np.asarray(x)
    if a.shape != shape:
        raise ValueError("%s must have shape %s, got %s" % (name, list(shape), list(a.shape)))
    if dtype != np.float32 and a.dtype.kind not in "iub":
        raise ValueError("%s must be integers" % name)
    return np.ascontiguousarray(a, dtype=dtype)


def plan_augmentation(sizes, centers, draws, trans_max=TRANS_MAX, frame_offsets=None, seg_offsets=None, clamp=False, out=None):
    """hpe_augment_plan: the per-sample table of ``augment_batch`` as a numpy record array [B] of ``TABLE_DTYPE``.  Pure host code.
    sizes [B,2] (H, W), centers [B,2] (x, y), draws as ``draw_augmentation`` returns them; the offsets default to frames and masks
    packed back to back.  A window that leaves the image padded by 112 + trans_max + 50, where the reference's tf.slice raises, is a
    ValueError unless ``clamp``; with ``clamp`` the entry has ``inside`` 0 and the kernel clamps to the edge."""
    sizes = np.asarray(sizes)
    if sizes.ndim != 2 or sizes.shape[0] < 1:
        raise ValueError("sizes must have shape [B,2] with B >= 1")
    B = sizes.shape[0]
    sizes = _host(sizes, np.int32, (B, 2), "sizes")
    centers = _host(centers, np.int32, (B, 2), "centers")
    if not isinstance(draws, dict) or not {"trans", "scale", "flip"} <= set(draws):
        raise ValueError("draws must be a dict with 'trans', 'scale' and 'flip'")
    trans = _host(draws["trans"], np.int32, (B, 2), "draws['trans']")
    scale = _host(draws["scale"], np.float32, (B,), "draws['scale']")
    flip = _host(draws["flip"], np.uint8, (B,), "draws['flip']")
    area = sizes[:, 0].astype(np.int64) * sizes[:, 1]
    if frame_offsets is None:
        frame_offsets = np.concatenate([[0], np.cumsum(area[:-1] * 3)])
    if seg_offsets is None:
        seg_offsets = np.concatenate([[0], np.cumsum(area[:-1])])
    fo = _host(frame_offsets, np.int64, (B,), "frame_offsets")
    so = _host(seg_offsets, np.int64, (B,), "seg_offsets")
    if out is None:
        out = np.empty(B, TABLE_DTYPE)
    elif out.dtype != TABLE_DTYPE or out.shape != (B,) or not out.flags.c_contiguous:
        raise ValueError("out must be a contiguous record array [B] of TABLE_DTYPE")
    _lib.check(_lib.load().hpe_augment_plan(B, _p(sizes), _p(centers), _p(trans), _p(scale), _p(flip), int(trans_max), _p(fo), _p(so), _p(out)))
    if not clamp and not out["inside"].all():
        bad = np.flatnonzero(out["inside"] == 0)
        raise ValueError("the 224 x 224 window of sample(s) %s leaves the frame padded by %d pixels (pass clamp=True to clamp to the edge)"
                         % (bad.tolist(), IMG_SIZE // 2 + int(trans_max) + 50))
    return out


def _pack(items, channels, name):
    """-> (torch uint8 tensors or one tensor, sizes [B,2], byte offsets [B], total bytes).  A list is packed with every item on a 16-byte
    boundary, the way preprocess_batch packs its frames; a single tensor is used as it is."""
    import torch

    tail = "[H,W,3]" if channels else "[H,W]"
    as_t = lambda f: torch.as_tensor(np.ascontiguousarray(f) if isinstance(f, np.ndarray) else f)  # noqa: E731
    nd = 3 if channels else 2
    if isinstance(items, DecodedBatch):  # decode_jpeg_batch's buffer is this packing already
        if items.channels != (channels or 1):
            raise ValueError("%s must be decoded with %d channel(s)" % (name, channels or 1))
        return items.buffer, items.sizes, items.offsets, items.nbytes
    if isinstance(items, (list, tuple)):
        ts = [as_t(f) for f in items]
        if not ts:
            raise ValueError("%s is empty" % name)
        for t in ts:
            if t.dtype != torch.uint8 or t.dim() != nd or (channels and t.shape[2] != channels) or t.numel() < 1:
                raise ValueError("%s must be uint8 %s arrays or tensors" % (name, tail))
        sizes = np.array([[int(t.shape[0]), int(t.shape[1])] for t in ts], np.int64)
        return (ts, sizes) + packed_offsets(sizes, channels or 1)
    t = as_t(items)
    if t.dtype != torch.uint8 or t.dim() != nd + 1 or (channels and t.shape[3] != channels) or t.numel() < 1:
        raise ValueError("%s must be a uint8 [B,%s tensor or a list of uint8 %s" % (name, tail[1:], tail))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    B, H, W = (int(v) for v in t.shape[:3])
    per = H * W * (channels or 1)
    return t, np.tile(np.array([[H, W]], np.int64), (B, 1)), np.arange(B, dtype=np.int64) * per, B * per


def _to_device(packed, offs, total, dev):
    import torch

    if not isinstance(packed, list):
        return packed if packed.is_cuda else packed.to(dev, non_blocking=True)
    buf = torch.empty(total, dtype=torch.uint8, device=dev)
    for t, o in zip(packed, offs):
        buf[int(o):int(o) + t.numel()].copy_(t.reshape(-1), non_blocking=True)
    return buf


def augment_batch(frames, segs, kp, centers, draws=None, generator=None, trans_max=TRANS_MAX, scale_range=SCALE_RANGE, clamp=False,
                  out=None):
    """One training batch from raw samples, in one launch: -> (images [B,224,224,3] in [-1,1], seg_gts [B,224,224] in [0,1] (not
    thresholded: the mesh loss takes > 0), kp_gt [B,19,3] (x, y in [-1,1], visibility; invisible rows 0)) as CUDA float32 -- what
    ``GeneratorTrainer.step(images, kp_gt, seg_gts=seg_gts)`` takes.

    frames / segs: lists of uint8 [H_i,W_i,3] / [H_i,W_i] arrays or tensors (host or device; packed into one device buffer each here),
    single uint8 tensors [B,H,W,3] / [B,H,W], or ``decode_jpeg_batch``'s ``DecodedBatch`` (3 / 1 channels), whose buffer and offsets are
    used as they are.  kp [B,19,3] (x, y, visibility in source pixels; host or device), centers int [B,2]
    (x, y; host).  draws: ``draw_augmentation``'s dict (host), drawn here with ``generator`` when None.  A sample whose window leaves
    the padded frame is a ValueError unless ``clamp`` (``plan_augmentation``).  out: an optional (images, seg_gts, kp_gt) triple of
    preallocated contiguous float32 CUDA tensors.  Nothing reads the device; the table goes up from pinned memory without blocking."""
    import torch

    fpk, fsizes, foffs, ftotal = _pack(frames, 3, "frames")
    spk, ssizes, soffs, stotal = _pack(segs, 0, "segs")
    B = fsizes.shape[0]
    if ssizes.shape[0] != B or (fsizes != ssizes).any():
        raise ValueError("segs must match frames in count and in every [H,W]")
    if not isinstance(kp, torch.Tensor):
        kp = torch.as_tensor(np.ascontiguousarray(kp, dtype=np.float32))
    if tuple(kp.shape) != (B, NUM_KP, 3) or not kp.dtype.is_floating_point:
        raise ValueError("kp must be float [B,19,3] with B = %d" % B)
    if draws is None:
        draws = draw_augmentation(B, generator=generator, trans_max=trans_max, scale_range=scale_range)
    cuda_in = [t for t in (fpk if isinstance(fpk, list) else [fpk]) + (spk if isinstance(spk, list) else [spk]) + [kp] if t.is_cuda]
    dev = cuda_in[0].device if cuda_in else torch.device("cuda", torch.cuda.current_device())
    if any(t.device != dev for t in cuda_in):
        raise ValueError("frames, segs and kp must live on one device (or on the host)")
    shapes = ((B, IMG_SIZE, IMG_SIZE, 3), (B, IMG_SIZE, IMG_SIZE), (B, NUM_KP, 3))
    if out is not None:
        if len(out) != 3:
            raise ValueError("out must be an (images, seg_gts, kp_gt) triple")
        for t, s in zip(out, shapes):
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != s or t.dtype != torch.float32 or t.device != dev or not t.is_contiguous():
                raise ValueError("out must hold contiguous float32 CUDA tensors %s on %s" % (list(shapes), dev))
    with torch.cuda.device(dev):
        table_pinned, host = pinned(B * TABLE_DTYPE.itemsize)
        plan_augmentation(fsizes, centers, draws, trans_max=trans_max, frame_offsets=foffs, seg_offsets=soffs, clamp=clamp,
                          out=host.view(TABLE_DTYPE))
        fbuf = _to_device(fpk, foffs, ftotal, dev)
        sbuf = _to_device(spk, soffs, stotal, dev)
        kpd = kp.to(device=dev, dtype=torch.float32, non_blocking=True).contiguous()
        table_dev = upload(table_pinned, dev)
        if out is None:
            out = tuple(torch.empty(s, dtype=torch.float32, device=dev) for s in shapes)
        _lib.check(_lib.load().hpe_augment_batch(fbuf.data_ptr(), sbuf.data_ptr(), table_pinned.data_ptr(), table_dev.data_ptr(), kpd.data_ptr(), B,
                                                 out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), stream_ptr(dev)))
    return tuple(out)


def mocap_real(engine, poses, shapes):
    """The reference's ``preprocess_poses`` (src/data_loader.py:139-143) for N mocap rows: poses [N,72], shapes [N,10] (CUDA float32) ->
    the (joints [N,19,3], shapes [N,10], Rs [N,24,3,3]) triple that ``CriticTrainer.step`` / ``step_from_thetas`` take as ``real``.
    ``engine.smpl`` runs in chunks of ``max_batch`` rows, without gradient."""
    import torch

    if not isinstance(poses, torch.Tensor) or not isinstance(shapes, torch.Tensor) or not poses.is_cuda or not shapes.is_cuda:
        raise ValueError("poses and shapes must be CUDA tensors")
    if poses.dim() != 2 or shapes.dim() != 2 or poses.shape[1] != 72 or shapes.shape[1] != 10 or poses.shape[0] != shapes.shape[0] or \
            poses.shape[0] < 1 or poses.dtype != torch.float32 or shapes.dtype != torch.float32:
        raise ValueError("poses must be float32 [N,72] and shapes float32 [N,10]")
    N = poses.shape[0]
    shapes = shapes.detach().contiguous()
    cam = poses.new_zeros((N, 3))  # the camera does not enter joints or Rs
    cam[:, 0] = 1.0
    theta = torch.cat([cam, poses.detach(), shapes], dim=1)
    mb = engine.max_batch
    with torch.no_grad():
        parts = [engine.smpl(theta[lo:lo + mb], want=("joints", "Rs")) for lo in range(0, N, mb)]
    return torch.cat([p["joints"] for p in parts]), shapes, torch.cat([p["Rs"] for p in parts])


def reflect_pose(pose72):
    """The SMPL pose [..., 72] (24 axis-angle vectors) of the body mirrored about the x axis, in the record's own format: joint j takes
    the vector of joint ``PERM24[j]`` with signs (1, -1, -1).  In rotation space that is M R[PERM24[j]] M with M = diag(-1, 1, 1), the
    rule hpe_loss3d applies to a flipped row (DESIGN.md "3-D supervision").  Host arrays; applying it twice is the identity."""
    p = np.asarray(pose72)
    if p.shape[-1] != 72:
        raise ValueError("pose must be [..., 72], got %s" % (list(p.shape),))
    v = p.reshape(p.shape[:-1] + (24, 3))[..., list(PERM24), :] * np.asarray((1, -1, -1), p.dtype)
    return np.ascontiguousarray(v.reshape(p.shape))


def reflect_joints3d(j14):
    """The 3-D joints [..., 14, 3] of the body mirrored about the x axis: joint k takes (-x, y, z) of joint ``SWAP14[k]``.  Host arrays;
    applying it twice is the identity."""
    j = np.asarray(j14)
    if j.shape[-2:] != (14, 3):
        raise ValueError("joints must be [..., 14, 3], got %s" % (list(j.shape),))
    return np.ascontiguousarray(j[..., list(SWAP14), :] * np.asarray((-1, 1, 1), j.dtype))


def gt3d_real(engine, records, flip=None):
    """The 3-D ground truth of a batch as the 3-D losses take it (``ops.Gt3D``; DESIGN.md "3-D supervision"), beside ``mocap_real``.
    records: parsed image records (``parse_image_example`` dicts; 'gt3d' [14,3], 'pose' [72] and 'shape' [10] are each optional per
    record), or one dict of stacked host arrays under those keys (a key that is absent is absent for every row).  flip: the
    augmentation's draw (bool [B], host or device; None: no flips) -- the labels stay UNFLIPPED, the loss mirrors them.
    Absent fields are zeros.  w_joints = 1 where 'gt3d' is present; w_smpl = 1 where 'pose' and 'shape' both are; Rs come from ONE pass
    of ``engine.smpl`` over the ground-truth theta (chunks of ``max_batch`` rows, no gradient), exactly as ``mocap_real`` makes them;
    a row with 'pose' and 'shape' but no 'gt3d' takes its joints from that same pass and w_joints = 1."""
    import torch

    if isinstance(records, dict):
        B = len(next(iter(records.values()))) if records else 0
        records = [{k: v[i] for k, v in records.items()} for i in range(B)]
    B = len(records)
    if B < 1:
        raise ValueError("records is empty")
    j, pose, shape = np.zeros((B, 14, 3), np.float32), np.zeros((B, 72), np.float32), np.zeros((B, 10), np.float32)
    has_j, has_s = np.zeros(B, bool), np.zeros(B, bool)
    for i, r in enumerate(records):
        if r.get("gt3d") is not None:
            j[i], has_j[i] = np.asarray(r["gt3d"], np.float32).reshape(14, 3), True
        if r.get("pose") is not None and r.get("shape") is not None:
            pose[i], shape[i], has_s[i] = np.asarray(r["pose"], np.float32).reshape(72), np.asarray(r["shape"], np.float32).reshape(10), True
    dev = engine.tdev
    joints, shapes = torch.from_numpy(j).to(dev), torch.from_numpy(shape).to(dev)
    if has_s.any():
        cam = np.zeros((B, 3), np.float32)  # the camera does not enter joints or Rs
        cam[:, 0] = 1.0
        theta = torch.from_numpy(np.concatenate([cam, pose, shape], 1)).to(dev)
        mb = engine.max_batch
        with torch.no_grad():
            parts = [engine.smpl(theta[lo:lo + mb].contiguous(), want=("joints", "Rs")) for lo in range(0, B, mb)]
        Rs = torch.cat([p["Rs"] for p in parts])
        from_smpl = has_s & ~has_j
        if from_smpl.any():
            joints = torch.where(torch.from_numpy(from_smpl).to(dev)[:, None, None], torch.cat([p["joints"] for p in parts])[:, :14], joints)
            has_j = has_j | from_smpl
    else:
        Rs = torch.zeros((B, 24, 3, 3), dtype=torch.float32, device=dev)
    if flip is not None:
        flip = torch.as_tensor(np.asarray(flip.cpu()) if hasattr(flip, "cpu") else np.asarray(flip)).reshape(B).to(torch.bool).to(dev)
    from .ops import Gt3D

    return Gt3D(joints.contiguous(), Rs.contiguous(), shapes, torch.from_numpy(has_j.astype(np.float32)).to(dev),
                torch.from_numpy(has_s.astype(np.float32)).to(dev), flip)
