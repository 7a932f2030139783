"""The drawings of the training summaries on the device: ``draw_skeleton`` (the reference's src/util/renderer.py:286-447, cv2 circles
and lines) and ``draw_results`` (the panels of src/trainer.py:622-679: keypoints over the crop | the mesh over the crop | the mesh over
the silhouette, one row block per stage).  The skeleton is rasterised and the panel composed by csrc/draw.hip in one launch; the two
mesh columns come from ``SMPLRenderer``, batched.  The raster rules are this project's own, in exact integer arithmetic (DESIGN.md
"Training summaries": PARITY UNPINNED against cv2); ``draw_text`` needs a font and is not here, so the panel's sc / tx / ty / kpl values
are not drawn.  HIP-backed through include/hpe.h; no CPU fallback."""
from __future__ import annotations

import numpy as np

from . import _lib
from .batch_io import stream_ptr

NUM_JOINTS = 19
MAX_RADIUS = 256

# the reference's tables for the 19-joint skeleton (renderer.py:315-375), as data
COLORS = {
    "pink": (197, 27, 125), "light_pink": (233, 163, 201), "light_green": (161, 215, 106), "green": (77, 146, 33), "red": (215, 48, 39),
    "light_red": (252, 146, 114), "light_orange": (252, 141, 89), "purple": (118, 42, 131), "light_purple": (175, 141, 195),
    "light_blue": (145, 191, 219), "blue": (69, 117, 180), "gray": (130, 130, 130), "white": (255, 255, 255),
}
JCOLORS = ["light_pink", "light_pink", "light_pink", "pink", "pink", "pink", "light_blue", "light_blue", "light_blue", "blue", "blue", "blue",
           "purple", "purple", "red", "green", "green", "white", "white"]
PARENTS = [1, 2, 8, 9, 3, 4, 7, 8, 12, 12, 9, 10, 14, -1, 13, -1, -1, 15, 16]  # -1: no parent
ECOLORS = {0: "light_pink", 1: "light_pink", 2: "light_pink", 3: "pink", 4: "pink", 5: "pink", 6: "light_blue", 7: "light_blue", 8: "light_blue",
           9: "blue", 10: "blue", 11: "blue", 12: "purple", 17: "light_green", 18: "light_green", 14: "purple"}

_tables = {}


def skeleton_table():
    """int32 [19, 8]: parent, the joint's R, G, B, its edge's R, G, B (zeros without a parent), 0 -- what the kernels read"""
    t = np.zeros((NUM_JOINTS, 8), np.int32)
    for j in range(NUM_JOINTS):
        t[j, 0] = PARENTS[j]
        t[j, 1:4] = COLORS[JCOLORS[j]]
        if PARENTS[j] >= 0:
            t[j, 4:7] = COLORS[ECOLORS[j]]
    return t


def _table_dev(dev):
    import torch

    if dev not in _tables:
        _tables[dev] = torch.from_numpy(skeleton_table()).to(dev)
    return _tables[dev]


def default_radius(H, W):
    return max(4, int(np.mean([H, W]) * 0.01))


def draw_panels(images, kp_gt, kp_pred, rend_img, rend_seg):
    """``combined`` of every image: images fp32 [n,S,S,3] in [-1,1], kp_gt [n,19,3], kp_pred [n,T,19,2], rend_img / rend_seg uint8
    [n*T,S,S,3] (image-major, stage-minor) -> uint8 [n, T*S, 3*S, 3].  Column 0 is trunc(((img + 1) * 0.5) * 255) under the ground-truth
    joints as rings (visible ones) and the predicted skeleton; columns 1 and 2 are the rendered batches.  One launch on the current
    stream; nothing reads the device."""
    import torch

    if not (isinstance(images, torch.Tensor) and images.is_cuda and images.dim() == 4 and images.shape[1] == images.shape[2] and images.shape[3] == 3):
        raise ValueError("images must be a CUDA tensor [n,S,S,3]")
    dev, n, S = images.device, int(images.shape[0]), int(images.shape[1])
    images = images.to(torch.float32).contiguous()
    kp_gt = torch.as_tensor(kp_gt).to(dev, torch.float32).contiguous()
    kp_pred = torch.as_tensor(kp_pred).to(dev, torch.float32).contiguous()
    if kp_pred.dim() != 4 or kp_pred.shape[0] != n or tuple(kp_pred.shape[2:]) != (NUM_JOINTS, 2):
        raise ValueError("kp_pred must be [n,T,19,2] with n = %d, got %s" % (n, tuple(kp_pred.shape)))
    T = int(kp_pred.shape[1])
    if tuple(kp_gt.shape) != (n, NUM_JOINTS, 3):
        raise ValueError("kp_gt must be [n,19,3] with n = %d, got %s" % (n, tuple(kp_gt.shape)))
    for name, r in (("rend_img", rend_img), ("rend_seg", rend_seg)):
        if not (isinstance(r, torch.Tensor) and r.device == dev and r.dtype == torch.uint8 and tuple(r.shape) == (n * T, S, S, 3)):
            raise ValueError("%s must be a uint8 tensor [n*T,S,S,3] = %s on %s" % (name, (n * T, S, S, 3), dev))
    rend_img, rend_seg = rend_img.contiguous(), rend_seg.contiguous()
    out = torch.empty((n, T * S, 3 * S, 3), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().hpe_draw_panels(images.data_ptr(), kp_gt.data_ptr(), kp_pred.data_ptr(), rend_img.data_ptr(), rend_seg.data_ptr(),
                                               _table_dev(dev).data_ptr(), n, T, S, out.data_ptr(), stream_ptr(dev)))
    return out


def draw_skeleton(image, joints, draw_edges=True, vis=None, radius=None):
    """The reference's ``draw_skeleton`` for one image [H,W,3] of any size: a numpy array or a tensor, uint8 or float, returned as the
    same kind on the same device.  joints: [19,2] or [2,19] in pixels (rounded half to even); vis: [19], 0 = skip the joint and the
    edges to it; draw_edges False: rings of radius - 1 instead of discs and edges; radius: default max(4, int(mean(H, W) * 0.01)).
    A float image goes through uint8 as in the reference (x 255 when its maximum is <= 2, truncated, here also clamped to [0, 255]) and
    comes back as float32 (/ 255 when its maximum was <= 1).  Reading that maximum waits for the device; a uint8 tensor does not."""
    import torch

    is_np = isinstance(image, np.ndarray)
    t = torch.as_tensor(image)
    if t.dim() != 3 or t.shape[2] != 3:
        raise ValueError("image must be [H,W,3], got %s" % (tuple(t.shape),))
    dev = t.device if t.is_cuda else torch.device("cuda", torch.cuda.current_device())
    H, W = int(t.shape[0]), int(t.shape[1])
    t = t.to(dev)
    max_val = None
    if t.dtype != torch.uint8:
        t = t.float()
        max_val = float(t.max())
        work = torch.trunc(t * 255.0 if max_val <= 2.0 else t).clamp_(0, 255).to(torch.uint8)
    else:
        work = t.clone()
    work = work.contiguous()
    j = np.asarray(joints.detach().cpu() if isinstance(joints, torch.Tensor) else joints, np.float32)
    if j.shape[0] != 2:
        j = j.T
    if j.shape != (2, NUM_JOINTS):
        raise ValueError("joints must be [19,2] or [2,19]")
    jd = torch.from_numpy(np.ascontiguousarray(j.T)).to(dev)
    vd = None
    if vis is not None:
        v = np.asarray(vis.detach().cpu() if isinstance(vis, torch.Tensor) else vis).reshape(-1)
        if v.shape != (NUM_JOINTS,):
            raise ValueError("vis must be [19]")
        vd = torch.from_numpy((v != 0).astype(np.uint8)).to(dev)
    radius = default_radius(H, W) if radius is None else int(radius)
    if not 1 <= radius <= MAX_RADIUS:
        raise ValueError("radius must be in [1, %d]" % MAX_RADIUS)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().hpe_draw_skeleton(work.data_ptr(), jd.data_ptr(), None if vd is None else vd.data_ptr(), _table_dev(dev).data_ptr(), 1, H,
                                                 W, 1 if draw_edges else 0, radius, stream_ptr(dev)))
    if max_val is not None:
        # k / 255 through a table divided on the host: correctly rounded whatever the device's division does
        work = torch.from_numpy(np.arange(256, dtype=np.float32) / np.float32(255)).to(dev)[work.long()] if max_val <= 1.0 else work.float()
    if is_np:
        return work.cpu().numpy()
    return work if torch.as_tensor(image).is_cuda else work.cpu()


def draw_results(renderer, images, segs_gt, gt_kps, est_verts, pred_kps, cams):
    """The reference's ``draw_results`` up to the PNG: images fp32 [n,S,S,3] in [-1,1], segs_gt [n,S,S] or [n,S,S,1] in [0,1], gt_kps
    [n,19,3], est_verts [n,T,V,3], pred_kps [n,T,19,2], cams [n,T,3] (s, tx, ty) -> uint8 [n, T*S, 3*S, 3] on the device.  Two batched
    calls of ``renderer`` (an ``SMPLRenderer``) draw vert + [tx, ty, 5 / s] with cam_for_render = 0.5 * S * [5, 1, 1] over (img + 1) *
    0.5 and over the silhouette stacked to three channels; ``draw_panels`` composes.  Nothing reads the device."""
    import torch

    dev = images.device
    n, S = int(images.shape[0]), int(images.shape[1])
    est_verts = est_verts.to(dev, torch.float32)
    cams = cams.to(dev, torch.float32)
    T = int(est_verts.shape[1])
    f = 5.0
    cam_t = torch.stack([cams[..., 1], cams[..., 2], f / cams[..., 0]], dim=-1)  # [n,T,3]
    verts = (est_verts + cam_t[:, :, None, :]).reshape(n * T, -1, 3)
    cam_for_render = (0.5 * S * np.array([f, 1.0, 1.0])).astype(np.float32)
    # the backgrounds as uint8, as SMPLRenderer converts a float frame in [0, 1] (round(255 x)), without asking the device for its maximum
    bg = torch.round(((images.float() + 1.0) * 0.5) * 255.0).clamp_(0, 255).to(torch.uint8)
    seg = segs_gt.to(dev).float().reshape(n, S, S, 1)
    seg3 = torch.round(seg * 255.0).clamp_(0, 255).to(torch.uint8).expand(n, S, S, 3)
    rep = lambda x: x[:, None].expand(n, T, S, S, 3).reshape(n * T, S, S, 3).contiguous()  # noqa: E731
    rend_img = renderer(verts, cam_for_render, img=rep(bg))
    rend_seg = renderer(verts, cam_for_render, img=rep(seg3))
    return draw_panels(images, gt_kps, pred_kps, rend_img, rend_seg)
