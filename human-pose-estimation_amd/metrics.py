"""Checkpoint scores (DESIGN.md "Checkpoint scores"): PCK of the 14 LSP joints and the foreground / background agreement of the projected
mesh's silhouette with the mask -- the numbers models of this family are compared by, where the validation losses depend on the loss
weights and compare with nothing.

``eval_scores`` is one ``hpe_eval_scores`` launch for all IEF stages of a batch (csrc/eval_scores.hip): per image and stage the
confusion counts tp, fp, fn, tn of the silhouette, the per-joint keypoint error in pixels, and per image the torso and head length of
the ground truth.  ``Scores`` sums those over the batches of a pass (plain sums in one float64 block, so one ``Reducer.sum_block`` makes
them the sums of every rank's shard) and ``Scores.result`` turns them into ratios.

    counts, kp_err, norm = eval_scores([st["verts2d"] for st in stages], faces_dev, seg_gts, kp_gt, [st["kp2d"] for st in stages])
    s = Scores(); s.add(counts, kp_err, norm); s.result()["pck_torso_0.2"]

The 3-D scores (DESIGN.md "3-D pose scores"): ``pose3d_scores`` is one ``hpe_pose3d_scores`` launch (csrc/pose3d_scores.hip) for all stages
of a batch -- per image and stage the root-aligned and the Procrustes-aligned error of every joint, MPJPE, PA-MPJPE, PVE, PA-PVE and both
similarity fits -- ``procrustes_align`` the fit alone, and ``Scores3D`` the sums and ratios, in millimetres.

    joint_err, summary, xform = pose3d_scores([st["joints"] for st in stages], joints_gt, [st["verts"] for st in stages], verts_gt)
    s = Scores3D(); s.add(joint_err, summary); s.result()["pa_mpjpe_mm"]
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

NUM_LSP_JOINTS = 14
PCK_ALPHAS = (0.1, 0.2, 0.5)
PCKH_ALPHAS = (0.5,)


def upload_faces(faces, num_verts, device):
    """host faces [F,3] -> int32 device tensor, every index checked against [0, num_verts): the library call cannot see a device
    list, and its kernel drops a face it could not read"""
    import torch

    f = np.asarray(faces)
    if f.ndim != 2 or f.shape[1] != 3 or f.shape[0] < 1 or not np.issubdtype(f.dtype, np.integer):
        raise _lib.HpeError("libhpe_hip error 1: hpe_eval_scores: faces must be an integer [F,3] array, got %s %s" % (f.dtype, f.shape))
    if f.min() < 0 or f.max() >= num_verts:
        raise _lib.HpeError("libhpe_hip error 1: hpe_eval_scores: face indices span [%d, %d], outside [0, %d)" % (f.min(), f.max(), num_verts))
    return torch.from_numpy(np.ascontiguousarray(f, dtype=np.int32)).to(device)


def _cuda_f32(t, name):
    if not (hasattr(t, "is_cuda") and t.is_cuda):
        raise TypeError("%s must be a CUDA tensor" % name)
    return t.float().contiguous()


def eval_scores(verts2d_list, faces, seg_gts, kp_gt, kp2d_list, img_size=None):
    """-> (counts int32 [n_stage,B,4] = tp, fp, fn, tn; kp_err float32 [n_stage,B,K] pixels, -1 where the joint is not visible; norm
    float32 [B,2] torso and head length in pixels, -1 where an end is not visible).  verts2d_list: per stage [B,P,2] CUDA tensors in
    the pixels of ``reproject_vertices``; faces: an int32 CUDA tensor [F,3] (``upload_faces``), or a host array, which is checked
    against P and uploaded; seg_gts [B,H,W(,1)], foreground where > 0; kp_gt [B,K,3] normalised x, y, visibility; kp2d_list per stage
    [B,K,2].  ``verts2d_list = None``: no silhouette part (counts is None; the image size then comes from seg_gts or ``img_size`` =
    (H, W)); ``kp_gt = None``: no keypoint part (kp_err and norm are None).  Enqueued on the current stream; nothing reads the device."""
    import torch

    lib = _lib.load()
    sil, kps = verts2d_list is not None, kp_gt is not None
    if not sil and not kps:
        raise ValueError("eval_scores: neither vertices nor keypoints are given")
    first = (verts2d_list if sil else kp2d_list)[0]
    dev, n = first.device, len(verts2d_list if sil else kp2d_list)
    B = int(first.shape[0])
    seg = None
    if seg_gts is not None:
        seg = _cuda_f32(seg_gts, "seg_gts")
        if seg.dim() == 4:
            seg = seg[..., 0].contiguous()
        H, W = int(seg.shape[1]), int(seg.shape[2])
    elif img_size is not None:
        H, W = int(img_size[0]), int(img_size[1])
    else:
        raise ValueError("eval_scores: the image size is needed: pass seg_gts or img_size=(H, W)")
    v_ptrs = k_ptrs = f_ptr = seg_ptr = gt_ptr = None
    counts = kp_err = norm = None
    P = F = K = 0
    if sil:
        if seg is None or int(seg.shape[0]) != B:
            raise ValueError("eval_scores: one mask per image is needed")
        verts = [_cuda_f32(t, "verts2d") for t in verts2d_list]
        P = int(verts[0].shape[1])
        if any(tuple(t.shape) != (B, P, 2) for t in verts):
            raise ValueError("eval_scores: every stage's verts2d must be [%d, %d, 2]" % (B, P))
        if not (hasattr(faces, "is_cuda") and faces.is_cuda):
            faces = upload_faces(faces, P, dev)
        if faces.dtype != torch.int32 or faces.dim() != 2 or faces.shape[1] != 3 or not faces.is_contiguous():
            raise TypeError("eval_scores: device faces must be a contiguous int32 [F,3] tensor")
        F = int(faces.shape[0])
        v_ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in verts])
        f_ptr, seg_ptr = faces.data_ptr(), seg.data_ptr()
        counts = torch.empty((n, B, 4), dtype=torch.int32, device=dev)
    if kps:
        gt = _cuda_f32(kp_gt, "kp_gt")
        K = int(gt.shape[1])
        kp2d = [_cuda_f32(t, "kp2d") for t in kp2d_list]
        if len(kp2d) != n or tuple(gt.shape) != (B, K, 3) or any(tuple(t.shape) != (B, K, 2) for t in kp2d):
            raise ValueError("eval_scores: kp_gt must be [%d, K, 3] and every stage's kp2d [%d, K, 2], one per stage" % (B, B))
        k_ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in kp2d])
        gt_ptr = gt.data_ptr()
        kp_err = torch.empty((n, B, K), dtype=torch.float32, device=dev)
        norm = torch.empty((B, 2), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(lib.hpe_eval_scores(v_ptrs, f_ptr, F, seg_ptr, gt_ptr, k_ptrs, n, B, P, K, H, W, None if counts is None else counts.data_ptr(),
                                       None if kp_err is None else kp_err.data_ptr(), None if norm is None else norm.data_ptr(), st))
    return counts, kp_err, norm


def image_iou(counts):
    """counts [..., 4] -> float64 tp / (tp + fp + fn) per image, NaN where the union is empty"""
    c = counts.double()
    union = c[..., 0] + c[..., 1] + c[..., 2]
    return c[..., 0] / union.where(union > 0, union.new_tensor(float("nan")))


class Scores(object):
    """Plain sums of ``eval_scores`` outputs over the batches of a pass, one float64 row per IEF stage (``sums`` [n_stage, M], on the
    device of what is added: ``add`` reads nothing back).  Per stage: the four pixel counts, the sum of the per-image IoU and the number
    of images with a non-empty union, the number of images, the pixel-error sum over visible joints, and per joint 0..13 the hit and
    visible counts of every threshold.

    ``result()``:
      tp, fp, fn, tn the pixel counts of the pass ("positive" = covered by the projected mesh)
      iou            pooled tp / (tp + fp + fn)
      iou_mean       mean of the per-image IoU over the images whose union is not empty (``iou_images`` of them; ``iou_empty_union``
                     images, with neither a silhouette nor a mask, are left out)
      fb_accuracy    (tp + tn) / (H W N);  fb_f1 = 2 tp / (2 tp + fp + fn)
      pck_torso_<a>  for a in ``pck_alphas``: the share of visible joints 0..13 with error <= a * torso, over the images whose torso
                     (left shoulder to right hip of the ground truth) has both ends visible and a positive length
                     (``torso_invalid_images`` are left out)
      pckh_<a>       for a in ``pckh_alphas``: the same on the head segment (head top to neck).  This is the ANNOTATED head segment of
                     the 14 LSP joints, not MPII's head-box rule (0.6 x the box diagonal): the records hold no head box
      mean_px_error  mean error of the visible joints 0..13, all images
      pck_per_joint  pck_torso at ``per_joint_alpha`` (0.2) for each of the 14 joints (NaN for a joint never visible)
      images, kp_images  how many images the silhouette part and the keypoint part have seen
    A ratio whose denominator is 0 is NaN."""

    def __init__(self, pck_alphas=PCK_ALPHAS, pckh_alphas=PCKH_ALPHAS, per_joint_alpha=0.2, num_joints=NUM_LSP_JOINTS):
        self.pck_alphas, self.pckh_alphas = tuple(float(a) for a in pck_alphas), tuple(float(a) for a in pckh_alphas)
        self.per_joint_alpha, self.J = float(per_joint_alpha), int(num_joints)
        if self.per_joint_alpha not in self.pck_alphas:
            raise ValueError("per_joint_alpha %g is not among pck_alphas %s" % (self.per_joint_alpha, self.pck_alphas))
        # columns: tp fp fn tn | iou_sum iou_images images | px_sum px_count kp_images torso_images head_images |
        #          per torso alpha: hits[J] | torso visible[J] | per head alpha: hits[J] | head visible[J]
        self._joint0 = 12
        self.M = self._joint0 + self.J * (len(self.pck_alphas) + 1 + len(self.pckh_alphas) + 1)
        self.sums = None

    def _block(self, n, like):
        import torch

        if self.sums is None:
            self.sums = torch.zeros((n, self.M), dtype=torch.float64, device=like.device)
        if self.sums.shape[0] != n:
            raise ValueError("Scores: %d stages were added before, now %d" % (self.sums.shape[0], n))
        return self.sums

    @staticmethod
    def _tensor(x):
        import torch

        return x if hasattr(x, "is_cuda") else torch.from_numpy(np.asarray(x))

    def add(self, counts=None, kp_err=None, norm=None):
        """one batch: counts [n_stage,B,4], kp_err [n_stage,B,K], norm [B,2] (tensors or arrays; a part that is None adds nothing)"""
        import torch

        if counts is not None:
            c = self._tensor(counts).double()
            s = self._block(c.shape[0], c)
            iou = image_iou(c)
            some = ~torch.isnan(iou)
            s[:, 0:4] += c.sum(1)
            s[:, 4] += torch.where(some, iou, torch.zeros_like(iou)).sum(1)
            s[:, 5] += some.sum(1)
            s[:, 6] += c.shape[1]
        if kp_err is not None:
            J = self.J
            e = self._tensor(kp_err).double()[:, :, :J]
            nm = self._tensor(norm).double().to(e.device)
            if e.shape[2] != J:
                raise ValueError("Scores: kp_err holds %d joints, %d are scored" % (e.shape[2], J))
            s = self._block(e.shape[0], e)
            vis = e >= 0
            s[:, 7] += torch.where(vis, e, torch.zeros_like(e)).sum((1, 2))
            s[:, 8] += vis.sum((1, 2))
            s[:, 9] += e.shape[1]
            col = self._joint0
            for c_norm, alphas in ((0, self.pck_alphas), (1, self.pckh_alphas)):
                length = nm[:, c_norm]
                ok = length > 0  # -1 marks an end that is not visible; a zero length normalises nothing
                s[:, 10 + c_norm] += ok.sum()
                scored = vis & ok[None, :, None]
                for a in alphas:
                    s[:, col:col + J] += (scored & (e <= a * length[None, :, None])).sum(1)
                    col += J
                s[:, col:col + J] += scored.sum(1)
                col += J
        return self

    def reduce(self, reducer):
        """the sums of every rank, in ONE ``Reducer.sum_block``: a data-parallel pass then scores the whole set, not this rank's shard"""
        if self.sums is None:
            raise ValueError("Scores.reduce: nothing was added")
        reducer.sum_block(self.sums)
        return self

    def result_tensors(self, stage=-1):
        """``result`` as 0-dim float64 tensors (``pck_per_joint`` [J]) on the device of the sums: nothing is read back"""
        if self.sums is None:
            raise ValueError("Scores.result: nothing was added")
        s, J = self.sums[stage], self.J
        nan = s.new_tensor(float("nan"))

        def ratio(a, b):
            return a / b.where(b > 0, nan)

        tp, fp, fn, tn = s[0], s[1], s[2], s[3]
        out = {"tp": tp, "fp": fp, "fn": fn, "tn": tn, "iou": ratio(tp, tp + fp + fn), "iou_mean": ratio(s[4], s[5]), "iou_images": s[5], "iou_empty_union": s[6] - s[5],
               "fb_accuracy": ratio(tp + tn, tp + fp + fn + tn), "fb_f1": ratio(2 * tp, 2 * tp + fp + fn), "images": s[6],
               "mean_px_error": ratio(s[7], s[8]), "kp_images": s[9], "torso_invalid_images": s[9] - s[10], "head_invalid_images": s[9] - s[11]}
        col = self._joint0
        for name, alphas in (("pck_torso", self.pck_alphas), ("pckh", self.pckh_alphas)):
            seen = s[col + J * len(alphas):col + J * (len(alphas) + 1)]
            for a in alphas:
                hits = s[col:col + J]
                out["%s_%g" % (name, a)] = ratio(hits.sum(), seen.sum())
                if name == "pck_torso" and a == self.per_joint_alpha:
                    out["pck_per_joint"] = ratio(hits, seen)
                col += J
            col += J
        return out

    def result(self, stage=-1):
        """the scores of one stage (default: the last) as Python floats and ints, ``pck_per_joint`` as a list: ONE transfer"""
        import torch

        t = self.result_tensors(stage)
        keys = [k for k in t if k != "pck_per_joint"]
        host = torch.cat([torch.stack([t[k] for k in keys]), t["pck_per_joint"]]).cpu().numpy()
        out = {k: float(v) for k, v in zip(keys, host)}
        for k in ("tp", "fp", "fn", "tn", "iou_images", "iou_empty_union", "images", "kp_images", "torso_invalid_images", "head_invalid_images"):
            out[k] = int(out[k])
        out["pck_per_joint"] = [float(v) for v in host[len(keys):]]
        return out

    def results(self):
        """``result`` of every stage"""
        return [self.result(i) for i in range(self.sums.shape[0])]


# ---------------------------------------------------------------------------------------------- 3-D scores (DESIGN.md "3-D pose scores")
POSE3D_FLAG_ROOT, POSE3D_FLAG_PA_JOINTS, POSE3D_FLAG_PA_VERTS, POSE3D_FLAG_NO_VERTS = 1, 2, 4, 8  # summary[..., 5] of hpe_pose3d_scores
PCK3D_THRESHOLDS_MM = tuple(range(0, 151, 5))  # the thresholds auc3d averages over; the last is pck3d_150's


def _launch_pose3d(joints, joints_gt, weights, verts, verts_gt, roots, want=(True, True, True)):
    """one hpe_pose3d_scores launch on checked, contiguous float32 CUDA tensors -> (joint_err, summary, xform), None where not wanted"""
    import torch

    lib = _lib.load()
    n, dev = len(joints), joints_gt.device
    B, K = int(joints_gt.shape[0]), int(joints_gt.shape[1])
    P = int(verts_gt.shape[1]) if verts_gt is not None else 0
    j_ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in joints])
    v_ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in verts]) if verts is not None else None
    joint_err = torch.empty((n, B, 2, K), dtype=torch.float32, device=dev) if want[0] else None
    summary = torch.empty((n, B, 6), dtype=torch.float32, device=dev) if want[1] else None
    xform = torch.empty((n, B, 2, 13), dtype=torch.float32, device=dev) if want[2] else None
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    with torch.cuda.device(dev):
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(lib.hpe_pose3d_scores(j_ptrs, joints_gt.data_ptr(), ptr(weights), v_ptrs, ptr(verts_gt), n, B, K, P, int(roots[0]), int(roots[1]),
                                         ptr(joint_err), ptr(summary), ptr(xform), st))
    return joint_err, summary, xform


def pose3d_scores(joints_list, joints_gt, verts_list=None, verts_gt=None, joint_weights=None, roots=(2, 3), num_joints=NUM_LSP_JOINTS):
    """-> (joint_err float32 [n_stage,B,2,K]: row 0 the root-aligned, row 1 the Procrustes-aligned error of every joint, -1 where the joint
    is not scored, NaN where the alignment is undefined; summary float32 [n_stage,B,6] = MPJPE, PA-MPJPE, PVE, PA-PVE, scored joints,
    flags (``POSE3D_FLAG_*``); xform float32 [n_stage,B,2,13] = scale, R row-major, t of the joint fit and of the vertex fit), all in the
    units of the inputs (``Scores3D`` reports millimetres).  joints_list: per stage [B,K,3] CUDA tensors; joints_gt [B,K,3]; the first
    ``num_joints`` of the K keypoints are scored (None: all), and of those the ones whose ``joint_weights`` [B,K] entry is > 0;
    ``roots``: the two joints whose mean is the root (the hips in LSP order).  verts_list per stage [B,P,3] with verts_gt [B,P,3], or
    neither: joints only.  ONE ``hpe_pose3d_scores`` launch on the current stream; nothing reads the device."""
    import torch

    gt = _cuda_f32(joints_gt, "joints_gt")
    if gt.dim() != 3 or gt.shape[2] != 3:
        raise ValueError("pose3d_scores: joints_gt must be [B, K, 3], got %s" % (tuple(gt.shape),))
    B, K = int(gt.shape[0]), int(gt.shape[1])
    joints = [_cuda_f32(t, "joints") for t in joints_list]
    if not joints or any(tuple(t.shape) != (B, K, 3) for t in joints):
        raise ValueError("pose3d_scores: every stage's joints must be [%d, %d, 3]" % (B, K))
    if (verts_list is None) != (verts_gt is None):
        raise ValueError("pose3d_scores: verts_list and verts_gt are given together or not at all")
    verts = vgt = None
    if verts_gt is not None:
        vgt = _cuda_f32(verts_gt, "verts_gt")
        verts = [_cuda_f32(t, "verts") for t in verts_list]
        if vgt.dim() != 3 or vgt.shape[0] != B or vgt.shape[2] != 3 or len(verts) != len(joints) or any(t.shape != vgt.shape for t in verts):
            raise ValueError("pose3d_scores: verts_gt must be [%d, P, 3] and every stage's verts the same, one per stage" % B)
    J = K if num_joints is None else int(num_joints)
    if not 1 <= J <= K:
        raise ValueError("pose3d_scores: num_joints %d outside [1, %d]" % (J, K))
    w = None
    if joint_weights is not None:
        w = _cuda_f32(joint_weights, "joint_weights")
        if tuple(w.shape) != (B, K):
            raise ValueError("pose3d_scores: joint_weights must be [%d, %d]" % (B, K))
    if J < K:  # the joints past num_joints are not scored: zero weights, no copy of the clouds
        w = torch.ones((B, K), dtype=torch.float32, device=gt.device) if w is None else w.clone()
        w[:, J:] = 0
    return _launch_pose3d(joints, gt, w, verts, vgt, roots)


def procrustes_align(src, dst, weights=None):
    """The similarity transform that best maps ``src`` onto ``dst`` ([N,3] or [B,N,3] CUDA tensors) over the points whose weight is > 0
    -> (aligned = scale * src R^T + t, scale [B], R [B,3,3], t [B,3]), without the batch axis for [N,3] inputs; NaN where the fit is
    undefined (fewer than 3 points, or all of ``src`` in one place).  The fit is the joint fit of one ``hpe_pose3d_scores`` launch."""
    s, d = _cuda_f32(src, "src"), _cuda_f32(dst, "dst")
    single = s.dim() == 2
    if single:
        s, d = s[None], d[None]
        weights = None if weights is None else weights[None]
    if s.dim() != 3 or s.shape[2] != 3 or s.shape != d.shape:
        raise ValueError("procrustes_align: src and dst must both be [N, 3] or [B, N, 3]")
    w = None if weights is None else _cuda_f32(weights, "weights")
    if w is not None and tuple(w.shape) != tuple(s.shape[:2]):
        raise ValueError("procrustes_align: weights must be %s" % (tuple(s.shape[:2]),))
    x = _launch_pose3d([s], d, w, None, None, (0, 0), want=(False, False, True))[2][0, :, 0]
    scale, R, t = x[:, 0], x[:, 1:10].reshape(-1, 3, 3), x[:, 10:13]
    aligned = scale[:, None, None] * (s @ R.transpose(1, 2)) + t[:, None, :]
    return (aligned[0], scale[0], R[0], t[0]) if single else (aligned, scale, R, t)


class Scores3D(object):
    """Plain sums of ``pose3d_scores`` outputs over the batches of a pass, one float64 row per IEF stage (``sums`` [n_stage, M], on the
    device of what is added: ``add`` reads nothing back), so one ``Reducer.sum_block`` makes them the sums of every rank's shard.

    ``result()``, lengths in millimetres (the inputs times ``to_mm``, 1000 for metres):
      mpjpe_mm, pa_mpjpe_mm   mean root-aligned / Procrustes-aligned error over the scored joints 0..J-1 of the images where that
                              alignment is defined (``root_invalid_images`` / ``pa_invalid_images`` are left out)
      pve_mm, pa_pve_mm       mean over the images of the per-image vertex error (images without vertices or without that alignment are
                              left out)
      mpjpe_per_joint_mm, pa_mpjpe_per_joint_mm   the first two for each joint (NaN for a joint never scored)
      pck3d_150               the share of those joints whose root-aligned error is at most 150 mm
      auc3d                   the mean of that share over the thresholds 0, 5, ..., 150 mm
      images, pa_invalid_images, root_invalid_images
    A ratio whose denominator is 0 is NaN; a NaN coordinate in a scored point makes the sums it enters NaN."""

    def __init__(self, num_joints=NUM_LSP_JOINTS, to_mm=1000.0):
        self.J, self.to_mm = int(num_joints), float(to_mm)
        # columns: images root_invalid pa_invalid | pve_sum pve_images pa_pve_sum pa_pve_images | root err sum[J] | root count[J] |
        #          pa err sum[J] | pa count[J] | hits per threshold[T]
        self._joint0, self.T = 7, len(PCK3D_THRESHOLDS_MM)
        self.M = self._joint0 + 4 * self.J + self.T
        self.sums = None

    def add(self, joint_err, summary, xform=None):
        """one batch: joint_err [n_stage,B,2,K >= J], summary [n_stage,B,6] (tensors or arrays); xform is taken and not read, so that
        ``add(*pose3d_scores(...))`` works"""
        import torch

        J, j0 = self.J, self._joint0
        e = Scores._tensor(joint_err).double()
        sm = Scores._tensor(summary).double().to(e.device)
        if e.dim() != 4 or e.shape[2] != 2 or e.shape[3] < J or sm.shape != e.shape[:2] + (6,):
            raise ValueError("Scores3D: joint_err must be [n_stage, B, 2, K >= %d] and summary [n_stage, B, 6]" % J)
        n = e.shape[0]
        if self.sums is None:
            self.sums = torch.zeros((n, self.M), dtype=torch.float64, device=e.device)
        if self.sums.shape[0] != n:
            raise ValueError("Scores3D: %d stages were added before, now %d" % (self.sums.shape[0], n))
        s = self.sums
        flags = sm[:, :, 5].long()
        root_ok, pa_ok = (flags & POSE3D_FLAG_ROOT) == 0, (flags & POSE3D_FLAG_PA_JOINTS) == 0
        has_v = (flags & POSE3D_FLAG_NO_VERTS) == 0
        pve_ok, pa_pve_ok = root_ok & has_v, has_v & ((flags & POSE3D_FLAG_PA_VERTS) == 0)
        zero = torch.zeros((), dtype=torch.float64, device=e.device)
        s[:, 0] += e.shape[1]
        s[:, 1] += (~root_ok).sum(1)
        s[:, 2] += (~pa_ok).sum(1)
        s[:, 3] += torch.where(pve_ok, sm[:, :, 2] * self.to_mm, zero).sum(1)
        s[:, 4] += pve_ok.sum(1)
        s[:, 5] += torch.where(pa_pve_ok, sm[:, :, 3] * self.to_mm, zero).sum(1)
        s[:, 6] += pa_pve_ok.sum(1)
        e0, e1 = e[:, :, 0, :J] * self.to_mm, e[:, :, 1, :J] * self.to_mm
        # -1 in both rows marks a joint that is not scored; an error is never negative, and a NaN (an undefined alignment, a NaN
        # coordinate) compares false here, so its joint counts as scored, as it is
        scored = ~((e0 < 0) & (e1 < 0))
        r_on, p_on = scored & root_ok[:, :, None], scored & pa_ok[:, :, None]
        s[:, j0:j0 + J] += torch.where(r_on, e0, zero).sum(1)
        s[:, j0 + J:j0 + 2 * J] += r_on.sum(1)
        s[:, j0 + 2 * J:j0 + 3 * J] += torch.where(p_on, e1, zero).sum(1)
        s[:, j0 + 3 * J:j0 + 4 * J] += p_on.sum(1)
        thr = torch.tensor(PCK3D_THRESHOLDS_MM, dtype=torch.float64, device=e.device)
        s[:, j0 + 4 * J:] += (r_on[..., None] & (e0[..., None] <= thr)).sum((1, 2))
        return self

    def reduce(self, reducer):
        """the sums of every rank, in ONE ``Reducer.sum_block``"""
        if self.sums is None:
            raise ValueError("Scores3D.reduce: nothing was added")
        reducer.sum_block(self.sums)
        return self

    def result(self, stage=-1):
        """the scores of one stage (default: the last) as Python floats, ints and lists: ONE transfer"""
        if self.sums is None:
            raise ValueError("Scores3D.result: nothing was added")
        s, J, j0 = self.sums[stage].cpu().numpy(), self.J, self._joint0

        def ratio(a, b):
            with np.errstate(invalid="ignore", divide="ignore"):
                return np.where(b > 0, a / np.where(b > 0, b, 1.0), np.nan)

        r_sum, r_cnt, p_sum, p_cnt = (s[j0 + i * J:j0 + (i + 1) * J] for i in range(4))
        share = ratio(s[j0 + 4 * J:], r_cnt.sum())
        return {"mpjpe_mm": float(ratio(r_sum.sum(), r_cnt.sum())), "pa_mpjpe_mm": float(ratio(p_sum.sum(), p_cnt.sum())),
                "pve_mm": float(ratio(s[3], s[4])), "pa_pve_mm": float(ratio(s[5], s[6])),
                "mpjpe_per_joint_mm": [float(v) for v in ratio(r_sum, r_cnt)], "pa_mpjpe_per_joint_mm": [float(v) for v in ratio(p_sum, p_cnt)],
                "pck3d_150": float(share[-1]), "auc3d": float(share.mean()), "images": int(s[0]), "pa_invalid_images": int(s[2]),
                "root_invalid_images": int(s[1])}

    def results(self):
        """``result`` of every stage"""
        return [self.result(i) for i in range(self.sums.shape[0])]
