"""3-D score timing (hpe_pose3d_scores): prints one JSON line, and writes it to --out (default profiles/pose3d_bench.json).

B = 64 and B = 256 images, 3 IEF stages, 19 joints of which 14 are scored and the 6890 vertices: seeded random clouds of body size, each
stage a rotated, scaled, shifted, noisy copy of the ground truth.  Timed with HIP events after 3 warm-up calls, median of 5 groups of 10
calls: the library call with preallocated outputs, the same through metrics.pose3d_scores, and the same four scores composed from
torch.linalg.svd on the same GPU (what a user had before this call; checked here to agree with the kernel).  The implied bandwidth counts
two reads of the clouds, float32: 2 * (n_stage + n_stage) * B * (P + K) * 12 bytes -- the prediction and the ground truth of every
(image, stage), each swept twice.  The same buffers are read by every call, so part of them may come from the last-level cache: it is an
implied figure, not a measured DRAM rate.  One run on a shared machine; there is no pass bar.

    python tools/pose3d_bench.py [--out profiles/pose3d_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from hpe_amd import _lib, metrics

N_STAGE, K, J, P, WARMUP, GROUPS, CALLS = 3, 19, 14, 6890, 3, 5, 10


def timed(fn):
    """-> (median, min, max) ms per call over GROUPS groups of CALLS calls"""
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    groups = []
    for _ in range(GROUPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CALLS):
            fn()
        e1.record()
        e1.synchronize()
        groups.append(e0.elapsed_time(e1) / CALLS)
    return [round(float(x), 5) for x in (np.median(groups), min(groups), max(groups))]


def make_clouds(B, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    gt_j, gt_v = torch.randn((B, K, 3), generator=g, device="cuda") * 0.3, torch.randn((B, P, 3), generator=g, device="cuda") * 0.3
    joints, verts = [], []
    for _ in range(N_STAGE):
        q = torch.randn((B, 4), generator=g, device="cuda")
        w, x, y, z = (q / q.norm(dim=1, keepdim=True)).unbind(1)
        R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                         2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(B, 3, 3)
        s = 0.8 + 0.4 * torch.rand((B, 1, 1), generator=g, device="cuda")
        t = 0.2 * torch.randn((B, 1, 3), generator=g, device="cuda")
        joints.append((s * gt_j @ R.transpose(1, 2) + t + 0.05 * torch.randn((B, K, 3), generator=g, device="cuda")).contiguous())
        verts.append((s * gt_v @ R.transpose(1, 2) + t + 0.05 * torch.randn((B, P, 3), generator=g, device="cuda")).contiguous())
    return joints, gt_j, verts, gt_v


def svd_align_error(X, Y):
    """mean |scale R (x - mu1) - (y - mu2)| per cloud, X, Y [N,M,3] float64: the HMR evaluation's compute_similarity_transform, batched"""
    X1, X2 = X - X.mean(1, keepdim=True), Y - Y.mean(1, keepdim=True)
    var1 = (X1 ** 2).sum((1, 2))
    Kmat = X1.transpose(1, 2) @ X2
    U, s, Vh = torch.linalg.svd(Kmat)
    V = Vh.transpose(1, 2)
    Z = torch.eye(3, dtype=X.dtype, device=X.device).repeat(X.shape[0], 1, 1)
    Z[:, 2, 2] = torch.sign(torch.linalg.det(U @ Vh))
    R = V @ Z @ U.transpose(1, 2)
    scale = (R @ Kmat).diagonal(dim1=1, dim2=2).sum(1) / var1
    return (scale[:, None, None] * X1 @ R.transpose(1, 2) - X2).norm(dim=2).mean(1)


def torch_scores(joints, gt_j, verts, gt_v):
    """[n_stage,B,4] = MPJPE, PA-MPJPE, PVE, PA-PVE from torch ops in float64, torch.linalg.svd for the two fits"""
    B = gt_j.shape[0]
    Xj, Xv = torch.stack(joints).double()[:, :, :J].reshape(-1, J, 3), torch.stack(verts).double().reshape(-1, P, 3)
    Yj, Yv = gt_j.double()[:, :J].repeat(N_STAGE, 1, 1), gt_v.double().repeat(N_STAGE, 1, 1)
    rx, ry = (Xj[:, 2] + Xj[:, 3])[:, None] / 2, (Yj[:, 2] + Yj[:, 3])[:, None] / 2
    out = torch.stack([((Xj - rx) - (Yj - ry)).norm(dim=2).mean(1), svd_align_error(Xj, Yj), ((Xv - rx) - (Yv - ry)).norm(dim=2).mean(1),
                       svd_align_error(Xv, Yv)], 1)
    return out.reshape(N_STAGE, B, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "pose3d_bench.json"))
    args = ap.parse_args()
    lib = _lib.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    res = {"tool": "pose3d_bench", "device": torch.cuda.get_device_name(0), "n_stage": N_STAGE, "joints": K, "scored_joints": J, "verts": P,
           "warmup": WARMUP, "groups": GROUPS, "calls_per_group": CALLS, "ms": "median, min, max over the groups",
           "note": "one run on a shared machine; implied GB/s = two float32 reads of every (image, stage)'s prediction and ground truth over the median"}
    for B in (64, 256):
        joints, gt_j, verts, gt_v = make_clouds(B, seed=B)
        w = torch.ones((B, K), device="cuda")
        w[:, J:] = 0
        err = torch.empty((N_STAGE, B, 2, K), device="cuda")
        summ = torch.empty((N_STAGE, B, 6), device="cuda")
        xf = torch.empty((N_STAGE, B, 2, 13), device="cuda")
        jp = (C.c_void_p * N_STAGE)(*[t.data_ptr() for t in joints])
        vp = (C.c_void_p * N_STAGE)(*[t.data_ptr() for t in verts])

        def call():
            _lib.check(lib.hpe_pose3d_scores(jp, gt_j.data_ptr(), w.data_ptr(), vp, gt_v.data_ptr(), N_STAGE, B, K, P, 2, 3, err.data_ptr(),
                                             summ.data_ptr(), xf.data_ptr(), st))

        r = {"pose3d_scores_ms": timed(call)}
        r["pose3d_scores_wrapper_ms"] = timed(lambda: metrics.pose3d_scores(joints, gt_j, verts, gt_v))
        r["pose3d_scores_joints_only_ms"] = timed(lambda: _lib.check(lib.hpe_pose3d_scores(
            jp, gt_j.data_ptr(), w.data_ptr(), None, None, N_STAGE, B, K, 0, 2, 3, err.data_ptr(), summ.data_ptr(), xf.data_ptr(), st)))
        call()
        r["torch_svd_ms"] = timed(lambda: torch_scores(joints, gt_j, verts, gt_v))
        ref = torch_scores(joints, gt_j, verts, gt_v)
        r["max_abs_diff_to_torch_svd_m"] = float((summ[..., :4].double() - ref).abs().max())
        nbytes = 2 * 2 * N_STAGE * B * (P + K) * 12
        r["bytes_two_reads"] = nbytes
        r["implied_GBps"] = round(nbytes / (r["pose3d_scores_ms"][0] * 1e-3) / 1e9, 1)
        r["torch_svd_over_kernel"] = round(r["torch_svd_ms"][0] / r["pose3d_scores_ms"][0], 1)
        res["B%d" % B] = r
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
