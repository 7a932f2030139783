"""augment_batch timed against its yardstick on the same GPU, in the same process: a torch-on-GPU restatement of the same steps (per
sample: interpolate, pad(mode="replicate") by 182, slice, flip, for the image and for the mask) -- what a user without the kernel would
run on the device.  Prints one JSON line and a table, writes profiles/augment_bench.json; sets no gate.

Rows at B in {8, 64, 256}, device-resident frames with sides drawn from [150, 500]:
  hip_launch_ms        hpe_augment_batch alone (table already on the device, outputs preallocated)
  hip_python_ms        the whole augment_batch call on lists of device tensors (packing copies, plan, table upload, launch, allocation)
  hip_python_out_ms    the same with preallocated ``out``
  torch_ms             the restatement
  generator_step_ms    one GeneratorTrainer.step from features with kp_gt and seg_gts (the encoder's forward is not in it, so the share
                       reported is an upper bound of the share of a step from images)
and the achieved GB/s of the launch on the algorithmic bytes: the outputs (224 * 224 * 16 + 19 * 12 bytes per sample) plus the source
bytes inside each window (4 bytes per source pixel of the rows and columns the window's taps span), beside the 6.29 TB/s the
microarchitecture guide measured for a device copy.

The method of tools/critic_bench.py: every shape is warmed up, each window is `--iters` calls between two device events (median of
`--repeats` windows, the variants alternated inside each repeat, spread = max - min beside every median), no profiler attached.

    python tools/augment_bench.py [--iters N] [--repeats R] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np
import torch

import hpe_amd
from hpe_amd import _lib, augment, synthetic
import regressor_train_ref as T
from critic_bench import measure

COPY_TBS = 6.29
MS = 112 + 20 + 50


def make_batch(B, seed):
    g = np.random.RandomState(seed)
    gen = torch.Generator(device="cuda").manual_seed(seed)
    sizes = g.randint(150, 501, (B, 2))
    frames = [torch.randint(0, 256, (int(h), int(w), 3), generator=gen, device="cuda", dtype=torch.uint8) for h, w in sizes]
    segs = [(torch.randint(0, 2, (int(h), int(w)), generator=gen, device="cuda", dtype=torch.uint8) * 255) for h, w in sizes]
    centers = np.stack([g.randint(sizes[:, 1] // 4, 3 * sizes[:, 1] // 4), g.randint(sizes[:, 0] // 4, 3 * sizes[:, 0] // 4)], 1).astype(np.int32)
    kp = np.concatenate([g.uniform(0, 1, (B, 19, 2)) * sizes[:, None, ::-1], np.ones((B, 19, 1))], 2).astype(np.float32)
    draws = augment.draw_augmentation(B, generator=torch.Generator().manual_seed(seed))
    return sizes, frames, segs, torch.from_numpy(kp).cuda(), centers, draws


def torch_restatement(frames, segs, table):
    """the same steps with torch ops on the device, materialising every stage (keypoints left out: 57 numbers per sample)"""
    imgs, sgs = [], []
    for f, s, t in zip(frames, segs, table):
        x = torch.cat([f.permute(2, 0, 1), s[None]]).float().mul_(1.0 / 255.0)[None]
        x = torch.nn.functional.interpolate(x, size=(int(t["newH"]), int(t["newW"])), mode="bilinear", align_corners=False, antialias=False)
        x = torch.nn.functional.pad(x, (MS, MS, MS, MS), mode="replicate")
        sy, sx = int(t["cy"]) + MS - 112, int(t["cx"]) + MS - 112
        x = x[0, :, sy:sy + 224, sx:sx + 224]
        if t["flip"]:
            x = x.flip(2)
        imgs.append((2.0 * (x[:3] - 0.5)).permute(1, 2, 0))
        sgs.append(x[3])
    return torch.stack(imgs), torch.stack(sgs)


def algorithmic_bytes(table):
    total = 0
    for t in table:
        rows = min(int(t["cy"]) + 111, int(t["newH"]) - 1) - max(int(t["cy"]) - 112, 0) + 1
        cols = min(int(t["cx"]) + 111, int(t["newW"]) - 1) - max(int(t["cx"]) - 112, 0) + 1
        src_rows = min(int(t["H"]), int(np.ceil(max(rows, 1) * float(t["ry"]))) + 1)
        src_cols = min(int(t["W"]), int(np.ceil(max(cols, 1) * float(t["rx"]))) + 1)
        total += 224 * 224 * 16 + 19 * 12 + 4 * src_rows * src_cols
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the device only")
    params, mean = T.fixture_params()
    eng = hpe_amd.HpeEngine(device=0, max_batch=256)
    eng.load_smpl(synthetic.make_smpl_model())
    eng.load_regressor(params)
    eng.load_mean_theta(mean)
    eng.load_critic(synthetic.make_critic_params())
    eng.finalize()
    start = eng.regressor_params().clone()
    lib = _lib.load()
    rows = []
    for B in (8, 64, 256):
        sizes, frames, segs, kp, centers, draws = make_batch(B, seed=B)
        # the launch alone: frames packed once, table on the device, outputs preallocated
        area = sizes[:, 0].astype(np.int64) * sizes[:, 1]
        pad16 = lambda n: (n + 15) // 16 * 16  # noqa: E731
        foffs = np.concatenate([[0], np.cumsum(pad16(area * 3))[:-1]])
        soffs = np.concatenate([[0], np.cumsum(pad16(area))[:-1]])
        table = augment.plan_augmentation(sizes, centers, draws, frame_offsets=foffs, seg_offsets=soffs)
        fbuf = torch.zeros(int(pad16(area * 3).sum()), dtype=torch.uint8, device="cuda")
        sbuf = torch.zeros(int(pad16(area).sum()), dtype=torch.uint8, device="cuda")
        for f, s, fo, so in zip(frames, segs, foffs, soffs):
            fbuf[int(fo):int(fo) + f.numel()] = f.reshape(-1)
            sbuf[int(so):int(so) + s.numel()] = s.reshape(-1)
        tdev = torch.from_numpy(table.view(np.uint8)).cuda()
        out = (torch.empty((B, 224, 224, 3), device="cuda"), torch.empty((B, 224, 224), device="cuda"), torch.empty((B, 19, 3), device="cuda"))
        thost = table.ctypes.data_as(C.c_void_p)

        def launch():
            st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            _lib.check(lib.hpe_augment_batch(fbuf.data_ptr(), sbuf.data_ptr(), thost, tdev.data_ptr(), kp.data_ptr(), B, out[0].data_ptr(),
                                             out[1].data_ptr(), out[2].data_ptr(), st))

        launch()
        ref_img, ref_seg = torch_restatement(frames, segs, table)
        agree = {"images_max_abs_diff": float((out[0] - ref_img).abs().max()), "seg_max_abs_diff": float((out[1] - ref_seg).abs().max())}
        images, seg_gts, kp_gt = augment.augment_batch(frames, segs, kp, centers, draws=draws)
        assert torch.equal(images, out[0]) and torch.equal(seg_gts, out[1])
        feat = torch.from_numpy(T.make_features(B, seed=B)).cuda()
        drop = torch.from_numpy(T.make_drop(B, seed=B)).cuda()
        trainer = hpe_amd.GeneratorTrainer(eng, generator=torch.Generator(device="cuda").manual_seed(1))
        row = {"B": B}
        row.update(measure({"hip_launch_ms": launch, "hip_python_ms": lambda: augment.augment_batch(frames, segs, kp, centers, draws=draws),
                            "hip_python_out_ms": lambda: augment.augment_batch(frames, segs, kp, centers, draws=draws, out=out),
                            "torch_ms": lambda: torch_restatement(frames, segs, table),
                            "generator_step_ms": lambda: trainer.step(feat, kp_gt, seg_gts=seg_gts, drop=drop)}, args.iters, args.repeats))
        eng.set_regressor_params(start)
        nbytes = algorithmic_bytes(table)
        row["algorithmic_MB"] = round(nbytes / 1e6, 3)
        row["launch_GBps"] = round(nbytes / (row["hip_launch_ms"] * 1e-3) / 1e9, 1)
        row["share_of_copy_rate"] = round(row["launch_GBps"] / (COPY_TBS * 1e3), 4)
        row["ratio_hip_python_over_torch"] = round(row["hip_python_ms"] / row["torch_ms"], 4)
        row["share_of_generator_step"] = round(row["hip_python_ms"] / row["generator_step_ms"], 4)
        row.update(agree)
        rows.append(row)
    res = {"tool": "augment_bench", "device": torch.cuda.get_device_name(0), "iters": args.iters, "repeats": args.repeats,
           "copy_rate_TBps": COPY_TBS, "rows": rows}
    line = json.dumps(res)
    print(line)
    print("%5s %10s %10s %12s %10s %10s %9s %12s %10s" % ("B", "launch", "python", "python+out", "torch", "gen step", "GB/s", "hip / torch", "of step"))
    for r in rows:
        print("%5d %10.4f %10.4f %12.4f %10.4f %10.4f %9.1f %12.4f %10.4f" % (r["B"], r["hip_launch_ms"], r["hip_python_ms"], r["hip_python_out_ms"],
                                                                             r["torch_ms"], r["generator_step_ms"], r["launch_GBps"],
                                                                             r["ratio_hip_python_over_torch"], r["share_of_generator_step"]))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
