#!/usr/bin/env python3
"""bench.py -- images/sec of the per-image forward hot path (BASELINE.json metric) on N MI355X of one node.

    python bench.py --gpus N --steps K --warmup W

N > 1 without a launcher: this process starts N rank processes itself (one per GPU, RANK / LOCAL_RANK / WORLD_SIZE /
MASTER_* in their environment) BEFORE it touches HIP -- the parent never initialises the GPU and never exec()s -- relays
rank 0's single JSON line and exits non-zero if any rank fails.  Under torchrun
(`python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N`) the ranks are already there and nothing is spawned.
`HPE_FORCE_DIST=1 python bench.py --gpus 1` takes the same spawned path with a world of one (rehearses the RCCL calls).

One "step" = one pass of the whole path over one batch of 256 synthetic 224x224x3 images per GPU, already
resident in HBM: ResNet-50 v1 encoder (fp32 MFMA) -> 3 IEF regressor stages -> SMPL (LBS, joint regress,
orthographic reprojection) at ALL three stages (what Trainer.val_step evaluates; nothing is skipped) ->
for N > 1 one RCCL all-gather of the final theta [256,85] per rank over xGMI.  Images shard by batch
(independent units, no data-path collective besides that gather): weak scaling.  --config5 adds the two
reprojection losses of every stage (one library call) and, for N > 1, ONE all-reduce of the [3,4] block of
(kp numerator, kp count, -, mesh sum).

Rank 0 prints ONE JSON line.  The top level is the HEADLINE (fp32, batch 256 / GPU).  A plain run does only what the headline
needs: set-up, W warm-up steps, the K timed steps, `--dump-outputs DIR` if given, the line.  Everything described below beyond
`metric` / `value` / `ms_per_step` (roofline, sustained, cpu_baseline, parity, dist_check, the other configurations) is measured
only with `--full`.

    python bench.py --gpus 1 --steps K --warmup W --full

`--dump-outputs DIR` writes the arrays the last timed step handed its caller (dump_outputs); inputs and weights are seeded, so two
builds run with the same arguments can be compared output for output.

With --full at N == 1 the run then measures the other single-GPU configurations of BASELINE.json in short legs (10 steps, no sustain
loop) and reports them as sub-blocks of the same line -- `configs.fp32_b64` (configs[1] as written), `configs.bf16_b256` (configs[3]),
`configs.config5_b256` (configs[4], on the well-conditioned "bounded" synthetic regressor so that all three stages project
the mesh over the silhouette) -- plus `graph` (the step captured into hipGraphs: host microseconds per step before / after)
and `from_host` (uint8 frames in pinned host memory -> H2D on a copy stream -> batched preprocess kernel -> the path).

`roofline` is for the dominant kernel family, the 53 convolution layers (implicit-GEMM conv_gemm_f32_dma_kernel; the 3x3
layers run as fp32 Winograd, which does fewer multiplies for the same layer -- the algorithmic FLOPs priced here are the
direct convolution's): achieved = 7.7119 GFLOP/img * B / (MEAN encoder span over the timed steps: HIP
events recorded on the launch stream around every step's encoder; the batch-chunk streams overlap their conv launches, so
the span -- not a sum of overlapping durations -- is the family's time; spans of successive steps are disjoint, so
launch_ms <= ms_per_step), peak = 157.3 TFLOP/s fp32 MFMA.  `roofline.serial` is the same quantity with the chunk streams
off and events around each launch (one extra step after the timed region); it is the number the rocprofv3 kernel stats in
profiles/ add up to.  `sustained` repeats the step untimed for >= 10 s and reports its rate with sampled board power / clock.
`cpu_baseline` is the CPU oracle (a NumPy / torch-CPU restatement of the reference path -- TensorFlow is not
installable here) timed on this host's cores with BASELINE.md §3's protocol (B = 1 and B = 64,
2 warm-ups, median of 5), rank 0, N == 1 only.  The run FAILS (exit 3) if a gated parity block exceeds its bar.
"""
import argparse
import contextlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ENCODER_GFLOP_PER_IMG = 7.711850496  # 2 * 3,855,925,248 MAC (resnet_spec.encoder_macs_per_image)
PEAK_FP32_MFMA_TFLOPS = 157.3  # /opt/skills/guides/MI355X_MICROARCH.md: Peak FP32 (matrix)
PEAK_BF16_MFMA_TFLOPS = 2500.0  # dense bf16 MFMA (same guide)
PEAK_HBM_GBS = 8000.0
# v_mfma_f32_32x32x2_f32 evaluates 1024 (vertex, pixel) pairs in 64 cycles on one of the 1024 SIMDs at 2.4 GHz
PEAK_TPAIRS = 1024.0 / 64.0 * 1024 * 2.4e9 / 1e12
PARITY_BAR = 1e-4
BF16_BAR = 1e-2      # bf16 encoder: rel-L2 of the outputs against the fp32 oracle (tests/test_gpu_parity.py::test_bf16_encoder_variant)
LOSS_BAR = 2e-4      # reprojection losses against the oracle (near-tie flips of the nearest-neighbour search: <= 1.5e-4 of an exact search)


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256, help="images per GPU (BASELINE metric: 256)")
    ap.add_argument("--cpu-sample", type=int, default=64, help="batch of the cpu_baseline's large case (BASELINE.md §3: 64; 0 = skip)")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--sustain", type=float, default=10.0, help="seconds of the untimed steady-state loop after the timed steps (0 = skip)")
    ap.add_argument("--encoder-dtype", default="fp32", choices=["fp32", "bf16"], help="bf16 = BASELINE configs[3] (bf16 encoder, fp32 SMPL)")
    ap.add_argument("--config5", action="store_true", help="also evaluate kp + mesh reprojection losses of every stage (BASELINE configs[4])")
    ap.add_argument("--regressor", default=None, choices=["survey", "bounded"],
                    help="synthetic regressor variant (synthetic.make_regressor_params); default: survey, bounded with --config5")
    ap.add_argument("--no-pipeline", action="store_true", help="serial steps: the regressor + SMPL tail of batch k does NOT overlap the encoder of batch k+1")
    ap.add_argument("--graph", action="store_true", help="headline steps as captured hipGraphs (hpe_encoder || hpe_tail of the previous batch, one replay per step)")
    ap.add_argument("--from-host", action="store_true", help="headline steps start from uint8 frames in pinned host memory (H2D on a copy stream + batched preprocess kernel)")
    ap.add_argument("--parity-sample", type=int, default=0, help="with --cpu-sample 0: check this many images against the oracle once (no CPU timing protocol); "
                                                                 "what the per-configuration child runs of the default line use")
    ap.add_argument("--no-legs", action="store_true", help="headline only: skip the configs / graph / from_host sub-blocks of the default N == 1 run")
    ap.add_argument("--leg-steps", type=int, default=10)
    ap.add_argument("--full", action="store_true", help="also measure and check everything beyond the headline: roofline, sustained loop, "
                                                        "CPU baseline and oracle parity, dist_check, the other configurations (the options above "
                                                        "that select or skip those act only with --full)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write the outputs of the last timed step as DIR/<name>.npy (dump_outputs)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return args


# ------------------------------------------------------------------------------------------------- synthetic assets, once per node
def make_assets():
    from hpe_amd import synthetic

    return dict(smpl=synthetic.make_smpl_model(), enc=synthetic.make_encoder_params(), reg=synthetic.make_regressor_params(),
                reg_bounded=synthetic.make_regressor_params(variant="bounded"), mean=synthetic.make_mean_params())


def save_assets(a, path):
    import numpy as np

    flat = {}
    for grp, d in a.items():
        for k, v in d.items():
            flat[grp + "::" + k] = np.asarray(v)
    tmp = path + ".tmp%d.npz" % os.getpid()
    np.savez(tmp, **flat)
    os.replace(tmp, path)  # atomic: a reader sees either nothing or the whole file


def load_assets(path):
    import numpy as np

    out = {}
    with np.load(path, allow_pickle=False) as z:
        for key in z.files:
            grp, k = key.split("::", 1)
            out.setdefault(grp, {})[k] = z[key]
    return out


def get_assets(world, local_rank):
    """The 128 MB of seeded synthetic weights are generated ONCE per node: by the launching parent (HPE_BENCH_ASSETS), or under
    torchrun by local rank 0 (the others wait for the file), instead of by every rank at the same time."""
    path = os.environ.get("HPE_BENCH_ASSETS")
    if world == 1 and not path:
        return make_assets(), None
    made = None
    if not path:
        path = "/dev/shm/hpe_bench_assets_%s_%s.npz" % (os.environ.get("MASTER_PORT", "0"), os.environ.get("TORCHELASTIC_RUN_ID", "run"))
        if local_rank == 0 and not os.path.exists(path):
            save_assets(make_assets(), path)
            made = path
    t0 = time.time()
    while not os.path.exists(path):
        if time.time() - t0 > 600:
            raise SystemExit("bench.py: timed out waiting for %s" % path)
        time.sleep(0.1)
    return load_assets(path), made


# ------------------------------------------------------------------------------------------------- rank launcher
def _free_port():
    import socket

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def launch_ranks(n):
    """Start n fresh rank processes of this script (the parent has made no HIP call and makes none), relay rank 0's JSON
    line, exit with the first failing rank's code."""
    import subprocess
    import threading

    port = _free_port()
    assets_path = None
    if n > 1:
        assets_path = "/dev/shm/hpe_bench_assets_%d.npz" % os.getpid()
        save_assets(make_assets(), assets_path)  # NumPy only: no HIP in this process
    procs = []
    for r in range(n):
        env = dict(os.environ)
        env.update(RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        if assets_path:
            env["HPE_BENCH_ASSETS"] = assets_path
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=subprocess.PIPE if r == 0 else sys.stderr, stderr=sys.stderr))
    out0 = []
    reader = threading.Thread(target=lambda: out0.append(procs[0].stdout.read()), daemon=True)
    reader.start()
    rc = 0
    live = set(range(n))
    while live:
        for r in list(live):
            code = procs[r].poll()
            if code is None:
                continue
            live.discard(r)
            if code != 0 and rc == 0:
                rc = code
                print("bench.py: rank %d exited with code %d; stopping the other ranks" % (r, code), file=sys.stderr)
                for q in live:
                    procs[q].terminate()  # exact PIDs this process started
        time.sleep(0.05)
    reader.join(timeout=10)
    if assets_path and os.path.exists(assets_path):
        os.remove(assets_path)
    text = (out0[0] if out0 else b"").decode(errors="replace")
    lines = [ln for ln in text.splitlines() if ln.startswith("{")]
    if rc == 0 and len(lines) != 1:
        print("bench.py: expected one JSON line from rank 0, got %d" % len(lines), file=sys.stderr)
        rc = 1
    for ln in lines[:1]:
        print(ln, flush=True)
    sys.exit(rc)


# ------------------------------------------------------------------------------------------------- CPU / NUMA placement of a rank
def parse_cpulist(text):
    """'0-3,8,10-11' -> [0, 1, 2, 3, 8, 10, 11]"""
    cpus = []
    for part in text.strip().split(","):
        if not part:
            continue
        if "-" in part:
            a, b = part.split("-")
            cpus.extend(range(int(a), int(b) + 1))
        else:
            cpus.append(int(part))
    return cpus


def cpu_share(cpus, n_sharing, index):
    """The index-th of n_sharing contiguous, disjoint, near-equal parts of a sorted CPU list (the first len % n parts get one more)."""
    cpus = sorted(cpus)
    n_sharing = max(1, n_sharing)
    q, r = divmod(len(cpus), n_sharing)
    lo = index * q + min(index, r)
    return cpus[lo:lo + q + (1 if index < r else 0)]


def plan_rank_cpus(node_of_rank, node_cpus, local_rank):
    """CPUs of one local rank: the cores of its GPU's NUMA node, split between the local ranks whose GPUs sit on the same node --
    disjoint sets over the ranks of a host (8 ranks on a 128-core two-node host: 16 cores each).  node_of_rank[r] = NUMA node of local
    rank r's GPU (-1 / missing: unknown -> None: no pinning), node_cpus[node] = usable cores of that node."""
    node = node_of_rank[local_rank]
    if node is None or node < 0 or not node_cpus.get(node):
        return None
    sharing = [r for r, nd in enumerate(node_of_rank) if nd == node]
    part = cpu_share(node_cpus[node], len(sharing), sharing.index(local_rank))
    return part or None


def _gpu_numa_node(torch, idx):
    p = torch.cuda.get_device_properties(idx)
    bdf = "%04x:%02x:%02x.0" % (getattr(p, "pci_domain_id", 0), p.pci_bus_id, p.pci_device_id)
    with open("/sys/bus/pci/devices/%s/numa_node" % bdf) as f:
        return bdf, int(f.read().strip())


def pin_rank_to_gpu_numa(torch, local_rank, world):
    """Pin this rank to its share of the cores of its GPU's NUMA node (sysfs `numa_node` of the PCI device; the node's cores are split
    between the local ranks on that node, disjoint sets) and cap the CPU thread pools at that share.  Best effort: returns a
    description or None."""
    try:
        bdf, node = _gpu_numa_node(torch, local_rank)
        if node < 0:
            return None
        n_local = min(world, torch.cuda.device_count())
        node_of_rank = []
        for r in range(n_local):
            try:
                node_of_rank.append(_gpu_numa_node(torch, r)[1])
            except Exception:  # noqa: BLE001
                node_of_rank.append(-1)
        with open("/sys/devices/system/node/node%d/cpulist" % node) as f:
            usable = sorted(set(parse_cpulist(f.read())) & set(os.sched_getaffinity(0)))
        cpus = plan_rank_cpus(node_of_rank, {node: usable}, local_rank) if local_rank < n_local else None
        if not cpus:
            return None
        os.sched_setaffinity(0, cpus)
        nthreads = max(1, len(cpus))
        torch.set_num_threads(nthreads)
        return {"pci": bdf, "numa_node": node, "cpus": len(cpus), "first_cpu": cpus[0], "torch_threads": nthreads}
    except Exception as e:  # noqa: BLE001 -- placement is an optimisation, never a reason to fail the run
        print("bench.py: NUMA pinning skipped (%s)" % e, file=sys.stderr)
        return None


# ------------------------------------------------------------------------------------------------- N > 1: the line verifies itself
def reduce_dist_check(torch, dist, world, gather_ok, parity_pass, worst_gated, device):
    """Every rank contributes (its gathered slice equals its own theta, its parity block passed, its worst gated error); ONE MIN
    all-reduce makes the verdict identical on every rank, so that every rank exits 3 when any rank failed (tests/test_distributed_gloo.py
    runs this over gloo with 8 ranks and one of them forced to fail)."""
    flags = torch.tensor([1.0 if gather_ok else 0.0, 1.0 if parity_pass else 0.0, -float(worst_gated)], dtype=torch.float64, device=device)
    dist.all_reduce(flags, op=dist.ReduceOp.MIN)
    return {"ranks": world, "gather_slice_equals_local_theta_on_every_rank": bool(flags[0].item() > 0.5),
            "parity_pass_on_every_rank": bool(flags[1].item() > 0.5), "worst_gated_over_ranks": float(-flags[2].item())}


def dist_check_failed(dist_check):
    return not (dist_check["gather_slice_equals_local_theta_on_every_rank"] and dist_check["parity_pass_on_every_rank"])


# ------------------------------------------------------------------------------------------------- power / clock sampling
class PowerSampler(object):
    """Samples board power (W) and shader clock (MHz) of the busiest GPU from sysfs hwmon in a side thread
    (rocm-smi as the fallback); no GPU call is made from the thread."""

    def __init__(self, period=0.5):
        import glob
        import threading

        self.period = period
        self.samples = []
        self._stop = False
        self._hw = sorted(glob.glob("/sys/class/drm/card*/device/hwmon/hwmon*"))
        self._t = threading.Thread(target=self._run, daemon=True)

    @staticmethod
    def _read(path):
        try:
            with open(path) as f:
                return float(f.read().strip())
        except Exception:
            return None

    def _sysfs(self):
        best = None
        for h in self._hw:
            p = self._read(os.path.join(h, "power1_average"))
            if p is None:
                p = self._read(os.path.join(h, "power1_input"))
            if p is None:
                continue
            f = self._read(os.path.join(h, "freq1_input"))
            cand = (p / 1e6, None if f is None else f / 1e6)
            if best is None or cand[0] > best[0]:
                best = cand
        return best

    @staticmethod
    def _smi():
        import re
        import subprocess

        try:
            o = subprocess.run(["rocm-smi", "--showpower", "--showclocks"], capture_output=True, text=True, timeout=10).stdout
        except Exception:
            return None
        pw = [float(m.group(1)) for m in re.finditer(r"Package Power[^:]*:\s*([0-9.]+)", o)]
        ck = [float(m.group(1)) for m in re.finditer(r"sclk clock level:[^(]*\(([0-9.]+)Mhz\)", o)]
        if not pw:
            return None
        i = max(range(len(pw)), key=lambda k: pw[k])
        return (pw[i], ck[i] if i < len(ck) else None)

    def _run(self):
        use_smi = self._sysfs() is None
        while not self._stop:
            s = self._smi() if use_smi else self._sysfs()
            if s is not None:
                self.samples.append((time.perf_counter(),) + s)
            time.sleep(self.period if not use_smi else max(self.period, 1.0))

    def start(self):
        self._t.start()

    def stop(self):
        self._stop = True
        self._t.join(timeout=15)

    def summary(self, skip_s=2.0):
        if not self.samples:
            return None, None, 0
        t0 = self.samples[0][0]
        use = [s for s in self.samples if s[0] - t0 >= skip_s] or self.samples
        pw = [s[1] for s in use]
        ck = [s[2] for s in use if s[2] is not None]
        return (round(sum(pw) / len(pw), 1), round(sum(ck) / len(ck), 1) if ck else None, len(use))


# ------------------------------------------------------------------------------------------------- one measured configuration
class Leg(object):
    """One configuration of the path on this rank: a Predictor (its own hpe_ctx), resident inputs, the step function and the
    fence that closes a timed region.  mode: 'pipelined' (hpe_forward_pipelined, the default), 'serial' (hpe_forward),
    'overlap' / 'graph' (hpe_encoder || hpe_tail of the previous batch in one stream-ordered step, eager / captured)."""

    def __init__(self, env, B, dtype="fp32", reg_variant="survey", config5=False, mode="pipelined", from_host=False, use_dist=False,
                 images=None, pred=None):
        torch, hpe_amd = env["torch"], env["hpe_amd"]
        self.env, self.B, self.dtype, self.config5, self.mode, self.use_dist, self.from_host = env, B, dtype, config5, mode, use_dist, from_host
        self.reg_variant = reg_variant
        a = env["assets"]
        self.reg = a["reg_bounded" if reg_variant == "bounded" else "reg"]
        if pred is None:
            class Cfg(object):
                img_size, num_stage, batch_size, data_format = 224, 3, B, "NHWC"
                checkpoint_dir = smpl_model_path = None
                encoder_dtype = dtype

            pred = hpe_amd.Predictor(Cfg(), smpl_model=a["smpl"], mean_params=a["mean"], encoder_params=a["enc"], regressor_params=self.reg,
                                     device=env["local_rank"])
        self.pred, self.eng = pred, pred.engine
        eng = self.eng
        self.images = images if images is not None else torch.from_numpy(hpe_amd.synthetic.make_images(B, seed=1000 + env["rank"])).cuda()
        self.want = eng.DEFAULT_OUTPUTS + (("verts2d",) if config5 else ())
        self.losses = {}
        self.step_no = 0
        self.pending = [None, None]
        self.host_s = 0.0  # host time spent inside step() calls of the last timed region
        world = env["world"]
        self.theta_all = [torch.empty((world * B, 85), dtype=torch.float32, device="cuda") for _ in range(2)] if use_dist else None
        if config5:
            seg_np, kp_np = hpe_amd.synthetic.make_lsp_targets(B, seed=2000 + env["rank"])
            self.seg_np, self.kp_np = seg_np, kp_np
            self.seg_gts = torch.from_numpy(seg_np[..., 0].copy()).cuda()
            self.kp_gts = torch.from_numpy(kp_np).cuda()
            self.loss_out = [torch.zeros((3, 4), dtype=torch.float32, device="cuda") for _ in range(2)]
        if mode in ("overlap", "graph"):
            eng.join()
            torch.cuda.synchronize()
            self.stepper = eng.make_overlapped_plan(B, all_stages=True, want=self.want, graph=(mode == "graph"),
                                                    tail_extra=self._losses_of if config5 else None)
            self.sets = self.stepper.sets
            self.tail = None
        else:
            # two output sets used alternately: the all-gather of step k reads theta_k while step k+1 already writes theta_{k+1}
            pipe = mode == "pipelined"
            self.plans = [eng.make_forward_plan(B, all_stages=True, want=self.want, pipelined=pipe) for _ in range(2)]
            self.sets = [p[1] for p in self.plans]
            self.tail = eng.tail_stream() if pipe else None
        self.pipe_on = True  # cleared for the per-launch-timed step (hpe_forward_pipelined then runs serially on the caller's stream)
        if from_host:
            import numpy as np

            # uint8 frames in pinned host memory (what a capture / decode thread hands over), two device staging buffers, a copy stream
            u8 = np.clip(np.rint((self.images.cpu().numpy().astype(np.float64) + 1.0) * 127.5), 0, 255).astype(np.uint8)
            self.frames_host = torch.from_numpy(u8).pin_memory()
            self.frames_dev = [torch.empty_like(self.frames_host, device="cuda") for _ in range(2)]
            self.img_dev = [torch.empty((B, 224, 224, 3), dtype=torch.float32, device="cuda") for _ in range(2)]
            self.copy_stream = torch.cuda.Stream()
            self.ev_copied = [torch.cuda.Event() for _ in range(2)]
            self.ev_consumed = [None, None]

    # consumers of a batch's outputs run on the tail stream in pipelined mode (hpe_tail_stream), on the current stream otherwise
    def _on_tail(self):
        torch = self.env["torch"]
        return torch.cuda.stream(self.tail) if (self.tail is not None and self.pipe_on) else contextlib.nullcontext()

    def _losses_of(self, outs, k):
        # one library call for the 2 x 3 losses, then (N > 1) ONE all-reduce of the [3,4] block
        packed = self.eng.val_losses(self.kp_gts, [st["kp2d"] for st in outs], self.seg_gts, [st["verts2d"] for st in outs], out=self.loss_out[k])
        self.losses["packed_local"] = packed
        return packed

    def _stage_inputs(self, k):
        """--from-host: frames (pinned) -> device staging k on the copy stream, then the batched preprocess kernel on the compute stream"""
        torch, hpe_amd = self.env["torch"], self.env["hpe_amd"]
        cur = torch.cuda.current_stream()
        if self.ev_consumed[k] is not None:
            self.copy_stream.wait_event(self.ev_consumed[k])  # the preprocess kernel of two steps ago has read this staging buffer
        with torch.cuda.stream(self.copy_stream):
            self.frames_dev[k].copy_(self.frames_host, non_blocking=True)
            self.ev_copied[k].record(self.copy_stream)
        cur.wait_event(self.ev_copied[k])
        hpe_amd.preprocess_batch(self.frames_dev[k], out=self.img_dev[k])
        ev = torch.cuda.Event()
        ev.record(cur)
        self.ev_consumed[k] = ev
        return self.img_dev[k]

    def step(self):
        t_in = time.perf_counter()
        D, dist = self.env["D"], self.env["dist"]
        k = self.step_no & 1
        self.step_no += 1
        x = self._stage_inputs(k) if self.from_host else self.images
        if self.mode in ("overlap", "graph"):
            prev = self.stepper(x)  # outputs of the PREVIOUS batch (losses already enqueued on its tail branch)
            if prev is not None and self.use_dist:
                self._collectives(prev, self.stepper.last)
            self.host_s += time.perf_counter() - t_in
            return prev
        if self.use_dist and self.pending[k] is not None:
            with self._on_tail():
                self.pending[k].wait()  # the gather that last used this output set (two steps ago), before the tail overwrites it
            self.pending[k] = None
        o = self.plans[k][0](x)
        with self._on_tail():
            if self.config5:
                self._losses_of(o, k)
            if self.use_dist:
                self._collectives(o, k)
        self.host_s += time.perf_counter() - t_in
        return o

    def _collectives(self, outs, k):
        D, dist = self.env["D"], self.env["dist"]
        if self.config5:
            self.losses["packed"] = D.reduce_losses(self.loss_out[k])
        # the ONE data-path collective: all-gather of the predicted theta over RCCL, asynchronous so that it overlaps the next
        # batch's encoder (it is waited for before its buffers are reused and before the timed region ends)
        if self.pending[k] is not None:
            self.pending[k].wait()
        self.pending[k] = dist.all_gather_into_tensor(self.theta_all[k], outs[-1]["theta"], async_op=True)

    def fence(self):
        """Everything enqueued so far has completed on every rank when this returns (tails, collectives, the last flush)."""
        torch, dist = self.env["torch"], self.env["dist"]
        if self.mode in ("overlap", "graph"):
            last = self.stepper.flush()
            if last is not None and self.use_dist:
                self._collectives(last, self.stepper.last)
        for k in range(2):
            if self.use_dist and self.pending[k] is not None:
                self.pending[k].wait()
                self.pending[k] = None
        torch.cuda.synchronize()
        if self.use_dist:
            dist.barrier()
            torch.cuda.synchronize()

    def _last_index(self):
        return self.stepper.last if self.mode in ("overlap", "graph") else (self.step_no - 1) & 1

    def last_outputs(self):
        return self.sets[self._last_index()]

    def last_losses(self):
        if "packed" in self.losses:
            return self.losses["packed"]
        return self.loss_out[self._last_index()]

    def run_timed(self, steps, warmup, timing=True):
        """W untimed warm-up steps, then exactly K steps bracketed by a barrier + synchronize on both sides; MAX over ranks."""
        torch, dist = self.env["torch"], self.env["dist"]
        for _ in range(warmup):
            self.step()
        self.fence()
        if timing and self.mode != "graph":
            self.eng.enable_timing(1)
        self.host_s = 0.0
        t0 = time.perf_counter()
        for _ in range(steps):
            self.step()
        self.fence()
        dt = time.perf_counter() - t0
        if self.use_dist:
            t = torch.tensor([dt], dtype=torch.float64, device="cuda")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t.item())
        return dt

    def close(self):
        self.eng.close()


def encoder_roofline(leg, dt_ms_per_step, serial_pass=True):
    """roofline block of the conv kernel family from the events of the timed region just closed (hpe_get_span_stats)."""
    env, eng, B = leg.env, leg.eng, leg.B
    hpe_amd = env["hpe_amd"]
    sp = eng.span_stats()
    tm = eng.timings()
    span_ms = sp["mean_ms"]
    achieved = ENCODER_GFLOP_PER_IMG * B / span_ms  # GFLOP/ms == TFLOP/s
    PEAK = PEAK_FP32_MFMA_TFLOPS if leg.dtype == "fp32" else PEAK_BF16_MFMA_TFLOPS
    roof = {
        "bound": "mfma",
        "kernel": eng.encoder_kernel_description() + "; batch chunks on %s concurrent streams" % os.environ.get("HPE_STREAMS", "2"),
        "achieved": round(achieved, 3), "peak": PEAK, "unit": "TFLOP/s", "frac": round(achieved / PEAK, 4), "traffic": None,
        "launch_ms": round(span_ms, 4),
        "launch_ms_def": "mean encoder span over the %d timed steps (min %.4f, max %.4f); spans of successive steps are disjoint" % (
            sp["calls"], sp["min_ms"], sp["max_ms"]),
        "flop_per_launch": ENCODER_GFLOP_PER_IMG * B * 1e9,
    }
    phase = {"encoder_ms": round(span_ms, 3), "regress_smpl_ms": round(tm["regress_smpl_ms"], 3)}
    per_conv = None
    if serial_pass:
        # serial cross-check, one extra step after the timed region: chunk streams off, events around each of the 53 launches;
        # the sum matches the rocprofv3 --kernel-trace --stats durations (profiles/)
        eng.enable_timing(2)
        leg.fence()
        leg.pipe_on = False
        leg.step()
        leg.fence()
        leg.pipe_on = True
        ts = eng.timings()
        per_conv = eng.conv_timings()
        serial_tf = ENCODER_GFLOP_PER_IMG * B / ts["conv_ms"]
        roof["serial"] = {"sum_of_53_launch_ms": round(ts["conv_ms"], 4), "achieved": round(serial_tf, 3), "frac": round(serial_tf / PEAK, 4)}
        phase["step_ms_serial_events"] = round(ts["total_ms"], 3)
    if leg.dtype == "bf16":
        # at 16x the fp32 matrix rate the bf16 encoder is HBM bound: price it in algorithmic bytes
        nbytes = hpe_amd.resnet_spec.encoder_min_bytes_per_image(2) * B
        gbs = nbytes / span_ms / 1e6
        roof.update({"bound": "hbm", "achieved": round(gbs, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": round(gbs / PEAK_HBM_GBS, 4),
                     "bytes_per_launch": nbytes, "mfma_tflops": round(achieved, 1)})
        roof.pop("flop_per_launch")
        if "serial" in roof:
            roof["serial"] = {"sum_of_53_launch_ms": roof["serial"]["sum_of_53_launch_ms"],
                              "achieved": round(nbytes / roof["serial"]["sum_of_53_launch_ms"] / 1e6, 1)}
            roof["serial"]["frac"] = round(roof["serial"]["achieved"] / PEAK_HBM_GBS, 4)
    # HBM bytes per launch from the committed PMC passes (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE cannot run inside the timed
    # region); scaled by batch, null if no measurement of this build + dtype is committed
    import glob

    cands = sorted(glob.glob(os.path.join(ROOT, "profiles", "*", "*conv_hbm_traffic_%s.json" % leg.dtype)))
    if cands:
        tj = json.load(open(cands[-1]))
        roof["traffic"] = round(tj["total_bytes"] * B / tj["batch"])
        roof["traffic_source"] = os.path.relpath(cands[-1], ROOT)
    eng.enable_timing(0)
    roof["launch_ms_le_ms_per_step"] = bool(span_ms <= dt_ms_per_step * 1.005)
    if not roof["launch_ms_le_ms_per_step"]:
        print("bench.py: WARNING mean encoder span %.4f ms above the step time %.4f ms" % (span_ms, dt_ms_per_step), file=sys.stderr)
    return roof, phase, per_conv


def loss_roofline_block(leg):
    """The pixel -> nearest-vertex search of the mesh loss (the dominant loss kernel): pairs ACTUALLY evaluated on the matrix cores
    (the kernels' own MFMA counters, one counted step) over the search time of an exclusive step, against 39.3 Tpair/s."""
    torch = leg.env["torch"]
    eng, B = leg.eng, leg.B
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    eng.enable_timing(2)  # level 2: the step runs serially on the caller's stream (no tail stream, no chunk streams)
    leg.fence()
    eng.set_loss_counter(cnt)
    leg.pipe_on = False  # exclusive: nothing else shares the GPU with the searches of this step
    leg.step()
    leg.fence()
    leg.pipe_on = True
    eng.set_loss_counter(None)
    lt = eng.loss_timings()
    eng.enable_timing(0)
    mf = cnt.cpu().numpy()
    evaluated = float(mf.sum()) * 1024.0
    n_sil = int((leg.seg_gts > 0).sum().item())
    full_pairs = float(n_sil) * 6890.0 * 3.0  # what an exhaustive search of the 3 stages evaluates (the reference's P x 6890 matrix)
    a2b_ms = lt["a2b_search_ms"]
    return {
        "kernel": "pixel -> nearest vertex x 3 stages: nn_a2b_grid_kernel (cell grid over the mesh, candidates as one K=2 fp32 MFMA per 32 "
                  "vertices x 32 pixels) + nn_a2b_mfma_kernel (full search) for images whose mesh is concentrated in < 40 cells",
        "bound": "mfma", "achieved": round(evaluated / a2b_ms / 1e9, 3), "peak": round(PEAK_TPAIRS, 3), "unit": "Tpair/s",
        "frac": round(evaluated / a2b_ms / 1e9 / PEAK_TPAIRS, 4), "launch_ms": round(a2b_ms / 3.0, 4),
        "pairs_evaluated_per_launch": evaluated / 3.0, "mfma_grid_search": int(mf[0]), "mfma_full_search": int(mf[1]),
        "full_search_pairs_per_launch": full_pairs / 3.0, "pruned_to": round(evaluated / full_pairs, 4),
        "full_search_equivalent_tpairs": round(full_pairs / a2b_ms / 1e9, 3),
        "val_losses_ms_per_step": round(lt["val_losses_ms"], 4),
        "note": "achieved / frac = pairs the matrix cores actually evaluated (MFMA counters of the two kernels, 1024 pairs each) over the "
                "search time of one exclusive step -- cannot exceed 1; full_search_equivalent_tpairs prices the pairs of an exhaustive search "
                "over the same time (an equivalent rate, not a utilisation)",
    }


def _rel(a, b):  # global-max normalisation (the north star's "1e-4 relative")
    import numpy as np

    return float(np.abs(a - b).max() / np.abs(b).max())


def _rel_rms(a, b):  # the tensor's own scale: max error over its RMS (small-magnitude outputs are not hidden)
    import numpy as np

    return float(np.abs(a - b).max() / (np.sqrt(np.mean(np.square(b.astype(np.float64)))) + 1e-30))


_KP2D_COND = {}


def kp2d_conditioning(O, images_np, assets, reg, ref, n=8):
    """Conditioning term of the own-scale kp2d error on the SURVEY regressor: the distance of the fp32 oracle from its own fp64 evaluation,
    rel_rms(kp2d_oracle32, kp2d_oracle64), on the first n images (kp2d = s (x + t) with the camera scale cancelled to s ~ -0.03 amplifies
    every rounding of theta; tests/test_gpu_parity.py::test_full_path_matches_oracle uses the same rule).  Cached per regressor."""
    import numpy as np

    key = id(reg)
    if key not in _KP2D_COND:
        n = min(n, images_np.shape[0], ref["generated_kp2d"].shape[0])
        r64 = O.predict(images_np[:n].astype(np.float64), assets["enc"], reg, O.SMPL(assets["smpl"], dtype=np.float64),
                        O.load_mean_param(assets["mean"], dtype=np.float64), dtype=np.float64)
        _KP2D_COND[key] = _rel_rms(ref["generated_kp2d"][:n], r64["generated_kp2d"])
    return _KP2D_COND[key]


def parity_block(outs_last, ref, n, dtype="fp32", gate_kp2d_rms=False, kp2d_cond=None):
    """Last-stage outputs of the first n images of a batch against the oracle's result dict `ref` (same images / weights).
    kp2d own-scale error: fixed 1e-4 bar on the bounded regressor (gate_kp2d_rms); on the survey regressor the bar is
    max(1e-4, 4 x kp2d_cond) with kp2d_cond = the oracle's own fp32-vs-fp64 distance (kp2d_conditioning) -- nothing printed is ungated."""
    import numpy as np

    j = outs_last["joints"][:n].cpu().numpy()
    v = outs_last["verts"][:n].cpu().numpy()
    par = {
        # "MPJPE vs ref" of BASELINE.json: mean Euclidean distance to the oracle's joints, same inputs and weights, on images taken
        # out of the full-size batch (so the Winograd / chunked paths are what is checked)
        "mpjpe_vs_oracle": float(np.linalg.norm(j - ref["generated_joints"][:n], axis=-1).mean()),
        "verts_rel_err": _rel(v, ref["generated_verts"][:n]),
        "joints_rel_err": _rel(j, ref["generated_joints"][:n]),
        "images_checked": n,
    }
    for key, rk in (("J_transformed", "J_transformed"), ("theta", "theta"), ("kp2d", "generated_kp2d"), ("cams", "generated_cams")):
        if key in outs_last:
            a = outs_last[key][:n].cpu().numpy()
            par["%s_rel_err" % key] = _rel(a, ref[rk][:n])
            par["%s_rel_rms" % key] = _rel_rms(a, ref[rk][:n])
    if "J_transformed" in outs_last:
        par["mpjpe24_vs_oracle"] = float(np.linalg.norm(outs_last["J_transformed"][:n].cpu().numpy() - ref["J_transformed"][:n], axis=-1).mean())
    if dtype == "fp32":
        gated = [k for k in par if k.endswith("_rel_err")] + ["cams_rel_rms", "theta_rel_rms"] + (["kp2d_rel_rms"] if gate_kp2d_rms else [])
        par["bar"] = "1e-4 relative fp32: *_rel_err = max|d| / max|ref| (the north star's bar) and the own-scale errors *_rel_rms = max|d| / RMS(ref) of cams, theta" + (
            " and kp2d (well-conditioned regressor variant: fixed bar)" if gate_kp2d_rms else
            "; kp2d_rel_rms is reported, not gated, on the survey regressor (its camera scale cancels to s ~ -0.03: kp2d = s (x + t) is ill-conditioned there)")
        par["worst_gated"] = max(par[k] for k in gated)
        par["pass"] = bool(par["worst_gated"] <= PARITY_BAR)
        if not gate_kp2d_rms and kp2d_cond is not None and "kp2d_rel_rms" in par:
            par["kp2d_conditioning"] = kp2d_cond
            par["kp2d_bar"] = max(PARITY_BAR, 4.0 * kp2d_cond)
            par["bar"] = par["bar"].replace("kp2d_rel_rms is reported, not gated, on the survey regressor",
                                            "kp2d_rel_rms on the survey regressor is gated at kp2d_bar = max(1e-4, 4 x kp2d_conditioning), the oracle's own fp32-vs-fp64 distance")
            par["pass"] = bool(par["pass"] and par["kp2d_rel_rms"] <= par["kp2d_bar"])
    else:
        l2 = float(np.linalg.norm(v.astype(np.float64) - ref["generated_verts"][:n]) / np.linalg.norm(ref["generated_verts"][:n]))
        par["verts_rel_l2"] = l2
        par["bar"] = "bf16 encoder (BASELINE configs[3]): rel-L2 of the vertices against the fp32 oracle <= 1e-2 (the 1e-4 bar is for fp32)"
        par["worst_gated"] = l2
        par["pass"] = bool(l2 <= BF16_BAR)
    return par


def loss_parity_block(lg, O, ref5, n5):
    """Both reprojection losses of the three stages for the first n5 images (a sub-batch call on the outputs of the last step) against
    the oracle's val_step (src/trainer.py:274-296 restated in oracle/hmr_oracle.py)."""
    o = lg.last_outputs()
    sub = lg.eng.val_losses(lg.kp_gts[:n5].contiguous(), [st["kp2d"][:n5].contiguous() for st in o], lg.seg_gts[:n5].contiguous(),
                            [st["verts2d"][:n5].contiguous() for st in o]).cpu().numpy()
    lo = O.val_losses(ref5["stage_verts"], ref5["stage_cams"], ref5["stage_kp2d"], lg.seg_np[:n5], lg.kp_np[:n5])
    errs = []
    for i in range(3):
        errs.append(abs(60.0 * sub[i, 2] - lo["kpr_losses"][i]) / abs(lo["kpr_losses"][i]))
        errs.append(abs(0.001 * sub[i, 3] - lo["mr_losses"][i]) / abs(lo["mr_losses"][i]))
    return {"images_checked": n5, "kpr_oracle": [float(x) for x in lo["kpr_losses"]], "mr_oracle": [float(x) for x in lo["mr_losses"]],
            "worst_rel_err": float(max(errs)), "bar": LOSS_BAR, "pass": bool(max(errs) <= LOSS_BAR)}


DUMP_MAX_BYTES = 64 * 10 ** 6


def dump_outputs(leg, out_dir):
    """--dump-outputs: what the last timed step handed its caller, as float32 .npy files in out_dir: stage<s>_<name> for the outputs of
    the three IEF stages (s = 1..3), `losses` (config 5: the [3,4] loss block) and `theta_gathered` (N > 1: the all-gathered theta).
    Written on rank 0 after the timed region.  If the files would exceed DUMP_MAX_BYTES (batch 256 does, narrowly: the vertices are
    21 MB per stage), every stage array keeps the same fixed, seeded sample of images, in batch order."""
    import numpy as np

    extra = {}
    if leg.config5:
        extra["losses"] = leg.last_losses().cpu().numpy()
    if leg.use_dist:
        extra["theta_gathered"] = leg.theta_all[leg._last_index()].cpu().numpy()
    arrays = {}
    for s, st in enumerate(leg.last_outputs()):
        for name, t in st.items():
            arrays["stage%d_%s" % (s + 1, name)] = t.cpu().numpy()
    budget = DUMP_MAX_BYTES - sum(a.nbytes for a in extra.values())
    total = sum(a.nbytes for a in arrays.values())
    if total > budget:
        n = leg.B * budget // total
        rows = np.sort(np.random.default_rng(0).choice(leg.B, n, replace=False))
        arrays = {k: a[rows] for k, a in arrays.items()}
    arrays.update(extra)
    os.makedirs(out_dir, exist_ok=True)
    for k, a in arrays.items():
        np.save(os.path.join(out_dir, k + ".npy"), np.ascontiguousarray(a, dtype=np.float64 if a.dtype == np.float64 else np.float32))
    return sorted(arrays)


# ------------------------------------------------------------------------------------------------- the benchmark (one rank)
def main():
    args = parse_args()
    force_dist = bool(os.environ.get("HPE_FORCE_DIST"))
    if "RANK" not in os.environ and "WORLD_SIZE" not in os.environ and (args.gpus > 1 or force_dist):
        launch_ranks(args.gpus)  # does not return

    # The encoder runs its batch chunks on 2 HIP streams, the regressor + SMPL tail on a third and RCCL adds its own; the HIP runtime
    # multiplexes all streams of a process onto GPU_MAX_HW_QUEUES (default 4) hardware queues, and once two busy streams share a
    # queue their overlap is lost (round 1: 20.1 -> 18.4 ms/step with a process group alive).  Must be set before HIP initialises.
    try:
        if int(os.environ.get("GPU_MAX_HW_QUEUES", "0")) < 8:
            os.environ["GPU_MAX_HW_QUEUES"] = "8"
    except ValueError:
        os.environ["GPU_MAX_HW_QUEUES"] = "8"

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("WORLD_SIZE=%d does not match --gpus %d" % (world, args.gpus))

    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)  # see the print at the end

    import numpy as np
    import torch

    import hpe_amd
    from hpe_amd import distributed as D

    torch.cuda.set_device(local_rank)
    placement = None
    if world > 1 or force_dist:
        # N ranks share one host: cap the CPU thread pools (oracle check, weight packing) at this rank's share of the cores, then
        # narrow the rank to the cores of its GPU's NUMA node where sysfs tells
        torch.set_num_threads(max(1, (os.cpu_count() or 1) // world))
        placement = pin_rank_to_gpu_numa(torch, local_rank, world)
    dist = None
    use_dist = world > 1 or force_dist  # HPE_FORCE_DIST: rehearse the RCCL calls at world 1
    if use_dist:
        import torch.distributed as dist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))

    assets, made_assets = get_assets(world, local_rank)
    env = dict(torch=torch, hpe_amd=hpe_amd, D=D, dist=dist, assets=assets, world=world, rank=rank, local_rank=local_rank)
    B = args.batch
    reg_variant = args.regressor or ("bounded" if args.config5 else "survey")
    mode = "graph" if args.graph else ("serial" if args.no_pipeline else "pipelined")
    leg = Leg(env, B, dtype=args.encoder_dtype, reg_variant=reg_variant, config5=args.config5, mode=mode, from_host=args.from_host,
              use_dist=use_dist)
    eng, images = leg.eng, leg.images

    # one-time initialisation that is not a benchmark step: code-object load / first-launch setup of every kernel and the RCCL
    # communicator (both are lazy); the W warm-up steps and the K timed steps follow
    eng.forward(images[:2], all_stages=True)
    if use_dist:
        dist.all_gather_into_tensor(leg.theta_all[0], leg.sets[0][-1]["theta"])
        dist.barrier()
    torch.cuda.synchronize()
    if made_assets and os.path.exists(made_assets):
        os.remove(made_assets)  # every rank has loaded it (barrier above)

    dt = leg.run_timed(args.steps, args.warmup, timing=args.full and not args.no_roofline)
    ms_per_step = dt / args.steps * 1e3
    host_us = leg.host_s / args.steps * 1e6
    if args.dump_outputs and rank == 0:
        dump_outputs(leg, args.dump_outputs)

    roofline = loss_roofline = phase = None
    if args.full and not args.no_roofline and mode != "graph":
        roofline, phase, per_conv = encoder_roofline(leg, ms_per_step)
        if args.config5:
            loss_roofline = loss_roofline_block(leg)
        if rank == 0 and os.environ.get("HPE_BENCH_LAYERS"):
            specs = list(hpe_amd.resnet_spec.CONV_SPECS)
            flops = {s.name: 2.0 * s.kh * s.kw * s.cin * s.cout * s.hout * s.hout * B for s in specs}
            for s, ms in zip(specs, per_conv):
                fl, note = flops[s.name], ""
                # conv_block: the projection shortcut runs inside branch2c's launch (dual-source GEMM) and has no launch of its own
                short = s.name.replace("branch2c", "branch1")
                dual = os.environ.get("HPE_DUAL", "1") != "0" and s.name.endswith("a_branch2c") and short in flops
                if dual:
                    fl, note = fl + flops[short], "  (+ %s in the same launch)" % short
                if s.name.endswith("branch1") and os.environ.get("HPE_DUAL", "1") != "0":
                    print("%-18s %8.3f ms        -     (inside %s)" % (s.name, ms, s.name.replace("branch1", "branch2c")), file=sys.stderr)
                    continue
                print("%-18s %8.3f ms %7.1f TF%s" % (s.name, ms, fl / ms / 1e9, note), file=sys.stderr)

    # ---- steady state: the same step, untimed by the driver, for >= args.sustain seconds with power / clock sampled
    sustained = None
    if args.full and args.sustain > 0:
        sampler = PowerSampler() if rank == 0 else None
        leg.fence()
        if sampler:
            sampler.start()
        n_sus = 0
        t_s = time.perf_counter()
        while True:
            for _ in range(20):
                leg.step()
            n_sus += 20
            torch.cuda.synchronize()
            flag = torch.tensor([1.0 if time.perf_counter() - t_s >= args.sustain else 0.0], device="cuda")
            if use_dist:
                dist.all_reduce(flag, op=dist.ReduceOp.MAX)  # all ranks leave the loop together
            if float(flag.item()) > 0:
                break
        leg.fence()
        dt_s = time.perf_counter() - t_s
        if sampler:
            sampler.stop()
            pw, ck, ns = sampler.summary()
            sustained = {"ms_per_step": round(dt_s / n_sus * 1e3, 4), "steps": n_sus, "seconds": round(dt_s, 2),
                         "images_per_sec": round(world * B * n_sus / dt_s, 2), "avg_power_w": pw, "sclk_mhz": ck, "samples": ns}
            trace = os.environ.get("HPE_POWER_TRACE")
            if trace:
                with open(trace, "w") as f:
                    f.write("t_s,power_w,sclk_mhz\n")
                    for ts_, p_, c_ in sampler.samples:
                        f.write("%.2f,%.1f,%s\n" % (ts_ - sampler.samples[0][0], p_, "" if c_ is None else "%.0f" % c_))

    # ---- N > 1 (and the HPE_FORCE_DIST rehearsal): every rank verifies itself, the flags are reduced into the one line
    dist_check = None
    if args.full and use_dist:
        from oracle import hmr_oracle as O  # the checker

        last = leg._last_index()
        mine = leg.last_outputs()[-1]["theta"]
        gather_ok = bool(torch.equal(leg.theta_all[last][rank * B:(rank + 1) * B], mine))
        n_chk = min(2, B)
        osmpl = O.SMPL(assets["smpl"])
        mean = O.load_mean_param(assets["mean"])
        ref2 = O.predict(images[:n_chk].cpu().numpy(), assets["enc"], leg.reg, osmpl, mean)
        p2 = parity_block(leg.last_outputs()[-1], ref2, n_chk, dtype=args.encoder_dtype, gate_kp2d_rms=(reg_variant == "bounded"))
        dist_check = reduce_dist_check(torch, dist, world, gather_ok, p2["pass"], p2["worst_gated"], "cuda")
        dist_check.update({"images_checked_per_rank": n_chk, "rank0": {k: p2[k] for k in p2 if k.endswith("_rel_err") or k.endswith("_rel_rms")},
                           "placement_rank0": placement})

    cpu_baseline = None
    parity = None
    ref = None
    if args.full and rank == 0 and world == 1 and args.cpu_sample > 0:
        from oracle import hmr_oracle as O  # the checker, timed as the CPU baseline

        n = min(args.cpu_sample, B)
        img_np = images[:n].cpu().numpy()
        osmpl = O.SMPL(assets["smpl"])
        mean = O.load_mean_param(assets["mean"])

        def timed(batch, reps=5, warm=2):
            x = img_np[:batch]
            for _ in range(warm):
                r = O.predict(x, assets["enc"], leg.reg, osmpl, mean)
            ts_ = []
            for _ in range(reps):
                tc = time.perf_counter()
                r = O.predict(x, assets["enc"], leg.reg, osmpl, mean)
                ts_.append(time.perf_counter() - tc)
            ts_.sort()
            return r, ts_[len(ts_) // 2]

        _, t1 = timed(1)
        ref, tn = timed(n)
        cpu_baseline = {
            "value": round(n / tn, 3),
            "unit": "images/sec",
            "cores": int(torch.get_num_threads()),
            "kind": "port",
            "sample": "BASELINE.md §3 protocol: batch 1 and batch %d of the bench images, full path (ResNet-50 + 3 IEF stages + SMPL x3), "
                      "2 warm-ups then the median of 5 runs each; value = the batch-%d rate.  CPU restatement of the reference "
                      "(NumPy + torch-CPU conv2d), not TensorFlow" % (n, n),
            "batch1": {"images_per_sec": round(1.0 / t1, 3), "median_ms": round(t1 * 1e3, 2)},
            "batch%d" % n: {"images_per_sec": round(n / tn, 3), "median_ms": round(tn * 1e3, 2)},
        }
        cond = None
        if args.encoder_dtype == "fp32" and reg_variant != "bounded":
            cond = kp2d_conditioning(O, images.cpu().numpy(), assets, leg.reg, ref)
        parity = parity_block(leg.last_outputs()[-1], ref, n, dtype=args.encoder_dtype, gate_kp2d_rms=(reg_variant == "bounded"), kp2d_cond=cond)

    loss_parity = None
    if args.full and rank == 0 and world == 1 and args.cpu_sample == 0 and args.parity_sample > 0:
        from oracle import hmr_oracle as O  # the checker

        n = min(args.parity_sample, B)
        osmpl = O.SMPL(assets["smpl"])
        mean = O.load_mean_param(assets["mean"])
        ref = O.predict(images[:n].cpu().numpy(), assets["enc"], leg.reg, osmpl, mean, all_stages=True)
        cond = None
        if args.encoder_dtype == "fp32" and reg_variant != "bounded":
            cond = kp2d_conditioning(O, images.cpu().numpy(), assets, leg.reg, ref)
        parity = parity_block(leg.last_outputs()[-1], ref, n, dtype=args.encoder_dtype, gate_kp2d_rms=(reg_variant == "bounded"), kp2d_cond=cond)
        if args.config5:
            loss_parity = loss_parity_block(leg, O, ref, min(n, 2) if n >= 2 else n)

    # ---- the other single-GPU configurations of BASELINE.json, short legs in the same run (N == 1, default flags only)
    configs = None
    extras = {}
    default_headline = (args.encoder_dtype == "fp32" and not args.config5 and mode == "pipelined" and not args.from_host and B == 256)
    if args.full and rank == 0 and world == 1 and not use_dist and not args.no_legs and default_headline and not args.no_roofline:
        from oracle import hmr_oracle as O  # the checker

        K, W = args.leg_steps, 3
        configs = {}
        osmpl = O.SMPL(assets["smpl"])
        mean = O.load_mean_param(assets["mean"])

        def run_leg(name, fn):
            t_leg = time.perf_counter()
            try:
                blk = fn()
            except Exception as e:  # noqa: BLE001 -- a failing side leg is reported in the line, the headline stays
                import traceback

                traceback.print_exc(file=sys.stderr)
                blk = {"error": "%s: %s" % (type(e).__name__, e)}
            blk["leg_seconds"] = round(time.perf_counter() - t_leg, 1)
            return blk

        def leg_block(lg, K, desc, ref_, n_par, gate_kp2d=False):
            dt_ = lg.run_timed(K, W)
            ms = dt_ / K * 1e3
            roof, ph, _ = encoder_roofline(lg, ms)
            blk = {"workload": desc, "batch": lg.B, "steps": K, "warmup": W, "ms_per_step": round(ms, 4),
                   "images_per_sec": round(lg.B * K / dt_, 2), "dtype": "f32" if lg.dtype == "fp32" else "bf16 encoder, fp32 accumulate / regressor / SMPL",
                   "host_us_per_step": round(lg.host_s / K * 1e6, 1), "roofline": roof, "phase_ms": ph}
            if ref_ is not None:
                cond_ = None
                if lg.dtype == "fp32" and not gate_kp2d:
                    cond_ = kp2d_conditioning(O, images.cpu().numpy(), assets, lg.reg, ref_)
                blk["parity"] = parity_block(lg.last_outputs()[-1], ref_, n_par, dtype=lg.dtype, gate_kp2d_rms=gate_kp2d, kp2d_cond=cond_)
            return blk

        def fp32_b64():
            # configs[1] as written: batch 64, fp32, one GPU -- the same context, the first 64 bench images (one chunk, serial tile rule)
            lg = Leg(env, 64, images=images[:64].contiguous(), pred=leg.pred)
            return leg_block(lg, K, "configs[1]: batch=64 224x224x3 synthetic images, fp32 ResNet-50 v1 + 3-iter regressor + SMPL LBS at all 3 stages, "
                                    "1 MI355X", ref, min(64, args.cpu_sample) if ref is not None else 0)

        # The other configurations run as CHILD PROCESSES of this one (the same script, `--no-legs`), one after the other: a context that
        # is created after another one in the same process inherits that process's mapped hardware queues, and the legs
        # measured 3 % (bf16) to 14 % (hipGraph replay) below their own-process rate when they ran here (round 3's line: bf16 63.9 k
        # against 65.9 k, graph replay 15.6 ms against 13.8 ms).  The node's synthetic weights go through one file in /dev/shm, as
        # for the ranks of an N > 1 run.  The parent's context stays alive meanwhile: measured to make no difference to the child.
        import subprocess

        assets_path = "/dev/shm/hpe_bench_assets_legs_%d.npz" % os.getpid()
        save_assets(assets, assets_path)

        def child_leg(extra, parity_n, how):
            env_c = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "HPE_FORCE_DIST", "HPE_POWER_TRACE")}
            env_c["HPE_BENCH_ASSETS"] = assets_path
            cmd = [sys.executable, os.path.abspath(__file__), "--gpus", "1", "--steps", str(K), "--warmup", str(W), "--batch", str(B), "--cpu-sample", "0",
                   "--parity-sample", str(parity_n), "--sustain", "0", "--no-legs", "--full"] + extra
            r = subprocess.run(cmd, env=env_c, capture_output=True, text=True, timeout=900)
            lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
            if not lines:
                return {"error": "child `%s` exited with code %d: %s" % (" ".join(extra), r.returncode, r.stderr[-400:])}
            d = json.loads(lines[0])
            blk = {"workload": d["config"]["workload"], "batch": B, "steps": K, "warmup": W, "ms_per_step": d["ms_per_step"], "images_per_sec": d["value"],
                   "dtype": d["dtype"], "host_us_per_step": d.get("host_us_per_step"), "roofline": d.get("roofline"), "phase_ms": d.get("phase_ms"),
                   "how": "own process: python bench.py " + " ".join(cmd[2:]) + " -- " + how, "child_exit_code": r.returncode}
            for key in ("parity", "loss_roofline", "losses_last_step", "loss_parity"):
                if key in d:
                    blk[key] = d[key]
            return blk

        def bf16_b256():
            return child_leg(["--encoder-dtype", "bf16"], 8, "configs[3] on one GPU")

        def config5_b256(variant="bounded"):
            return child_leg(["--config5", "--regressor", variant], 2, "configs[4] on one GPU, %s" % (
                "well-conditioned synthetic regressor (camera scale 0.83 / 0.76 / 0.69: every stage on the cell-grid search)" if variant == "bounded" else
                "SURVEY regressor (camera scale 0.59 / 0.28 / -0.03: the meshes of stages 2-3 collapse into a few cells and take the full-search fallback)"))

        def graph_leg():
            # the same fp32 B = 256 step as ONE stream-ordered unit (encoder of batch k || tail of batch k-1) captured into hipGraphs
            blk = child_leg(["--graph"], 8, "step = fork; hpe_tail(features of batch k-1) on the ctx's tail stream || hpe_encoder(images of batch k); join, "
                                             "captured (torch.cuda.CUDAGraph; graphs: first / steady x 2 / flush x 2) and replayed")
            if "error" in blk:
                return blk
            return {"what": blk.pop("how"), "eager_pipelined": {"ms_per_step": round(ms_per_step, 4), "host_us_per_step": round(host_us, 1),
                                                               "images_per_sec": round(B * args.steps / dt, 2)},
                    "graph_replay": {"ms_per_step": blk["ms_per_step"], "host_us_per_step": blk["host_us_per_step"], "images_per_sec": blk["images_per_sec"]},
                    "parity_graph": blk.get("parity")}

        def from_host_leg(pred4):
            lg = Leg(env, B, from_host=True, images=images, pred=pred4)
            dt_ = lg.run_timed(K, W, timing=False)
            exact = 2.0 * (lg.frames_host[:4].numpy().astype(np.float64) / 255.0 - 0.5)
            err = float(np.abs(lg.img_dev[(lg.step_no - 1) & 1][:4].cpu().numpy() - exact).max())
            nbytes = int(lg.frames_host.numel())
            return {"what": "uint8 frames [256,224,224,3] in pinned host memory -> H2D on a copy stream (double buffered, overlaps the previous batch's "
                            "encoder) -> hpe_preprocess_u8_batch (one launch) -> the fp32 path; same step as the headline otherwise",
                    "ms_per_step": round(dt_ / K * 1e3, 4), "images_per_sec": round(B * K / dt_, 2), "host_us_per_step": round(lg.host_s / K * 1e6, 1),
                    "vs_resident": round((B * K / dt_) / (B * args.steps / dt), 4), "h2d_bytes_per_step": nbytes,
                    "preprocess_max_abs_err": err, "pass": bool(err <= 1e-6)}

        # Order matters: every HIP stream a process has ever used keeps a hardware queue mapped, and a fifth mapped queue costs the
        # bf16 step ~20 % (DESIGN.md "hardware queues").  So each leg runs with ONE context alive (its 2 chunk-stream + tail-stream
        # queues), the headline's context is destroyed before the bf16 / config-5 contexts are created, and the legs that need extra
        # torch streams (graph capture, the H2D copy stream) run last.
        configs["fp32_b64"] = run_leg("fp32_b64", fp32_b64)
        try:
            # from_host stays in this process (it shares nothing but the headline's predictor and checks the preprocess kernel's output)
            extras["from_host"] = run_leg("from_host", lambda: from_host_leg(leg.pred))
        except Exception as e:  # noqa: BLE001
            extras["from_host"] = {"error": "%s: %s" % (type(e).__name__, e)}
        configs["bf16_b256"] = run_leg("bf16_b256", bf16_b256)
        configs["config5_b256"] = run_leg("config5_b256", config5_b256)
        configs["config5_b256_survey"] = run_leg("config5_b256_survey", lambda: config5_b256("survey"))
        extras["graph"] = run_leg("graph", graph_leg)
        if os.path.exists(assets_path):
            os.remove(assets_path)

    if rank == 0:
        value = world * B * args.steps / dt
        if world > 1:
            cfg_name = "configs[4]" if args.config5 else ("configs[3]" if args.encoder_dtype == "bf16" else "configs[2]")
        else:
            cfg_name = ("configs[4] on one GPU" if args.config5 else ("configs[3] on one GPU" if args.encoder_dtype == "bf16" else
                        ("configs[1] as written" if B == 64 else "configs[1] at batch %d" % B)))
        line = {
            "metric": "images/sec (224x224, batch 256/GPU)",
            "value": round(value, 2),
            "unit": "images/sec",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 4),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f32" if args.encoder_dtype == "fp32" else "bf16 (encoder; fp32 accumulate, fp32 regressor+SMPL)",
            "data": "synthetic",
            "config": {
                "workload": "batch=%d/GPU 224x224x3 synthetic images, %s ResNet-50 v1 + 3-iter regressor + SMPL LBS at all 3 stages%s (%s%s)" % (
                    B, args.encoder_dtype, ", RCCL all-gather of theta" if use_dist else "", cfg_name,
                    "; the BASELINE metric batch" if B == 256 else "; NOT the metric batch of 256"),
                "global_batch": world * B,
                "parallelism": "dp%d (batch shard, replicated weights)" % world,
                "regressor": "synthetic '%s' variant" % reg_variant,
                "pipeline": {"pipelined": "regressor+SMPL tail of batch k overlaps the encoder of batch k+1 (tail stream); all work of the K steps "
                                          "completes inside the timed region",
                             "serial": "serial steps",
                             "graph": "hipGraph replay per step: encoder of batch k || regressor+SMPL tail of batch k-1, flushed inside the timed region"}[mode],
                "input": "uint8 frames in pinned host memory (H2D + batched preprocess inside the step)" if args.from_host else "float32 images resident in HBM",
            },
            "host_us_per_step": round(host_us, 1),
            "roofline": roofline,
            "cpu_baseline": cpu_baseline,
        }
        if args.config5:
            line["config"]["workload"] += " + kp/mesh reprojection losses of all 3 stages, one all-reduce of the [3,4] loss block"
            pk = leg.last_losses().cpu().numpy()
            line["losses_last_step"] = {"kpr": [float(60.0 * x) for x in pk[:, 2]], "mr": [float(0.001 * x) for x in pk[:, 3]]}
            line["loss_roofline"] = loss_roofline
        if phase:
            line["phase_ms"] = phase
        if sustained:
            line["sustained"] = sustained
        if parity:
            line["parity"] = parity
        if loss_parity:
            line["loss_parity"] = loss_parity
        if dist_check:
            line["dist_check"] = dist_check
        if configs:
            line["configs"] = configs
        line.update(extras)
        if configs:
            # the LAST key of the line: the figures of every leg in one short block (a log tail that keeps only the end of the line keeps this)
            def _ips(blk):
                return blk.get("images_per_sec") if isinstance(blk, dict) else None

            line["summary_images_per_sec"] = {"fp32_b256_headline": round(value, 1), **{k: _ips(v) for k, v in configs.items()},
                                              "from_host": _ips(extras.get("from_host")),
                                              "graph_replay": (extras.get("graph") or {}).get("graph_replay", {}).get("images_per_sec"),
                                              "bf16_b256_frac_of_8TBs": ((configs.get("bf16_b256") or {}).get("roofline") or {}).get("frac"),
                                              "fp32_b256_frac_of_157TF": (roofline or {}).get("frac")}
        # stdout carries exactly one line: native libraries (RCCL prints a version banner on fd 1 when its communicator is
        # created) wrote to stderr for the whole run, the JSON goes to the real stdout
        sys.stdout.flush()
        os.dup2(real_stdout, 1)
        print(json.dumps(line), flush=True)
        os.dup2(2, 1)
    failed = []
    if parity is not None and not parity["pass"]:
        failed.append("headline parity: worst gated relative error %.3g" % parity["worst_gated"])
    if loss_parity is not None and not loss_parity["pass"]:
        failed.append("loss parity: worst relative error %.3g" % loss_parity["worst_rel_err"])
    if dist_check is not None and dist_check_failed(dist_check):
        failed.append("dist_check: %s" % json.dumps({k: v for k, v in dist_check.items() if k != "rank0"}))
    for name, blk in list((configs or {}).items()) + list(extras.items()):
        for key in ("parity", "loss_parity", "parity_graph"):
            if isinstance(blk.get(key), dict) and blk[key].get("pass") is False:
                failed.append("%s.%s: worst %.3g" % (name, key, blk[key].get("worst_gated", blk[key].get("worst_rel_err", float("nan")))))
        if blk.get("pass") is False:
            failed.append("%s: check failed" % name)
    if use_dist:
        dist.destroy_process_group()
    if failed:
        print("bench.py: PARITY FAILED: " + "; ".join(failed), file=sys.stderr)
        sys.exit(3)


if __name__ == "__main__":
    main()
