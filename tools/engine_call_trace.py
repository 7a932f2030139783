"""What the Python binding asks of libhpe_hip.so, and what comes back, as text that two trees can be compared by (cmp).

    python tools/engine_call_trace.py --out trace.txt

Builds the synthetic engine of tests/test_gpu_encoder_bn_mixed.py (encoder of seed 7 with gamma in [0.5, 1.5], fp32 context, here with
max_batch 3, SMPL, regressor, mean theta and critic loaded, reserve_encoder_train(3, batch_norm=True, precision="mixed")) and a second,
bf16 context, then puts a recorder in place of the loaded library (``engine.lib`` and ``_lib.load()``) that forwards every call, and runs
one fixed script over HpeEngine: forward / tail / the two plan builders (eager and graph), SMPL and its backward, the critic and regressor
training calls with and without their optional arguments, every encoder-training and one-layer debug call in each (bn, precision)
combination it accepts, the refusals, the statistics and parameter setters and the loss calls.  Shapes are the smallest that tell the
branches apart: B = 2 and 3, N = 2 critic rows, res3a_branch1 (1x1), res2a_branch2b (3x3) and layer 0 for the one-layer calls.

One line per library call: the symbol, every scalar argument, null / nonnull for every pointer (never the address; the fields of an
HpeOutputs one by one) and the result.  One line per returned tensor: shape, dtype, SHA-256 of its bytes.  Each line starts with its
section; the sections named enc_* are the encoder-training calls.  Run it from a checkout of each tree, a fresh process each, and compare
the files: a refactor of the binding leaves them identical (profiles/engine_binding_ab.txt)."""
import argparse
import ctypes as C
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import hpe_amd  # noqa: E402
from hpe_amd import _lib, engine as engine_mod, synthetic  # noqa: E402
from hpe_amd.resnet_spec import CONV_INDEX, CONV_SPECS  # noqa: E402
from oracle import hmr_oracle as O  # noqa: E402

LINES = []
SECTION = ["setup"]


def emit(text):
    LINES.append("%-12s| %s" % (SECTION[0], text))


def _pointer(v):
    if isinstance(v, (C.c_void_p, C.c_char_p)):
        v = v.value
    return "nonnull" if v else "null"


def _describe(arg, argtype):
    obj = getattr(arg, "_obj", arg)  # byref(x) -> x
    if isinstance(obj, C.Array) and issubclass(obj._type_, C.Structure):
        return "[" + ", ".join(_describe(o, None) for o in obj) + "]"
    if isinstance(obj, C.Structure):
        return "{" + " ".join("%s=%s" % (n, _pointer(getattr(obj, n)) if t is C.c_void_p else getattr(obj, n)) for n, t in obj._fields_) + "}"
    if isinstance(obj, C.Array) and obj._type_ is C.c_void_p:
        return "[" + ", ".join(_pointer(o) for o in obj) + "]"
    if isinstance(obj, (C.Array, C._CFuncPtr)):
        return "nonnull"
    if argtype in (C.c_int, C.c_longlong):
        return "%d" % int(arg)
    if argtype in (C.c_float, C.c_double):
        return repr(float(arg))
    return _pointer(arg)


class Recorder(object):
    """stands in for the ctypes library: every attribute is the real function behind a wrapper that writes the call down"""

    def __init__(self, lib):
        self._real = lib

    def __getattr__(self, name):
        fn = getattr(self._real, name)

        def call(*args):
            types = list(fn.argtypes or ())
            shown = ", ".join(_describe(a, types[i] if i < len(types) else None) for i, a in enumerate(args))
            rc = fn(*args)
            emit("lib %s(%s) -> %s" % (name, shown, rc if fn.restype in (C.c_int, C.c_longlong, C.c_char_p) else _pointer(rc)))
            return rc

        return call


def _tensors(label, value):
    if isinstance(value, torch.Tensor):
        raw = value.detach().contiguous().cpu().reshape(-1).view(torch.uint8).numpy().tobytes()
        emit("ret %s %s %s %s" % (label, tuple(value.shape), str(value.dtype).replace("torch.", ""), hashlib.sha256(raw).hexdigest()))
    elif isinstance(value, dict):
        for k in sorted(value):
            _tensors("%s[%s]" % (label, k), value[k])
    elif isinstance(value, (list, tuple)) and any(isinstance(v, (torch.Tensor, dict, list, tuple)) for v in value):
        for i, v in enumerate(value):
            _tensors("%s[%d]" % (label, i), v)
    else:
        emit("ret %s %r" % (label, value))


def run(label, fn, refused=None):
    """one scripted call: its library calls, then its result tensor by tensor; refused: the exception it has to end in"""
    emit("call %s" % label)
    if refused is not None:
        try:
            fn()
        except refused as e:
            emit("raised %s: %s" % (type(e).__name__, e))
            return None
        raise AssertionError("%s was not refused" % label)
    out = fn()
    torch.cuda.synchronize()
    _tensors(label, out)
    return out


def rnd(seed, *shape, dtype=torch.float32, relu=False):
    t = torch.randn(*shape, generator=torch.Generator().manual_seed(seed))
    return (t.clamp_min(0) if relu else t).to(dtype).cuda()


def make_params():
    p = synthetic.make_encoder_params(seed=7)
    g = np.random.default_rng(11)
    for s in CONV_SPECS:
        p[s.bn_name + "/gamma"] = g.uniform(0.5, 1.5, s.cout).astype(np.float32)
    return p


def make_engine(params, **kw):
    e = hpe_amd.HpeEngine(device=0, max_batch=3, **kw)
    e.load_smpl(synthetic.make_smpl_model())
    e.load_encoder(params)
    e.load_regressor(synthetic.make_regressor_params())
    e.load_mean_theta(O.load_mean_param(synthetic.make_mean_params()))
    e.load_critic(synthetic.make_critic_params())
    e.finalize()
    return e


def serving(e, bf):
    SECTION[0] = "serve"
    img = {B: torch.from_numpy(synthetic.make_images(B, seed=40 + B)).cuda() for B in (2, 3)}
    for B in (2, 3):
        for all_stages in (False, True):
            run("forward B=%d all_stages=%d" % (B, all_stages), lambda: e.forward(img[B], all_stages=all_stages))
    run("forward want=verts2d,Rs", lambda: e.forward(img[2], want=("verts2d", "Rs", "cams")))
    keep = run("forward pipelined", lambda: (e.forward(img[3], all_stages=True, pipelined=True), e.join())[0])
    del keep
    feat = run("encoder", lambda: e.encoder(img[3]))
    for all_stages in (False, True):
        run("tail all_stages=%d" % all_stages, lambda: e.tail(feat, all_stages=all_stages))
    run("regress_stage", lambda: e.regress_stage(feat))
    run("regress_stage theta_prev", lambda: e.regress_stage(feat, rnd(1, 3, 85)))
    run("bf16 forward", lambda: bf.forward(img[2], all_stages=True))
    for name in ("res2b_branch2c", "res3b_branch2c"):  # the chained launch of an identity block, C = 64 and C = 128
        i = CONV_INDEX[name]
        s, first = CONV_SPECS[i], CONV_SPECS[i + 1].name.endswith("branch1")
        run("bf16 debug_chain %s" % name, lambda: bf.debug_chain(i, rnd(2, 2, s.hin, s.hin, s.cin, relu=True),
                                                                  rnd(3, 2, s.hout, s.hout, CONV_SPECS[i + 1].cin if first else s.cout, relu=True)))

    SECTION[0] = "plan"
    for kw in (dict(), dict(all_stages=True), dict(graph=True), dict(all_stages=True, want=("verts", "kp2d", "verts2d"), graph=True)):
        def forward_plan():
            step, outs = e.make_forward_plan(2, **kw)
            for k in range(2):
                step(img[2] if k == 0 else img[3][1:])
            return outs
        run("make_forward_plan %r" % sorted(kw.items()), forward_plan)
    def pipelined_plan():
        step, outs = e.make_forward_plan(2, pipelined=True)
        step(img[2])
        step(img[3][:2])
        e.join()
        return outs
    run("make_forward_plan pipelined", pipelined_plan)
    run("make_forward_plan pipelined graph", lambda: e.make_forward_plan(2, pipelined=True, graph=True), refused=ValueError)
    kp_gt, losses = rnd(9, 2, 19, 3), torch.zeros(3, 3, 4, device="cuda")
    for graph in (False, True):
        for n_sets in (2, 3):
            for extra in (False, True):
                def overlapped_plan():
                    def tail_extra(outs, k):
                        emit("tail_extra set %d" % k)
                        e.val_losses(kp_gt, [o["kp2d"] for o in outs], out=losses[k])
                    step = e.make_overlapped_plan(2, all_stages=extra, graph=graph, n_sets=n_sets, tail_extra=tail_extra if extra else None)
                    got = []
                    for k in range(3):
                        r = step(img[3][k % 2:k % 2 + 2])
                        torch.cuda.synchronize()
                        got.append((step.last, None if r is None else [{n: t.clone() for n, t in o.items()} for o in r]))
                    r = step.flush()
                    torch.cuda.synchronize()
                    got.append((step.last, r, len(step.sets), step.flush() is None, losses.clone()))
                    if graph:
                        got.append([len(g) if isinstance(g, list) else 1 for g in step.graphs])
                    return got
                run("make_overlapped_plan graph=%d n_sets=%d tail_extra=%d" % (graph, n_sets, extra), overlapped_plan)


def heads(e):
    SECTION[0] = "smpl"
    th = torch.from_numpy(synthetic.make_thetas(4, seed=8)).cuda()
    run("smpl", lambda: e.smpl(th[:3]))
    run("smpl want=verts,joints", lambda: e.smpl(th[:2], want=("verts", "joints")))
    run("smpl_backward B=4", lambda: e.smpl_backward(th, {"verts": rnd(4, 4, 6890, 3), "joints": None, "kp2d": rnd(5, 4, 19, 2), "Rs": rnd(6, 4, 24, 3, 3)}))
    run("smpl_backward B=2", lambda: e.smpl_backward(th[:2], {"J_transformed": rnd(7, 2, 24, 3)}))
    run("smpl_backward unknown", lambda: e.smpl_backward(th[:2], {"faces": None}), refused=KeyError)

    SECTION[0] = "critic"
    theta = torch.from_numpy(synthetic.make_thetas(2, seed=9)).cuda()
    joints, Rs, betas = rnd(10, 2, 19, 3), rnd(11, 2, 24, 3, 3), theta[:, 75:]
    gs = rnd(12, 2, 3)
    run("critic", lambda: e.critic(joints, betas, Rs))
    run("critic want_kcs", lambda: e.critic(joints, betas.contiguous(), Rs, want_kcs=True))
    run("critic_backward", lambda: e.critic_backward(joints, betas, Rs))
    run("critic_backward grad_scores kcs", lambda: e.critic_backward(joints, betas, Rs, grad_scores=gs, want=("kcs", "betas")))
    run("critic_backward bad want", lambda: e.critic_backward(joints, betas, Rs, want=("theta",)), refused=ValueError)
    run("critic_reserve", lambda: e.critic_reserve(2))
    run("critic_weight_grad grad_scores", lambda: e.critic_weight_grad(joints, betas, Rs, grad_scores=gs))
    run("critic_weight_grad shared tangents", lambda: e.critic_weight_grad(joints, betas, Rs, tangents={"kcs": rnd(13, 13, 13), "betas": rnd(14, 10), "Rs": None}))
    run("critic_weight_grad per-row tangents", lambda: e.critic_weight_grad(joints, betas, Rs, grad_scores=gs, tangents={"joints": rnd(15, 2, 14, 3), "Rs": rnd(16, 2, 23, 3, 3)}))
    run("critic_weight_grad nothing", lambda: e.critic_weight_grad(joints, betas, Rs), refused=ValueError)
    flat = run("critic_params", lambda: e.critic_params())
    run("set_critic_params", lambda: e.set_critic_params(flat * 0.5))
    run("set_critic_params short", lambda: e.set_critic_params(flat[:-1]), refused=ValueError)
    run("critic after set", lambda: e.critic(joints, betas, Rs))

    SECTION[0] = "regressor"
    feat, gth = rnd(20, 2, 2048, relu=True), rnd(21, 3, 2, 85)
    drop = (torch.rand(2, 2, 1024, generator=torch.Generator().manual_seed(22)) < 0.8).float().cuda() / 0.8
    run("regressor_forward_train", lambda: e.regressor_forward_train(feat))
    run("regressor_forward_train drop", lambda: e.regressor_forward_train(feat, drop))
    run("regressor_backward", lambda: e.regressor_backward(feat, gth))
    run("regressor_backward drop no features", lambda: e.regressor_backward(feat, gth, drop, want_grad_features=False))
    run("regressor_backward no grad_thetas", lambda: e.regressor_backward(feat, None, drop))
    run("regressor_backward bad drop", lambda: e.regressor_backward(feat, gth, drop[:, :1]), refused=ValueError)
    flat = run("regressor_params", lambda: e.regressor_params())
    run("set_regressor_params", lambda: e.set_regressor_params(flat * 0.5))
    run("set_regressor_params short", lambda: e.set_regressor_params(flat[1:]), refused=ValueError)
    run("regressor_forward_train after set", lambda: e.regressor_forward_train(feat))

    SECTION[0] = "loss"
    tg = synthetic.make_lsp_targets(2, seed=4)
    seg, kp_gt = torch.from_numpy(tg[0][..., 0].copy()).cuda(), torch.from_numpy(tg[1]).cuda()
    v2d, kp = [rnd(30 + i, 2, 6890, 2) * 0.3 for i in range(2)], [rnd(33 + i, 2, 19, 2) for i in range(2)]
    run("mesh_loss", lambda: e.mesh_loss(seg, v2d[0]))
    run("mesh_loss_grad", lambda: e.mesh_loss_grad(seg, v2d[0]))
    run("mesh_loss_grad neighbours", lambda: e.mesh_loss_grad(seg, v2d[1], want_neighbours=True))
    run("val_losses", lambda: e.val_losses(kp_gt, kp, seg, v2d))
    run("val_losses out", lambda: e.val_losses(kp_gt, kp, seg, v2d, out=torch.zeros(2, 4, device="cuda")))
    run("kp_loss_backward", lambda: engine_mod.kp_loss_backward(kp_gt, kp[0]))
    run("kp_loss_backward grad_loss", lambda: engine_mod.kp_loss_backward(kp_gt, kp[0], torch.full((1,), 0.5, device="cuda")))
    run("kp_loss_parts", lambda: engine_mod.kp_loss_parts(kp_gt, kp[1]))


def encoder_training(e):
    BF = torch.bfloat16
    SECTION[0] = "enc_refuse"
    img = {B: torch.from_numpy(synthetic.make_images(B, seed=50 + B)).cuda() for B in (2, 3)}
    gf = {B: rnd(60 + B, B, 2048) for B in (2, 3)}
    for precision in ("fp32", "bf16"):
        run("encoder_stash before a forward %s" % precision, lambda: e.encoder_stash(0, precision=precision), refused=hpe_amd.HpeError)
    for precision in ("fp32", "mixed"):
        run("encoder_stash_raw before a forward %s" % precision, lambda: e.encoder_stash_raw(0, precision=precision), refused=hpe_amd.HpeError)
    run("forward bf16 batch", lambda: e.encoder_forward_train(img[2], bn="batch", precision="bf16"), refused=ValueError)
    run("backward bf16 batch", lambda: e.encoder_backward(img[2], gf[2], bn="batch", precision="bf16"), refused=ValueError)
    run("reserve bf16 batch", lambda: e.reserve_encoder_train(3, batch_norm=True, precision="bf16"), refused=ValueError)
    run("stash_raw bf16", lambda: e.encoder_stash_raw(0, precision="bf16"), refused=ValueError)
    run("forward bad bn", lambda: e.encoder_forward_train(img[2], bn="moving"), refused=ValueError)
    run("backward bad precision", lambda: e.encoder_backward(img[2], gf[2], precision="fp16"), refused=ValueError)
    run("backward bad grad_features", lambda: e.encoder_backward(img[2], gf[3]), refused=ValueError)
    run("debug_conv_backward float32 x as mixed", lambda: e.debug_conv_backward(1, rnd(1, 2, 56, 56, 64), None, rnd(2, 2, 56, 56, 64), precision="bf16"),
        refused=TypeError)

    SECTION[0] = "enc_walk"
    for batch_norm, precision in ((False, "fp32"), (False, "bf16"), (False, "mixed"), (True, "fp32"), (True, "mixed")):
        run("reserve_encoder_train batch_norm=%d %s" % (batch_norm, precision), lambda: e.reserve_encoder_train(3, batch_norm=batch_norm, precision=precision))
    for B in (2, 3):
        for bn, precision in (("frozen", "fp32"), ("frozen", "bf16"), ("frozen", "mixed"), ("batch", "fp32"), ("batch", "mixed")):
            tag = "B=%d %s %s" % (B, bn, precision)
            run("encoder_forward_train " + tag, lambda: e.encoder_forward_train(img[B], bn=bn, precision=precision))
            for idx in (0, 10, 52, -1):
                run("encoder_stash %d %s" % (idx, tag), lambda: e.encoder_stash(idx, precision="fp32" if precision == "fp32" else "bf16"))
                if bn == "batch" and idx >= 0:
                    run("encoder_stash_raw %d %s" % (idx, tag), lambda: e.encoder_stash_raw(idx, precision=precision))
            if bn == "batch":
                run("encoder_batch_stats " + tag, lambda: e.encoder_batch_stats())
            run("encoder_backward " + tag, lambda: e.encoder_backward(img[B], gf[B], bn=bn, precision=precision))

    SECTION[0] = "enc_layer"
    for B in (2, 3):
        for name in ("res3a_branch1", "res2a_branch2b", "conv1", "res2a_branch2c"):
            idx = CONV_INDEX[name] if name != "conv1" else 0
            s = CONV_SPECS[idx]
            x32 = rnd(100 + idx, B, s.hin, s.hin, s.cin, relu=idx != 0)
            yzd = [rnd(200 + 3 * idx + i, B, s.hout, s.hout, s.cout, relu=i == 0) for i in range(3)]  # y, z, dy
            res32 = rnd(300 + idx, B, s.hout, s.hout, s.cout) if name.endswith("2c") else None
            for precision in ("fp32", "bf16", "mixed"):
                dt = torch.float32 if precision == "fp32" else BF
                x = x32 if idx == 0 else x32.to(dt)
                y, z, dy = (t.to(dt) for t in yzd)
                res = res32.to(dt) if res32 is not None else None
                tag = "%s B=%d %s" % (name, B, precision)
                run("debug_conv_backward " + tag, lambda: e.debug_conv_backward(idx, x, y, dy, precision=precision))
                run("debug_conv_backward ungated no dx " + tag, lambda: e.debug_conv_backward(idx, x, None, dy, want_dx=False, precision=precision))
                if precision == "bf16":
                    continue
                run("debug_conv_batchnorm " + tag, lambda: e.debug_conv_batchnorm(idx, x, res, relu=res is None, precision=precision))
                run("debug_conv_backward_batchnorm " + tag, lambda: e.debug_conv_backward_batchnorm(idx, x, z, y, dy, precision=precision))
                run("debug_conv_backward_batchnorm ungated no dx " + tag,
                    lambda: e.debug_conv_backward_batchnorm(idx, x, z, None, dy, want_dx=False, precision=precision))
            run("debug_conv %s B=%d" % (name, B), lambda: e.debug_conv(idx, x32, residual=res32, relu=res32 is None))
            y, z, dy = yzd
            M = 2 * B * s.hout * s.hout  # as if a second rank held as many rows
            sums = run("debug_bn_sums %s B=%d" % (name, B), lambda: e.debug_bn_sums(idx, z))
            run("debug_bn_finish %s B=%d" % (name, B), lambda: e.debug_bn_finish(idx, sums * 2, M, z, residual=res32, relu=res32 is None))
            bsums = run("debug_bn_backward_sums %s B=%d" % (name, B), lambda: e.debug_bn_backward_sums(idx, z, y, dy, sums * 2, M))
            run("debug_bn_backward_sums ungated %s B=%d" % (name, B), lambda: e.debug_bn_backward_sums(idx, z, None, dy, sums * 2, M))
            run("debug_bn_backward_finish %s B=%d" % (name, B), lambda: e.debug_bn_backward_finish(idx, x32, z, y, dy, sums * 2, bsums * 2, M))
            run("debug_bn_backward_finish ungated no dx %s B=%d" % (name, B),
                lambda: e.debug_bn_backward_finish(idx, x32, z, None, dy, sums * 2, bsums * 2, M, want_dx=False))
        for precision in ("fp32", "bf16"):
            dt = torch.float32 if precision == "fp32" else BF
            run("debug_maxpool_backward B=%d %s" % (B, precision),
                lambda: e.debug_maxpool_backward(rnd(400, B, 112, 112, 64, dtype=dt, relu=True), rnd(401, B, 56, 56, 64, dtype=dt), precision=precision))
            run("debug_avgpool_backward B=%d %s" % (B, precision), lambda: e.debug_avgpool_backward(rnd(402, B, 2048), 49, precision=precision))

    SECTION[0] = "enc_state"
    stats = run("encoder_stats", lambda: e.encoder_stats())
    e.encoder_forward_train(img[3], bn="batch", precision="mixed")
    run("update_encoder_stats", lambda: e.update_encoder_stats(stats.clone(), momentum=0.9))
    run("update_encoder_stats biased", lambda: e.update_encoder_stats(stats, momentum=0.5, unbiased=False))
    run("update_encoder_stats short", lambda: e.update_encoder_stats(stats[:-1]), refused=ValueError)
    run("set_encoder_stats_dev", lambda: e.set_encoder_stats_dev(stats))
    run("set_encoder_stats_dev 2-D", lambda: e.set_encoder_stats_dev(stats.reshape(2, -1)), refused=ValueError)
    run("encoder_stats after set", lambda: e.encoder_stats())
    flat = run("encoder_params", lambda: e.encoder_params())
    run("set_encoder_params_dev", lambda: e.set_encoder_params_dev(flat * 0.75))
    run("set_encoder_params_dev short", lambda: e.set_encoder_params_dev(flat[:-1]), refused=ValueError)
    run("encoder_forward_train after set_dev", lambda: e.encoder_forward_train(img[2], precision="mixed"))
    run("set_encoder_params", lambda: e.set_encoder_params(flat))
    run("encoder_params after set", lambda: e.encoder_params())
    run("encoder_backward after set", lambda: e.encoder_backward(img[2], gf[2], bn="batch"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    params = make_params()
    e = make_engine(params)
    e.reserve_encoder_train(3, batch_norm=True, precision="mixed")
    bf = make_engine(params, encoder_dtype="bf16")
    e.lib = bf.lib = _lib._lib = Recorder(_lib.load())
    encoder_training(e)  # first: the "before a forward" refusals need a context that has not run one
    serving(e, bf)
    heads(e)
    SECTION[0] = "end"
    run("check_device", lambda: e.check_device())
    e.lib = bf.lib = _lib._lib = e.lib._real
    e.close()
    bf.close()
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
    print("%d lines, sha256 %s" % (len(LINES), hashlib.sha256("\n".join(LINES).encode()).hexdigest()))


if __name__ == "__main__":
    main()
