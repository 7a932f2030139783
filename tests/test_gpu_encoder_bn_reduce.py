"""Batch statistics over the batch of ALL ranks (hpe_encoder_set_reduce) on one GPU, no process group: the two halves of a layer's
reductions with the parts' sums added on the host, an identity hook in a world of one, and two ranks as two engines in one process whose
hooks meet at a barrier.  The bars are those of tests/test_gpu_encoder_bn_train.py: statistics within four half-ulps of float of the
float64 statistics of the z they were taken from, everything else within 4 x the error of the float64 restatement
(tests/encoder_bn_train_ref.py, which IS BatchNorm over the global batch) run in float32 on the same inputs.

Figures of one run on an MI355X: DESIGN.md "Data-parallel training"."""
import threading

import pytest
import torch

import encoder_bn_train_ref as RB
import encoder_train_ref as R
import test_gpu_encoder_bn_train as T
from hpe_amd import _lib, distributed as D, resnet_spec, synthetic
from hpe_amd.resnet_spec import CONV_SPECS, ENCODER_PARAM_OFFSETS, ENCODER_STAT_OFFSETS

pytestmark = pytest.mark.gpu
MARGIN, ULP4, FEATURE_BAR = T.MARGIN, T.ULP4, T.FEATURE_BAR
N_LAYERS = len(CONV_SPECS)


def _pick(pred):
    return next(i for i, s in enumerate(CONV_SPECS) if pred(s))


# conv1, a 3x3, a stride-2 1x1 and a stage-5 1x1 (the last expand convolution: 2048 channels, with a residual)
LAYERS = [0, _pick(lambda s: s.kh == 3), _pick(lambda s: s.kh == 1 and s.stride == 2), N_LAYERS - 1]


@pytest.fixture(scope="module")
def params():
    return T.make_params()


@pytest.fixture(scope="module")
def engine(params):
    e = T.make_engine(params)  # max_batch 4, reserved for 3
    yield e
    e.close()


def _stats_errors(mu, var, z):
    mu64, var64 = RB.batch_stats(z.double())
    emu = float(((mu.double() - mu64).abs() / torch.maximum(mu64.abs(), var64.sqrt())).max())
    evar = float(((var.double() - var64).abs() / var64).max())
    return emu, evar, mu64, var64


@pytest.mark.parametrize("idx", LAYERS)
def test_layer_split(engine, params, idx):
    """B = 3 rows as 2 + 1: the debug sums of each part, added in double on the host, finished with the M of the three rows"""
    s = CONV_SPECS[idx]
    B, cut = 3, 2
    M = B * s.hout * s.hout
    x, res, dy = T._layer_inputs(s, idx, B)
    relu = not s.name.endswith("branch1")
    _, z, _ = engine.debug_conv_batchnorm(idx, x.cuda(), res.cuda() if res is not None else None, relu=relu)
    parts = [slice(0, cut), slice(cut, B)]
    part = lambda t, p: t[p].contiguous().cuda() if t is not None else None  # noqa: E731
    zs = [z[p].contiguous() for p in parts]
    sums = sum(engine.debug_bn_sums(idx, zp).cpu() for zp in zs).cuda()  # float64, added on the host
    outs = [engine.debug_bn_finish(idx, sums, M, zp, part(res, p), relu=relu) for zp, p in zip(zs, parts)]
    assert torch.equal(outs[0][1], outs[1][1])  # the same sums, the same statistics
    y, st = torch.cat([o[0] for o in outs]).cpu(), outs[0][1].cpu()
    zc = z.cpu()
    emu, evar, mu64, var64 = _stats_errors(st[:s.cout], st[s.cout:], zc)
    lt, lt32 = R.layer_tensors(params, s), R.layer_tensors(params, s, torch.float32)
    r64 = res.double() if res is not None else None
    ref = RB.layer_apply(zc.double(), mu64, var64, lt[2], lt[3], r64, relu)
    f32 = RB.layer_apply(zc, *RB.batch_stats(zc), lt32[2], lt32[3], res, relu)
    ey, bar = R.rel(y, ref), MARGIN * R.rel(f32, ref)
    print("split layer %2d %-16s mu %.3g  var %.3g (bar %.3g)  y %.3g (bar %.3g)" % (idx, s.name, emu, evar, ULP4, ey, bar))
    assert emu <= ULP4 and evar <= ULP4, (s.name, emu, evar)
    assert ey < bar, (s.name, ey, bar)
    # the backward: every part's sums with the statistics of all rows, added on the host, then every part's finish
    gated = relu
    ys = [o[0] if gated else None for o in outs]
    bsums = sum(engine.debug_bn_backward_sums(idx, zp, yp, part(dy, p), sums, M).cpu() for zp, yp, p in zip(zs, ys, parts)).cuda()
    back = [engine.debug_bn_backward_finish(idx, part(x, p), zp, yp, part(dy, p), sums, bsums, M) for zp, yp, p in zip(zs, ys, parts)]
    torch.cuda.synchronize()
    got = R.split_layer_grad(s, back[0][1].cpu() + back[1][1].cpu())  # each entry a partial: their sum is the layer's gradient
    # the local dbeta of a part is the rounded sum of its own rows
    local = engine.debug_bn_backward_sums(idx, zs[1], ys[1], part(dy, parts[1]), sums, M).cpu()
    assert torch.equal(R.split_layer_grad(s, back[1][1].cpu())["dbeta"], local[0].float())
    yc = y if gated else None
    ref = RB.layer_backward(s, x.double(), zc.double(), yc, dy.double(), lt, gated=gated)
    f32 = RB.layer_backward(s, x, zc, yc, dy, lt32, gated=gated)
    assert float(got.pop("db").abs().max()) == 0.0
    if idx != 0:
        got["dx"] = torch.cat([b[0] for b in back]).cpu()
    for k, v in got.items():
        e, bar = R.rel(v, ref[k]), MARGIN * R.rel(f32[k], ref[k])
        print("split layer %2d %-16s %-6s gpu %.3g  bar %.3g" % (idx, s.name, k, e, bar))
        assert e < bar, (s.name, k, e, bar)


def test_world_of_one_is_bit_exact(engine):
    """an identity hook with G = B: features, grad_flat, the batch statistics and the moved statistics have the bits of the path without
    a hook; 53 hook calls per forward, 2 x 53 per backward (which runs its own forward), each on the layer's 2 * cout doubles"""
    img = torch.from_numpy(synthetic.make_images(2, seed=31)).cuda()
    gf = torch.randn(2, 2048, generator=torch.Generator().manual_seed(3)).cuda()

    def run():
        feat = engine.encoder_forward_train(img, bn="batch")
        n_fwd = len(calls)
        grad = engine.encoder_backward(img, gf, bn="batch")
        moved = engine.update_encoder_stats(engine.encoder_stats(), momentum=0.9, unbiased=True)
        return (feat, grad, engine.encoder_batch_stats(), moved), n_fwd

    calls = []
    plain, _ = run()
    assert calls == []
    hook = _lib.REDUCE_FN(lambda user, ptr, count, stream: calls.append(count) or 0)
    engine.set_encoder_reduce(hook, 2)
    try:
        hooked, n_fwd = run()
    finally:
        engine.set_encoder_reduce(None)
    assert n_fwd == N_LAYERS and len(calls) == N_LAYERS + 2 * N_LAYERS
    walk = [2 * CONV_SPECS[i].cout for i in _forward_order()]
    assert calls[:N_LAYERS] == walk and calls[N_LAYERS:2 * N_LAYERS] == walk
    assert sorted(calls[2 * N_LAYERS:]) == sorted(walk)
    for a, b in zip(plain, hooked):
        assert torch.equal(a, b)
    again, _ = run()  # the hook cleared: the plain path, bit for bit, and no call
    assert len(calls) == 3 * N_LAYERS
    for a, b in zip(plain, again):
        assert torch.equal(a, b)


def _forward_order():
    order = [0]
    for i2a, i2b, i2c, i1 in R.blocks():
        order += [i2a, i2b] + ([i1] if i1 is not None else []) + [i2c]
    return order


class Meeting(object):
    """two hooks that meet: each leaves its buffer, rank 0 adds the two, both take the sum.  Every wait has a timeout: a hook that never
    arrives breaks the barrier, which makes the other return nonzero -- a failed test, not a hung one"""

    def __init__(self):
        self.barrier = threading.Barrier(2, timeout=60)
        self.bufs, self.total, self.errors = [None, None], None, []

    def hook(self, rank):
        def fn(user, ptr, count, stream):
            try:
                self.bufs[rank] = D.device_doubles(ptr, count, torch.device("cuda", 0))
                self.barrier.wait()
                if rank == 0:
                    self.total = self.bufs[0] + self.bufs[1]
                self.barrier.wait()
                self.bufs[rank].copy_(self.total)
                self.barrier.wait()  # nobody overwrites `total` before both have queued their copy
                return 0
            except BaseException as e:  # noqa: B902
                self.errors.append(repr(e))
                self.barrier.abort()
                return 1

        return _lib.REDUCE_FN(fn)


def run_two_ranks(params, images, shards, gf=None):
    """one engine and one Python thread per rank, one stream; rank r runs its rows of ``images`` with the global batch set
    -> per rank: dict feat, grad (with gf), stash, zstash, pooled, bstats (CPU tensors)"""
    G = images.shape[0]
    meet = Meeting()
    engines = [T.make_engine(params, max_batch=2, reserve=max(hi - lo for lo, hi in shards)) for _ in shards]
    out, failures = [None] * len(shards), []

    def work(r):
        try:
            e, (lo, hi) = engines[r], shards[r]
            img = images[lo:hi].contiguous().cuda()
            o = {"feat": e.encoder_forward_train(img, bn="batch")}
            if gf is not None:
                o["grad"] = e.encoder_backward(img, gf[lo:hi].contiguous().cuda(), bn="batch")
            out[r] = o
        except BaseException as e:  # noqa: B902
            failures.append((r, repr(e)))
            meet.barrier.abort()

    try:
        hooks = [meet.hook(r) for r in range(len(shards))]
        for e, h in zip(engines, hooks):
            e.set_encoder_reduce(h, G)
        threads = [threading.Thread(target=work, args=(r,)) for r in range(len(shards))]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=120)
        assert not any(t.is_alive() for t in threads), "a rank did not finish"
        assert not failures and not meet.errors, (failures, meet.errors)
        torch.cuda.synchronize()
        for e, o in zip(engines, out):
            o["stash"] = [e.encoder_stash(i).cpu() for i in range(N_LAYERS)]
            o["zstash"] = [e.encoder_stash_raw(i).cpu() for i in range(N_LAYERS)]
            o["pooled"], o["bstats"] = e.encoder_stash(-1).cpu(), e.encoder_batch_stats().cpu()
            o["feat"] = o["feat"].cpu()
            if gf is not None:
                o["grad"] = o["grad"].cpu()
    finally:
        for e in engines:
            e.close()
    return out


def check_statistics(ranks):
    """every rank holds the same bits, within ULP4 of the float64 statistics of the concatenated z"""
    assert all(torch.equal(r["bstats"], ranks[0]["bstats"]) for r in ranks[1:])
    worst = 0.0
    for i, (s, (om, ov)) in enumerate(zip(CONV_SPECS, ENCODER_STAT_OFFSETS)):
        z = torch.cat([r["zstash"][i] for r in ranks])
        b = ranks[0]["bstats"]
        emu, evar, _, _ = _stats_errors(b[om:om + s.cout], b[ov:ov + s.cout], z)
        worst = max(worst, emu, evar)
        assert emu <= ULP4 and evar <= ULP4, (s.name, emu, evar)
    return worst


def check_features(ranks, shards, params, images, bar=None):
    """the rule of test_forward_features: against the float64 restatement of the whole batch, 4 x the float32 restatement's error (or the
    fixed bar, valid where the float32 restatement stays below a quarter of it)"""
    ref, _ = RB.network_forward(params, images)
    f32, _ = RB.network_forward(params, images, torch.float32)
    scale = float(ref.abs().max())
    budget = float((f32.double() - ref).abs().max()) / scale
    if bar is None:
        bar = MARGIN * budget
    else:
        assert budget < bar / 4
    worst = 0.0
    for r, (lo, hi) in zip(ranks, shards):
        e = float((r["feat"].double() - ref[lo:hi]).abs().max()) / scale
        worst = max(worst, e)
        assert e < bar, (lo, hi, e, bar)
    return worst, bar


def test_two_ranks_forward_backward(params):
    """shards 1 + 1 of the G = 2 images of test_gpu_encoder_bn_train's ``whole``: the concatenated stashes drive the restatements as there"""
    images = torch.from_numpy(synthetic.make_images(2, seed=31))
    gf = torch.randn(2, 2048, generator=torch.Generator().manual_seed(3))
    shards = [(0, 1), (1, 2)]
    ranks = run_two_ranks(params, images, shards, gf)
    es = check_statistics(ranks)
    ef, fbar = check_features(ranks, shards, params, images)
    cat = lambda k: [torch.cat([r[k][i] for r in ranks]) for i in range(N_LAYERS)]  # noqa: E731
    stash, zstash, pooled = cat("stash"), cat("zstash"), torch.cat([r["pooled"] for r in ranks])
    win = R.maxpool_winners(stash[0])
    ref = RB.network_backward(params, images, zstash, stash, pooled, win, gf)
    f32 = RB.network_backward(params, images, zstash, stash, pooled, win, gf, dtype=torch.float32)
    grad = ranks[0]["grad"] + ranks[1]["grad"]  # what one SUM all-reduce of the flat tensor leaves on every rank
    worst = (0.0, None)
    for i, (s, off) in enumerate(zip(CONV_SPECS, ENCODER_PARAM_OFFSETS)):
        n = s.kh * s.kw * s.cin * s.cout + 3 * s.cout
        got, rr, ff = (R.split_layer_grad(s, t[off[0]:off[0] + n]) for t in (grad, ref, f32))
        assert float(got.pop("db").abs().max()) == 0.0
        for k in got:
            e, bar = R.rel(got[k], rr[k]), MARGIN * R.rel(ff[k], rr[k])
            if e / bar > worst[0]:
                worst = (e / bar, (s.name, k, e, bar))
            assert e < bar, (s.name, k, e, bar)
    print("two ranks 1 + 1: statistics worst %.3g (bar %.3g); features worst %.3g (bar %.3g); summed gradient, worst layer against its bar: %s"
          % (es, ULP4, ef, fbar, worst))


def test_two_ranks_own_encoder_features():
    """the fixed 2e-5 bar of test_forward_features on synthetic.py's own encoder, shards 1 + 1"""
    own = synthetic.make_encoder_params()
    images = torch.from_numpy(synthetic.make_images(2, seed=31))
    shards = [(0, 1), (1, 2)]
    ranks = run_two_ranks(own, images, shards)
    check_statistics(ranks)
    e, bar = check_features(ranks, shards, own, images, bar=FEATURE_BAR)
    print("two ranks 1 + 1, synthetic.py's own encoder: features worst %.3g (bar %.3g)" % (e, bar))


def test_two_ranks_unequal_shards(params):
    """shards 2 + 1 of G = 3, forward only: an M taken as world x local would be 4 or 2 images' rows, not 3"""
    images = torch.from_numpy(synthetic.make_images(3, seed=31))
    shards = [(0, 2), (2, 3)]
    ranks = run_two_ranks(params, images, shards)
    es = check_statistics(ranks)
    ef, bar = check_features(ranks, shards, params, images)
    print("two ranks 2 + 1: statistics worst %.3g (bar %.3g); features worst %.3g (bar %.3g)" % (es, ULP4, ef, bar))


def test_refusals(engine):
    lib, h = engine.lib, engine._h
    img = torch.from_numpy(synthetic.make_images(2, seed=31)).cuda()
    gf = torch.randn(2, 2048, generator=torch.Generator().manual_seed(3)).cuda()
    out, gflat = torch.empty(2, 2048, device="cuda"), torch.empty(resnet_spec.ENCODER_PARAM_FLOATS, device="cuda")
    plain = engine.encoder_forward_train(img, bn="batch")
    calls = []
    fail_at = [None]

    def fn(user, ptr, count, stream):
        calls.append(count)
        return 1 if fail_at[0] is not None and len(calls) == fail_at[0] + 1 else 0

    hook = _lib.REDUCE_FN(fn)
    null = _lib.REDUCE_FN()
    assert lib.hpe_encoder_set_reduce(None, hook, None, 2) == 1
    assert lib.hpe_encoder_set_reduce(h, hook, None, 0) == 1 and lib.hpe_encoder_set_reduce(h, hook, None, 65537) == 1
    assert lib.hpe_encoder_set_reduce(h, null, None, 0) == 0  # clearing takes any batch
    frozen = T.make_engine(T.make_params(), max_batch=2, reserve=1, batch_norm=False)
    try:
        assert lib.hpe_encoder_set_reduce(frozen._h, hook, None, 2) == 3  # before the batch-norm reserve
    finally:
        frozen.close()
    # the reduce buffers are part of the reserve, whose size a hook does not change
    want = {B: lib.hpe_encoder_train_ws_floats_batchnorm(B) for B in (1, 2, 3)}
    engine.set_encoder_reduce(hook, 2)
    try:
        engine.encoder_backward(img, gf, bn="batch")
        assert {B: lib.hpe_encoder_train_ws_floats_batchnorm(B) for B in want} == want
        # B above the global batch
        three = torch.zeros(3, 224, 224, 3, device="cuda")
        assert lib.hpe_encoder_forward_batchnorm(h, three.data_ptr(), 3, torch.empty(3, 2048, device="cuda").data_ptr(), engine._stream()) == 1
        # a stream in capture: refused before any launch, with or without a hook call
        n = len(calls)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                rc_f = lib.hpe_encoder_forward_batchnorm(h, img.data_ptr(), 2, out.data_ptr(), engine._stream())
                msg = lib.hpe_last_error().decode()
                rc_b = lib.hpe_encoder_backward_batchnorm(h, img.data_ptr(), 2, gf.data_ptr(), gflat.data_ptr(), engine._stream())
                out.zero_()  # the graph is not empty
        torch.cuda.current_stream().wait_stream(side)
        assert (rc_f, rc_b) == (3, 3) and "captured" in msg and len(calls) == n
        # a hook that fails at its third call: the walk stops there, the message names the layer
        third = _forward_order()[2]
        fail_at[0], n = len(calls) + 2, len(calls)
        with pytest.raises(_lib.HpeError, match=r"error 5: .*layer %d \(%s\)" % (third, CONV_SPECS[third].name)):
            engine.encoder_forward_train(img, bn="batch")
        assert len(calls) == n + 3
        fail_at[0] = None
    finally:
        engine.set_encoder_reduce(None)
    n = len(calls)
    assert torch.equal(engine.encoder_forward_train(img, bn="batch"), plain) and len(calls) == n  # cleared: the plain path, bit for bit
    # the half-layer debug calls
    s = CONV_SPECS[1]
    z = torch.zeros(1, s.hout, s.hout, s.cout, device="cuda")
    sums = torch.zeros(2, s.cout, dtype=torch.float64, device="cuda")
    st, zp, sp, M = engine._stream(), z.data_ptr(), sums.data_ptr(), s.hout * s.hout
    assert lib.hpe_debug_bn_sums(h, 53, zp, 1, sp, st) == 1 and lib.hpe_debug_bn_sums(h, 1, None, 1, sp, st) == 1
    assert lib.hpe_debug_bn_sums(h, 1, zp, 4, sp, st) == 1  # reserved for 3
    assert lib.hpe_debug_bn_finish(h, 1, sp, M - 1, zp, 1, None, 1, zp, zp, st) == 1  # M below the rows given
    assert lib.hpe_debug_bn_finish(h, 1, None, M, zp, 1, None, 1, zp, zp, st) == 1
    assert lib.hpe_debug_bn_backward_sums(h, 1, zp, None, None, 1, sp, M, sp, st) == 1
    assert lib.hpe_debug_bn_backward_finish(h, 0, zp, zp, zp, zp, 1, sp, sp, 112 * 112, zp, zp, st) == 1  # conv1 has no data gradient
    assert lib.hpe_debug_bn_backward_finish(h, 1, zp, zp, zp, zp, 1, sp, None, M, None, zp, st) == 1
