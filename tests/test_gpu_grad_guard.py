"""GPU tests of the guarded optimiser step (csrc/adam.hip; run with -m gpu on an MI355X) against tests/grad_guard_ref.py:
hpe_grad_stats bit for bit at every chunk edge, alignment and table shape, and inside the a-priori bound against math.fsum; non-finite
elements; position independence; hpe_adam_guard / hpe_adam_apply_guarded against hpe_adam_advance / hpe_adam_apply and against the
restatement (no clipping, clipping, skipping, in a graph); KerasAdam, GeneratorTrainer, CriticTrainer and Trainer with the new options.

The bound: a segment's sum of squares has relative error at most 1.01 * (d + c) * 2^-53 against the exact sum (every term >= 0, squares
exact in float64, d = 14 additions inside a chunk, c = the segment's chunk partials); sums of several records add one rounding per
record, so S records of at most c chunks each are within 1.01 * (d + c + S) * 2^-53 (``bound``)."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import hpe_amd
from hpe_amd import _lib, synthetic
from hpe_amd.critic_train import CRITIC_LR
from hpe_amd.optim import layer_segments

import grad_guard_ref as G
from test_gpu_adam import B1, B2, EPS, LR, OMB1, OMB2, dev, grads, new_state, same, stream
from test_gpu_trainer import data, make_trainer, weights  # noqa: F401  (data, weights: fixtures)

pytestmark = pytest.mark.gpu
CH = G.CHUNK
SIZES = (1, 3, 4, 5, 255, 256, 257, CH - 1, CH, CH + 1, 2 * CH + 1, 100003)
U = 2.0 ** -53
INF = float("inf")


@pytest.fixture(scope="module")
def lib():
    lib = _lib.load()
    assert lib.hpe_grad_stats_chunk() == CH
    return lib


def bound(chunks, records=0):
    return 1.01 * (G.DEPTH + chunks + records) * U


def values(n, kind, seed=0):
    rng = np.random.RandomState(seed + n % 997)
    if kind == "normal":
        return rng.standard_normal(n).astype(np.float32)
    if kind == "tiny":
        return (rng.standard_normal(n) * 1e-30).astype(np.float32)
    return np.where(rng.rand(n) < 0.5, np.float32(3e38), np.float32(-3e38)).astype(np.float32)


def table_for(n):
    """many segments: length 1, lengths that are no multiple of 4, one chunk less one element, one chunk and one element, the rest"""
    cuts = [0]
    for length in (1, 3, 5, CH - 1, CH + 1):
        if cuts[-1] + length < n:
            cuts.append(cuts[-1] + length)
    return cuts + [n]


class Stats(object):
    """the device side of one hpe_grad_stats call: the table, the records and the workspace"""

    def __init__(self, lib, n, offsets=None):
        self.lib, self.n = lib, n
        self.off = np.array([0, n] if offsets is None else offsets, np.int64)
        self.S = self.off.size - 1
        self.off_dev = torch.from_numpy(self.off).cuda()
        self.rec = torch.full((self.S, G.RECORD), -1.0, dtype=torch.float64, device="cuda")
        self.bytes = lib.hpe_grad_stats_workspace_bytes(n, self.S)
        self.ws = torch.empty((self.bytes + 7) // 8, dtype=torch.int64, device="cuda")

    def run(self, g):
        assert g.numel() == self.n and g.dtype == torch.float32
        _lib.check(self.lib.hpe_grad_stats(g.data_ptr(), self.n, self.off.ctypes.data, self.off_dev.data_ptr(), self.S, self.rec.data_ptr(),
                                           self.ws.data_ptr(), self.bytes, stream()))
        return self

    def host(self):
        return self.rec.cpu().numpy()


def stats(lib, a, offsets=None, offset=0):
    return Stats(lib, a.size, offsets).run(dev(a, offset)).host()


def bits(a, b):
    """equal bits; a NaN equals a NaN (the payload of an arithmetic NaN is not part of the contract)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))))


# ---------------------------------------------------------------------------------------------- 1: statistics
@pytest.mark.parametrize("kind", ("normal", "tiny", "huge"))
@pytest.mark.parametrize("n", SIZES)
def test_statistics_equal_the_restatement(lib, n, kind):
    a = values(n, kind)
    for offsets in (None, table_for(n)):
        off = [0, n] if offsets is None else offsets
        ref = G.grad_stats(a, off)
        for shift in (0, 1):  # the pointer at a 16-byte boundary and one float past it
            got = stats(lib, a, offsets, shift)
            assert np.isfinite(got).all() and got.tobytes() == ref.tobytes(), (n, kind, shift, off, got, ref)
        for (lo, hi), (s, mx, bad) in zip(zip(off[:-1], off[1:]), got):
            exact = G.exact_sumsq(a[lo:hi])
            err, bar = abs(s - exact) / exact, bound(G.chunks_of(hi - lo))
            assert err <= bar, (n, kind, lo, hi, err, bar)
            assert mx == float(np.abs(a[lo:hi]).max()) and bad == 0.0
    print("n = %d %s: last segment's relative error %.3g, bound %.3g" % (n, kind, err, bar))


# ---------------------------------------------------------------------------------------------- 2: non-finite elements
def test_non_finite_elements_are_counted_and_stay_in_their_segment(lib):
    n = 2 * CH + 7
    off = [0, 1, 6, CH + 9, n]  # a length-1 segment; 5 elements (a scalar tail of 1); a chunk and a tail of 3; one chunk less 2
    a = values(n, "normal", 3)
    clean = {None: stats(lib, a), "table": stats(lib, a, off)}
    # alone in the length-1 segment, first / last element of a segment, inside a scalar tail, first / last element of the tensor
    places = (0, 1, 5, 6, CH + 7, CH + 8, CH + 9, n - 2, n - 1)
    for bad in (np.nan, np.inf, -np.inf):
        for at in places:
            b = a.copy()
            b[at] = bad
            for shift in (0, 1):
                for key, offsets in ((None, [0, n]), ("table", off)):
                    got = stats(lib, b, None if key is None else off, shift)
                    ref = G.grad_stats(b, offsets)
                    assert bits(got, ref), (bad, at, shift, key)
                    hit = int(np.searchsorted(offsets, at, side="right")) - 1
                    lo, hi = offsets[hit], offsets[hit + 1]
                    assert got[hit, 2] == 1.0 and not np.isfinite(got[hit, 0])
                    assert got[hit, 1] == (float(np.abs(np.delete(b[lo:hi], at - lo)).max()) if hi - lo > 1 else 0.0)
                    for s in range(len(offsets) - 1):
                        if s != hit:
                            assert got[s].tobytes() == clean[key][s].tobytes(), (bad, at, shift, s)
    b = a.copy()
    b[[0, 3, CH + 8, n - 1]] = (np.nan, np.inf, -np.inf, np.nan)
    got = stats(lib, b, off)
    assert got[:, 2].tolist() == [1.0, 1.0, 1.0, 1.0] and bits(got, G.grad_stats(b, off))
    assert stats(lib, b)[0, 2] == 4.0


# ---------------------------------------------------------------------------------------------- 3: position independence
def test_a_record_depends_on_its_segment_alone(lib):
    seg = values(CH + 5, "normal", 7)
    N = 3 * CH + 64
    want = None
    for at in (0, 3, CH + 2):
        for seed in (1, 2):
            big = values(N, "normal" if seed == 1 else "huge", 10 * seed + at)
            big[at:at + seg.size] = seg
            offsets = sorted(set([0, at, at + seg.size, N]))
            k = offsets.index(at)
            for shift in (0, 1):
                got = stats(lib, big, offsets, shift)[k]
                want = got if want is None else want
                assert got.tobytes() == want.tobytes(), (at, seed, shift)
    assert want.tobytes() == np.array(G.segment_record(seg)).tobytes() == stats(lib, seg)[0].tobytes()


# ---------------------------------------------------------------------------------------------- the guarded step, by hand
class Tensor(object):
    """p, m, v and a gradient buffer on the device (p and g each optionally one float past a 16-byte boundary), with their statistics"""

    def __init__(self, lib, p0, m0=None, v0=None, p_shift=0, g_shift=0, offsets=None):
        z = np.zeros_like(p0)
        self.p, self.m, self.v = dev(p0, p_shift), dev(z if m0 is None else m0), dev(z if v0 is None else v0)
        self.g = dev(z, g_shift)
        self.stats = Stats(lib, p0.size, offsets)

    def host(self):
        return [t.cpu().numpy() for t in (self.p, self.m, self.v)]


def new_guard():
    return torch.zeros(G.GUARD_DOUBLES, dtype=torch.float64, device="cuda")


def guarded_step(lib, tensors, state, guard, clip=INF, skip=False):
    """the launches of KerasAdam's guarded step on the gradients in the tensors' buffers"""
    for t in tensors:
        t.stats.run(t.g)
    recs = (C.c_void_p * len(tensors))(*[t.stats.rec.data_ptr() for t in tensors])
    counts = (C.c_int * len(tensors))(*[t.stats.S for t in tensors])
    _lib.check(lib.hpe_adam_guard(state.data_ptr(), guard.data_ptr(), recs, counts, len(tensors), LR, B1, B2, clip, int(skip), stream()))
    for t in tensors:
        _lib.check(lib.hpe_adam_apply_guarded(t.p.data_ptr(), t.m.data_ptr(), t.v.data_ptr(), t.g.data_ptr(), t.p.numel(), state.data_ptr(),
                                              guard.data_ptr(), float(OMB1), float(OMB2), float(np.float32(EPS)), stream()))


def plain_step(lib, tensors, state):
    _lib.check(lib.hpe_adam_advance(state.data_ptr(), LR, B1, B2, stream()))
    for t in tensors:
        _lib.check(lib.hpe_adam_apply(t.p.data_ptr(), t.m.data_ptr(), t.v.data_ptr(), t.g.data_ptr(), t.p.numel(), state.data_ptr(), float(OMB1),
                                      float(OMB2), float(np.float32(EPS)), stream()))


def set_grads(tensors, gs):
    for t, g in zip(tensors, gs):
        t.g.copy_(torch.from_numpy(g))


def restated_step(ref, gs, state, block, clip=INF, skip=False, alpha=None):
    """ref: [(p, m, v)] per tensor -> the same after one guarded step, with the restated state and guard block.  alpha: the device's
    (float64 sqrt and divide feed a float32 rounding: tests/test_gpu_adam.py gate (a) allows it one float32 ulp, so p, m, v are restated
    from the device's own alpha, as there)"""
    state, block = G.guard(state, block, [G.grad_stats(g) for g in gs], LR, B1, B2, clip, skip)
    used = np.array(state)
    if alpha is not None and block[G.APPLIED]:
        used[3] = alpha
    return [G.apply_guarded(p, m, v, g, used, block, OMB1, OMB2, EPS) for (p, m, v), g in zip(ref, gs)], state, block


def check_tensors(tensors, ref, what):
    for i, (t, want) in enumerate(zip(tensors, ref)):
        for name, a, b in zip("pmv", t.host(), want):
            assert same(a, b), (what, i, name)


def check_state(state, want):
    got = state.cpu().numpy()
    assert got[:3].tobytes() == np.asarray(want[:3]).tobytes(), (got, want)
    assert abs(got[3] - want[3]) <= np.spacing(np.float32(want[3])), (got, want)


def two(lib, n, shifts=(0, 0), seed=0):
    rng = np.random.RandomState(seed + n)
    return [Tensor(lib, rng.standard_normal(n).astype(np.float32), p_shift=shifts[0], g_shift=shifts[1]),
            Tensor(lib, rng.standard_normal(70).astype(np.float32))]


# ---------------------------------------------------------------------------------------------- 4: no clipping, nothing to skip
@pytest.mark.parametrize("shifts", ((0, 0), (1, 0), (0, 1)))
@pytest.mark.parametrize("n", (5, 4099))
def test_guarded_step_without_clipping_has_the_unguarded_bits(lib, n, shifts):
    a, b = two(lib, n, shifts), two(lib, n, shifts)
    sa, sb, guard = new_state(), new_state(), new_guard()
    for t in (1, 2, 3):
        gs = [grads(n, 30 + t), grads(70, 40 + t)]
        set_grads(a, gs)
        set_grads(b, gs)
        guarded_step(lib, a, sa, guard, skip=(t == 2))  # skip_nonfinite set or not: these gradients are finite
        plain_step(lib, b, sb)
        assert sa.cpu().numpy().tobytes() == sb.cpu().numpy().tobytes()
        check_tensors(a, [x.host() for x in b], (n, shifts, t))
        gd = guard.cpu().numpy()
        assert gd[G.SCALE] == 1.0 and gd[G.APPLIED] == 1.0 and gd[G.SKIPPED] == gd[G.CLIPPED] == gd[G.NONFINITE] == 0.0
        assert gd[G.MAXABS] == max(float(np.abs(g).max()) for g in gs)


# ---------------------------------------------------------------------------------------------- 5: clipping
def test_clipping_equals_the_restatement(lib):
    n = CH + 4099
    gs = [grads(n, 51), grads(70, 52)]
    norm = float(np.sqrt(np.float64(G.grad_stats(gs[0])[0, 0]) + np.float64(G.grad_stats(gs[1])[0, 0])))
    clipped = 0.0
    for clip in (0.5 * norm, norm, np.nextafter(norm, 0.0), 2.0 * norm, 1e-3):
        ts, state, guard = two(lib, n), new_state(), new_guard()
        ref = [t.host() for t in ts]
        set_grads(ts, gs)
        guarded_step(lib, ts, state, guard, clip=clip)
        gd, st = guard.cpu().numpy(), state.cpu().numpy()
        ref, rstate, rblock = restated_step(ref, gs, G.new_state(), G.new_guard(), clip, alpha=st[3])
        assert gd.tobytes() == rblock.tobytes(), (clip, gd, rblock)  # norm, scale, the counts, max |g|, sumsq: bit for bit
        check_state(state, rstate)
        check_tensors(ts, ref, clip)
        assert gd[G.NORM] == norm
        if clip >= norm:
            assert gd[G.SCALE] == 1.0 and gd[G.CLIPPED] == 0.0  # norm == clip_norm: exactly 1.0f, not counted
        else:
            assert gd[G.SCALE] == float(np.float32(clip / norm)) and gd[G.CLIPPED] == float(gd[G.SCALE] < 1.0)
            clipped += gd[G.CLIPPED]
    assert clipped == 2.0  # 0.5 * norm and 1e-3; one ulp below the norm rounds to 1.0f: not a clipped step


# ---------------------------------------------------------------------------------------------- 6: skipping
def test_a_non_finite_gradient_is_skipped_or_propagated(lib):
    n = 4099
    good = [[grads(n, 60 + t), grads(70, 70 + t)] for t in range(2)]
    bad = [g.copy() for g in good[0]]
    bad[1][33] = np.nan
    ts, state, guard = two(lib, n), new_state(), new_guard()
    never, nstate, nguard = two(lib, n), new_state(), new_guard()  # the run that never sees the bad gradient
    set_grads(ts, good[0])
    guarded_step(lib, ts, state, guard, clip=1.0, skip=True)
    before, sbefore = [t.host() for t in ts], state.cpu().numpy()
    set_grads(ts, bad)
    guarded_step(lib, ts, state, guard, clip=1.0, skip=True)
    gd = guard.cpu().numpy()
    assert gd[G.APPLIED] == 0.0 and gd[G.SKIPPED] == 1.0 and gd[G.NONFINITE] == 1.0 and np.isnan(gd[G.NORM]) and gd[G.CLIPPED] == 1.0
    assert state.cpu().numpy().tobytes() == sbefore.tobytes() and sbefore[0] == 1.0
    check_tensors(ts, before, "skipped")
    set_grads(ts, good[1])
    guarded_step(lib, ts, state, guard, clip=1.0, skip=True)
    for g in good:
        set_grads(never, g)
        guarded_step(lib, never, nstate, nguard, clip=1.0, skip=True)
    assert state.cpu().numpy().tobytes() == nstate.cpu().numpy().tobytes() and nstate.cpu().numpy()[0] == 2.0  # t moved once
    check_tensors(ts, [t.host() for t in never], "after the skipped step")
    assert guard.cpu().numpy()[G.SKIPPED] == 1.0 and nguard.cpu().numpy()[G.SKIPPED] == 0.0
    # skip_nonfinite off: the NaN goes through, as in TensorFlow; nothing is counted as skipped
    ts, state, guard = two(lib, n), new_state(), new_guard()
    ref = [t.host() for t in ts]
    set_grads(ts, bad)
    guarded_step(lib, ts, state, guard, clip=1.0, skip=False)
    gd = guard.cpu().numpy()
    assert gd[G.APPLIED] == 1.0 and gd[G.SKIPPED] == 0.0 and gd[G.NONFINITE] == 1.0 and gd[G.SCALE] == 1.0 and state.cpu().numpy()[0] == 1.0
    p, m, v = ts[1].host()
    assert np.isnan(p[33]) and np.isnan(m[33]) and np.isnan(v[33]) and np.isfinite(np.delete(p, 33)).all()
    ref, _, rblock = restated_step(ref, bad, G.new_state(), G.new_guard(), 1.0, alpha=state.cpu().numpy()[3])
    assert bits(gd, rblock)
    for t, want in zip(ts, ref):
        assert all(bits(a.astype(np.float64), b.astype(np.float64)) for a, b in zip(t.host(), want))


# ---------------------------------------------------------------------------------------------- 7: in a graph
def test_three_guarded_steps_in_a_graph_give_the_eager_bits(lib):
    """one stream, no parallel branches (the pattern of test_gpu_adam.py's graph test); the middle step's gradient is made non-finite by
    rewriting the gradient buffer between replays: the same graph then skips it"""
    n = 4099
    fine = [grads(n, 81), grads(70, 82)]
    nan = [fine[0].copy(), fine[1].copy()]
    nan[0][n - 2] = np.inf

    def three(ts, state, guard, mid):
        """eager: the middle step reads other buffers; captured: all three read t.g, and the replay is fed through it"""
        for i in range(3):
            if mid is not None:
                set_grads(ts, mid if i == 1 else fine)
            guarded_step(lib, ts, state, guard, clip=0.5, skip=True)

    outs = {}
    for label, mid in (("finite", fine), ("skipped", nan)):
        ts, state, guard = two(lib, n), new_state(), new_guard()
        three(ts, state, guard, mid)
        outs[label] = ([t.host() for t in ts], state.cpu().numpy(), guard.cpu().numpy())
    assert outs["finite"][1][0] == 3.0 and outs["skipped"][1][0] == 2.0 and outs["skipped"][2][G.SKIPPED] == 1.0
    # a graph of ONE guarded step, replayed three times with the gradient buffer rewritten in between
    ts, state, guard = two(lib, n), new_state(), new_guard()
    start = [t.host() for t in ts]
    set_grads(ts, fine)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        guarded_step(lib, ts, state, guard, clip=0.5, skip=True)
    check_tensors(ts, start, "a capture runs nothing")
    assert state.cpu().numpy()[0] == 0.0
    for i in range(3):
        set_grads(ts, nan if i == 1 else fine)
        graph.replay()
    torch.cuda.synchronize()
    want = outs["skipped"]
    check_tensors(ts, want[0], "replayed")
    assert state.cpu().numpy().tobytes() == want[1].tobytes() and bits(guard.cpu().numpy(), want[2])
    # and three steps captured in one graph give the eager bits of three finite steps
    ts, state, guard = two(lib, n), new_state(), new_guard()
    set_grads(ts, fine)
    torch.cuda.synchronize()
    graph3 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph3):
        three(ts, state, guard, None)
    graph3.replay()
    torch.cuda.synchronize()
    want = outs["finite"]
    check_tensors(ts, want[0], "three in one graph")
    assert state.cpu().numpy().tobytes() == want[1].tobytes() and guard.cpu().numpy().tobytes() == want[2].tobytes()


# ---------------------------------------------------------------------------------------------- 8: KerasAdam
def test_keras_adam_guarded(lib):
    rng = np.random.RandomState(90)
    a0, b0 = rng.standard_normal(2 * CH + 13).astype(np.float32), rng.standard_normal(70).astype(np.float32)
    ga, gb = grads(a0.size, 91), grads(b0.size, 92)
    cuts = [0, 7, CH + 8, a0.size]
    opt = hpe_amd.KerasAdam(LR, B1, B2, EPS, global_clipnorm=1.0, skip_nonfinite=True)
    a = opt.add("a", torch.from_numpy(a0.copy()).cuda(), segments=cuts)
    b = opt.add("b", torch.from_numpy(b0.copy()).cuda())
    with pytest.raises(ValueError):
        opt.add("c", torch.zeros(8, device="cuda"), segments=[0, 5, 4, 8])
    a.grad, b.grad = torch.from_numpy(ga).cuda(), torch.from_numpy(gb).cuda()
    opt.step()
    ra, rb = G.grad_stats(ga, cuts), G.grad_stats(gb)
    assert opt.grad_stats("a").cpu().numpy().tobytes() == ra.tobytes() and opt.grad_stats("b").cpu().numpy().tobytes() == rb.tobytes()
    st, gd = G.guard(G.new_state(), G.new_guard(), [ra, rb], LR, B1, B2, 1.0, True)
    assert opt._guard.cpu().numpy().tobytes() == gd.tobytes()
    assert opt.grad_norm.is_cuda and opt.grad_norm.dim() == 0 and float(opt.grad_norm) == gd[G.NORM] and float(opt.step_applied) == 1.0
    assert float(opt.clip_scale) == gd[G.SCALE] < 1.0 and (opt.iterations, opt.clipped_steps, opt.skipped_steps) == (1, 1, 0)
    alpha = opt._state.cpu().numpy()[3]
    used = np.array([st[0], st[1], st[2], alpha])
    for ten, slot, x0, g in ((a, opt.slots["a"], a0, ga), (b, opt.slots["b"], b0, gb)):
        p, m, v = G.apply_guarded(x0, np.zeros_like(x0), np.zeros_like(x0), g, used, gd, OMB1, OMB2, EPS)
        assert same(ten.detach().cpu().numpy(), p) and same(slot["m"].cpu().numpy(), m) and same(slot["v"].cpu().numpy(), v)
    # the segments' records against the whole tensor's: the count and the maximum exactly, the sum of squares to rounding -- two
    # segmentations add in different orders, so bit equality across them is not promised
    whole = stats(lib, ga)[0]
    assert ra[:, 2].sum() == whole[2] and ra[:, 1].max() == whole[1]
    assert abs(math.fsum(ra[:, 0]) - whole[0]) <= 2 * bound(G.chunks_of(ga.size), len(cuts)) * whole[0]
    # only=: the norm is that of the tensors stepped; b, its moments and its records stay
    keep = [b.detach().clone(), opt.slots["b"]["m"].clone(), opt.slots["b"]["v"].clone()]
    a.grad = torch.from_numpy(grads(a0.size, 93)).cuda()
    opt.step(only=("a",))
    st2, gd2 = G.guard(st, gd, [G.grad_stats(grads(a0.size, 93), cuts)], LR, B1, B2, 1.0, True)
    assert opt._guard.cpu().numpy().tobytes() == gd2.tobytes() and opt.iterations == 2
    assert same(b.detach().cpu().numpy(), keep[0].cpu().numpy()) and torch.equal(opt.slots["b"]["m"], keep[1]) and torch.equal(opt.slots["b"]["v"], keep[2])
    # a NaN in b: the whole step is skipped
    snap = [a.detach().clone(), opt.slots["a"]["m"].clone(), opt._state.clone()]
    b.grad = torch.from_numpy(np.where(np.arange(70) == 69, np.nan, gb).astype(np.float32)).cuda()
    opt.step()
    assert float(opt.step_applied) == 0.0 and (opt.iterations, opt.skipped_steps) == (2, 1)
    assert torch.equal(a.detach(), snap[0]) and torch.equal(opt.slots["a"]["m"], snap[1]) and torch.equal(opt._state, snap[2])
    assert set(opt.state_dict()) == {"iterations", "learning_rate", "beta_1", "beta_2", "epsilon", "slots"}  # the checkpoint layout is as it was
    plain = hpe_amd.KerasAdam(LR)
    plain.add("a", torch.zeros(8, device="cuda"))
    with pytest.raises(RuntimeError):
        plain.grad_norm
    with pytest.raises(KeyError):
        plain.grad_stats("a")


# ---------------------------------------------------------------------------------------------- 9: the two trainers
def exact_sumsq_dev(t):
    """sum of squares of a float32 CUDA tensor, exact to far below 2^-53: float64 squares (exact) summed in 80-bit long double, pairwise"""
    assert np.finfo(np.longdouble).nmant >= 63
    x = t.detach().cpu().numpy().astype(np.float64).ravel()
    total = np.longdouble(0.0)
    for lo in range(0, x.size, 1 << 22):
        part = x[lo:lo + (1 << 22)]
        total += np.sum((part * part).astype(np.longdouble))
    return total


def norm_error(reported, tensors):
    """|reported^2 - exact| / exact, reported the float64 norm of the guard block: one sqrt and one square more than the sum"""
    exact = sum(exact_sumsq_dev(t) for t in tensors)
    return float(abs(np.longdouble(float(reported)) ** 2 - exact) / exact)


def table_bound(tables, extra=4):
    """the bound of a sum over whole tables: the most chunks any segment has, one rounding per record, and `extra` roundings for the
    square root and the test's own squaring"""
    chunks = max(G.chunks_of(b - a) for off in tables for a, b in zip(off[:-1], off[1:]))
    return bound(chunks, sum(len(off) - 1 for off in tables) + extra)


@pytest.fixture(scope="module")
def engine():
    from oracle import hmr_oracle as O

    e = hpe_amd.HpeEngine(device=0, max_batch=4)
    e.load_smpl(synthetic.make_smpl_model())
    e.load_encoder(synthetic.make_encoder_params())
    e.load_regressor(synthetic.make_regressor_params(variant="bounded"))
    e.load_mean_theta(O.load_mean_param(synthetic.make_mean_params()))
    e.load_critic(synthetic.make_critic_params())
    e.finalize()
    e.reserve_encoder_train(2, batch_norm=True)
    e.reserve_encoder_train(2, batch_norm=True, precision="mixed")
    yield e
    e.close()


def tbits(x, y):
    as_int = {torch.float32: torch.int32, torch.float64: torch.int64}
    return torch.equal(x.contiguous().view(as_int[x.dtype]), y.contiguous().view(as_int[y.dtype]))


def generator_state(tr):
    o = tr.optimizer
    return [tr.params.detach().clone(), tr.encoder_params.detach().clone(), tr.encoder_stats.clone(), o._state.clone()] + \
        [o.slots[k][s].clone() for k in ("regressor", "encoder") for s in ("m", "v")]


@pytest.mark.parametrize("precision", ("fp32", "mixed"))
def test_generator_trainer_skips_and_clips(engine, precision):
    e = engine
    img = torch.from_numpy(synthetic.make_images(2, seed=13)).cuda()
    g = torch.Generator().manual_seed(4)
    kp = torch.cat([torch.rand(2, 19, 2, generator=g) * 1.2 - 0.6, torch.ones(2, 19, 1)], 2).cuda()
    kw = dict(dropout=0.5, generator=torch.Generator(device="cuda").manual_seed(1), train_encoder=True, encoder_bn="batch", optimizer="keras",
              encoder_precision=precision)
    with pytest.raises(ValueError):
        hpe_amd.GeneratorTrainer(e, skip_nonfinite=True)  # optimizer="torch"
    tr = hpe_amd.GeneratorTrainer(e, skip_nonfinite=True, **kw)
    masks = tr.draw_masks(2)
    r = tr.step(img, kp, use_critic=False, drop=masks)  # a finite step first: the moments are no longer zeros
    assert float(r["step_applied"]) == 1.0 and tr.optimizer.iterations == 1 and float(r["grad_norm"]) > 0
    before = generator_state(tr)
    predict = {k: v.clone() for k, v in e.forward(img)[0].items()}
    bad = kp.clone()
    bad[1, 3, 0] = float("nan")  # one visible joint's x
    r = tr.step(img, bad, use_critic=False, drop=masks)
    assert all(bool(torch.isfinite(t).all()) for t in r["thetas"]) and bool(torch.isfinite(r["pred_keypoints"]).all())  # the forward is finite
    assert bool(torch.isnan(tr.params.grad).any()) and bool(torch.isnan(tr.encoder_params.grad).any())  # the cotangents are not
    assert float(r["step_applied"]) == 0.0 and tr.optimizer.iterations == 1 and tr.optimizer.skipped_steps == 1
    assert all(tbits(x, y) for x, y in zip(before, generator_state(tr)))
    assert torch.equal(e.encoder_params(), before[1]) and torch.equal(e.encoder_stats(), before[2]) and torch.equal(e.regressor_params(), before[0])
    after = e.forward(img)[0]
    assert set(after) == set(predict) and all(torch.equal(after[k], predict[k]) for k in predict)
    # the same step with a finite kp_gt under clipnorm = 1e-3, from the engine as it stands (the skipped step left it alone)
    tr = hpe_amd.GeneratorTrainer(e, clipnorm=1e-3, **kw)
    p0, q0, s0 = tr.params.detach().cpu().numpy(), tr.encoder_params.detach().cpu().numpy(), tr.encoder_stats.clone()
    r = tr.step(img, kp, use_critic=False, drop=masks)
    tables = [layer_segments("regressor")[0], layer_segments("encoder")[0]]
    err, bar = norm_error(r["grad_norm"], (tr.params.grad, tr.encoder_params.grad)), table_bound(tables)
    print("generator %s: grad_norm %.6g, relative error of its square %.3g, bound %.3g" % (precision, float(r["grad_norm"]), err, bar))
    assert err <= bar
    gr, ge = tr.params.grad.cpu().numpy(), tr.encoder_params.grad.cpu().numpy()
    st, gd = G.guard(G.new_state(), G.new_guard(), [G.grad_stats(gr, tables[0]), G.grad_stats(ge, tables[1])], LR, B1, B2, 1e-3, False)
    assert tr.optimizer._guard.cpu().numpy().tobytes() == gd.tobytes() and gd[G.SCALE] < 1.0 and float(r["step_applied"]) == 1.0
    assert tr.optimizer.clipped_steps == 1 and float(r["grad_norm"]) == gd[G.NORM]
    used = np.array(st)
    used[3] = tr.optimizer._state.cpu().numpy()[3]
    for ten, x0, gx, name in ((tr.params, p0, gr, "regressor"), (tr.encoder_params, q0, ge, "encoder")):
        p, m, v = G.apply_guarded(x0, np.zeros_like(x0), np.zeros_like(x0), gx, used, gd, OMB1, OMB2, EPS)
        assert same(ten.detach().cpu().numpy(), p), name
        assert same(tr.optimizer.slots[name]["m"].cpu().numpy(), m) and same(tr.optimizer.slots[name]["v"].cpu().numpy(), v), name
    assert not torch.equal(tr.encoder_stats, s0) and torch.equal(e.encoder_stats(), tr.encoder_stats)  # an applied step moves the statistics


def test_critic_trainer_skips_and_clips(engine):
    e = engine
    N = 4
    real_th = torch.from_numpy(synthetic.make_thetas(N, seed=31)).cuda()
    fake_th = torch.from_numpy(synthetic.make_thetas(N, seed=32)).cuda()
    o = e.smpl(real_th, want=("joints", "Rs"))
    real = (o["joints"].clone(), real_th[:, 75:].contiguous(), o["Rs"].clone())
    g = torch.Generator().manual_seed(33)
    interp = tuple(torch.rand(shape, generator=g).cuda() for shape in ((N, 14, 3), (N, 10), (N, 24, 3, 3)))
    with pytest.raises(ValueError):
        hpe_amd.CriticTrainer(e, clipnorm=1.0)  # optimizer="torch"
    tr = hpe_amd.CriticTrainer(e, optimizer="keras", skip_nonfinite=True)
    r = tr.step_from_thetas(real, [fake_th], interp=interp)
    assert float(r["step_applied"]) == 1.0 and tr.optimizer.iterations == 1
    opt = tr.optimizer
    before = [tr.params.clone(), opt.slots["critic"]["m"].clone(), opt.slots["critic"]["v"].clone(), opt._state.clone()]
    bad = (real[0].clone(), real[1], real[2])
    bad[0][2, 5, 1] = float("nan")
    r = tr.step_from_thetas(bad, [fake_th], interp=interp)
    assert float(r["step_applied"]) == 0.0 and opt.iterations == 1 and opt.skipped_steps == 1 and bool(torch.isnan(tr.params.grad).any())
    now = [tr.params, opt.slots["critic"]["m"], opt.slots["critic"]["v"], opt._state]
    assert all(tbits(x, y) for x, y in zip(before, now)) and torch.equal(e.critic_params(), before[0])
    tr = hpe_amd.CriticTrainer(e, optimizer="keras", clipnorm=1e-3)
    p0 = tr.params.cpu().numpy()
    r = tr.step_from_thetas(real, [fake_th], interp=interp)
    table = layer_segments("critic")[0]
    err, bar = norm_error(r["grad_norm"], (tr.params.grad,)), table_bound([table])
    print("critic: grad_norm %.6g, relative error of its square %.3g, bound %.3g" % (float(r["grad_norm"]), err, bar))
    assert err <= bar
    gc = tr.params.grad.cpu().numpy()
    st, gd = G.guard(G.new_state(), G.new_guard(), [G.grad_stats(gc, table)], CRITIC_LR, B1, B2, 1e-3, False)
    assert tr.optimizer._guard.cpu().numpy().tobytes() == gd.tobytes() and gd[G.SCALE] < 1.0
    used = np.array(st)
    used[3] = tr.optimizer._state.cpu().numpy()[3]
    p, m, v = G.apply_guarded(p0, np.zeros_like(p0), np.zeros_like(p0), gc, used, gd, OMB1, OMB2, EPS)
    assert same(tr.params.cpu().numpy(), p) and same(tr.optimizer.slots["critic"]["m"].cpu().numpy(), m)
    assert same(tr.optimizer.slots["critic"]["v"].cpu().numpy(), v) and torch.equal(e.critic_params(), tr.params)


# ---------------------------------------------------------------------------------------------- 10: Trainer
def test_trainer_writes_the_optimiser_scalars(weights, data, tmp_path):  # noqa: F811
    """the pattern of tests/test_gpu_summaries.py: one epoch of two steps on the four records, summaries on, no image step"""
    model_dir = str(tmp_path / "model")
    tr = make_trainer(weights, data, tmp_path / "ckpt", epoch=1, model_dir=model_dir, log_img_step=0, generator_clipnorm=1e-3, log_grad_norms=True)
    try:
        results, step = [], tr.train_step
        tr.train_step = lambda *a, **k: results.append(step(*a, **k)) or results[-1]
        assert tr.train(save_every=100)["steps"] == 2
        assert tr.generator.guarded and tr.critic.guarded and tr.generator.optimizer.global_clipnorm == 1e-3
        assert tr.critic.optimizer.global_clipnorm == INF  # logging alone: a guard that never clips
        assert (tr.generator.optimizer.clipped_steps, tr.critic.optimizer.clipped_steps) == (2, 0)
    finally:
        tr.engine.close()
    files = os.listdir(os.path.join(model_dir, "training"))
    assert len(files) == 1
    ev = [(e["step"], e["values"][0]["tag"], e["values"][0]["simple_value"]) for e in hpe_amd.read_events(os.path.join(model_dir, "training", files[0]))[1:]]
    optim_tags = ["optim/%s_%s" % (who, what) for who in ("generator", "critic") for what in ("grad_norm", "clip_scale", "skipped_steps")]
    gen_layers = list(dict.fromkeys(layer_segments("regressor")[1] + layer_segments("encoder")[1]))
    critic_layers = list(dict.fromkeys(layer_segments("critic")[1]))
    assert len(gen_layers) == 4 + 53 and len(critic_layers) == 9
    tables = {"generator": [layer_segments("regressor")[0], layer_segments("encoder")[0]], "critic": [layer_segments("critic")[0]]}
    for s in (1, 2):
        got = {t: v for st, t, v in ev if st == s}
        r = results[s - 1]
        assert [t for st, t, _ in ev if st == s and t.startswith("optim/")] == optim_tags
        assert sorted(t for t in got if t.startswith("grad_norm/")) == sorted("grad_norm/" + n for n in gen_layers + critic_layers)
        for tag in optim_tags:
            assert got[tag] == float(np.float32(float(r[tag[len("optim/"):]]))), (s, tag)
        assert got["optim/generator_clip_scale"] < 1.0 and got["optim/critic_clip_scale"] == 1.0 and got["optim/generator_skipped_steps"] == 0.0
        for who, layers in (("generator", gen_layers), ("critic", critic_layers)):
            for n in layers:
                assert got["grad_norm/" + n] == float(np.float32(float(r["layer_grad_norms"][n]))), (s, n)
            # a layer's square: its records added, one sqrt, squared again here; the global one: all records added in order, one sqrt,
            # squared here: both within the table's bound of the exact sum
            total = math.fsum(float(r["layer_grad_norms"][n]) ** 2 for n in layers)
            whole = float(r[who + "_grad_norm"]) ** 2
            assert abs(total - whole) <= 2 * table_bound(tables[who]) * whole, (s, who, total, whole)
