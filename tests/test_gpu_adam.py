"""GPU tests of the fused optimiser update (csrc/adam.hip; run with -m gpu on an MI355X) against tests/adam_ref.py.

Gates, per size, alignment and step:
  (a) alpha read back from the device is within one float32 ulp of the float64 Python value; the two powers equal Python's
      square-and-multiply loop exactly (two double multiplies per bit, nothing to contract);
  (b) p, m and v equal, bit for bit, the NumPy float32 restatement fed the device's alpha;
  (c) each of m, v and the update p_new - p_old has a norm-relative error against float64 of at most 4 x the float32 restatement's
      (the project's usual bar; with (b) holding the two are equal);
  (d) the misaligned (all-scalar) launches and the scalar tail give the bits of the aligned vector path for the same elements.
Gradients are normal draws at the scales 1e-6, 1 and 1e3 mixed in one tensor."""
import ctypes as C

import numpy as np
import pytest
import torch

import hpe_amd
from hpe_amd import _lib

import adam_ref as R

pytestmark = pytest.mark.gpu
LR, B1, B2, EPS = 1e-4, 0.9, 0.999, 1e-7
OMB1, OMB2 = R.one_minus(B1), R.one_minus(B2)
SIZES = (1, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025, 8 * 2 ** 20 + 3)
ALIGNMENTS = ("aligned", "p+1", "g+1")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(a, offset=0):
    """a device copy of the float32 array whose first element sits `offset` floats past a 16-byte boundary"""
    buf = torch.empty(a.size + 4, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    t = buf[offset:offset + a.size]
    t.copy_(torch.from_numpy(a))
    return t


def new_state():
    return torch.tensor([0.0, 1.0, 1.0, 0.0], dtype=torch.float64, device="cuda")


def advance(lib, state):
    """one hpe_adam_advance -> (t, beta1^t, beta2^t, alpha) as read back"""
    _lib.check(lib.hpe_adam_advance(state.data_ptr(), LR, B1, B2, stream()))
    return state.cpu().numpy()


def apply(lib, p, m, v, g, state, eps=EPS):
    _lib.check(lib.hpe_adam_apply(p.data_ptr(), m.data_ptr(), v.data_ptr(), g.data_ptr(), p.numel(), state.data_ptr(), float(OMB1), float(OMB2),
                                  float(np.float32(eps)), stream()))


def check_state(st, t):
    assert st[0] == t and st[1] == R.power(B1, t) and st[2] == R.power(B2, t), st
    want = R.alpha64(LR, B1, B2, t)
    assert abs(st[3] - want) <= np.spacing(np.float32(want)), (st[3], want)


def grads(n, seed):
    rng = np.random.RandomState(seed)
    return (rng.standard_normal(n) * rng.choice([1e-6, 1.0, 1e3], n)).astype(np.float32)


def same(a, b):
    return np.array_equal(np.asarray(a).view(np.int32), np.asarray(b).view(np.int32))


WORST = {"m": (0.0, 0.0), "v": (0.0, 0.0), "update": (0.0, 0.0)}


def gate_c(what, got, ref32, ref64):
    e, bar = R.rel_err(got, ref64), 4.0 * R.rel_err(ref32, ref64)
    if e >= WORST[what][0]:
        WORST[what] = (e, bar)
    assert e <= bar, (what, e, bar)


def run_steps(lib, n, ts, start=None, seed=0):
    """the steps `ts` (consecutive) from zero moments (or, after hpe_adam_set_step(start), from drawn ones) on all three alignments"""
    rng = np.random.RandomState(seed + n % 1000)
    p0 = rng.standard_normal(n).astype(np.float32)
    if start is None:
        m0 = v0 = np.zeros(n, np.float32)
    else:
        m0 = (rng.standard_normal(n) * 0.1).astype(np.float32)
        v0 = (rng.standard_normal(n) ** 2).astype(np.float32)
    gs = [grads(n, 100 + seed + t % 1000) for t in ts]
    runs = []
    for al in ALIGNMENTS:
        p, m, v = dev(p0, 1 if al == "p+1" else 0), dev(m0), dev(v0)
        state = new_state()
        if start is not None:
            _lib.check(lib.hpe_adam_set_step(state.data_ptr(), start, B1, B2, stream()))
            st = state.cpu().numpy()
            assert st[0] == start and st[1] == R.power(B1, start) and st[2] == R.power(B2, start) and st[3] == 0.0
        per_step = []
        for t, g in zip(ts, gs):
            gd = dev(g, 1 if al == "g+1" else 0)
            st = advance(lib, state)
            check_state(st, t)  # (a)
            apply(lib, p, m, v, gd, state)
            per_step.append((st[3], p.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy()))
        runs.append(per_step)
    # the restatements, once: fed the device's alpha (equal on all alignments: the same launch sequence)
    p32, m32, v32 = p0, m0, v0
    p64, m64, v64 = (a.astype(np.float64) for a in (p0, m0, v0))
    for i, (t, g) in enumerate(zip(ts, gs)):
        alpha = runs[0][i][0]
        assert all(r[i][0] == alpha for r in runs)
        q32, m32, v32 = R.step32(p32, m32, v32, g, alpha, OMB1, OMB2, EPS)
        q64, m64, v64 = R.step64(p32, m64, v64, g, R.alpha64(LR, B1, B2, t), OMB1, OMB2, EPS)
        for al, r in zip(ALIGNMENTS, runs):
            _a, pg, mg, vg = r[i]
            assert same(pg, q32) and same(mg, m32) and same(vg, v32), (n, t, al)  # (b), and with it (d)
            if al != ALIGNMENTS[0]:
                continue  # the same bits as the aligned run: (c) would measure the same numbers again
            gate_c("m", mg, m32, m64)
            gate_c("v", vg, v32, v64)
            gate_c("update", pg.astype(np.float64) - p32, q32.astype(np.float64) - p32, q64 - p32)
        p32 = q32
        m64, v64 = m32.astype(np.float64), v32.astype(np.float64)  # each step is judged on the same inputs


@pytest.mark.parametrize("n", SIZES)
def test_first_three_steps(lib, n):
    run_steps(lib, n, (1, 2, 3))
    print("n = %d: worst (error, bar) so far: %s" % (n, WORST))


@pytest.mark.parametrize("start", (999, 10 ** 6))
@pytest.mark.parametrize("n", (5, 1025))
def test_resumed_step(lib, n, start):
    """after hpe_adam_set_step both powers are near 0 (10^6: beta1^t underflows to 0) and alpha is near lr"""
    run_steps(lib, n, (start + 1,), start=start, seed=7)


def test_position_and_path_do_not_matter(lib):
    """the same values as elements 0..1022 of an n = 1023 launch (three of them in the scalar tail), of an n = 1025 launch (all of them
    in vectors) and at another offset of a longer tensor give the same bits"""
    n = 1025
    rng = np.random.RandomState(11)
    p0, m0, v0 = rng.standard_normal(n).astype(np.float32), (rng.standard_normal(n) * 0.1).astype(np.float32), (rng.standard_normal(n) ** 2).astype(np.float32)
    g = grads(n, 12)
    state = new_state()
    advance(lib, state)
    outs = []
    for k in (1023, 1025):
        p, m, v, gd = dev(p0[:k]), dev(m0[:k]), dev(v0[:k]), dev(g[:k])
        apply(lib, p, m, v, gd, state)
        outs.append([t.cpu().numpy() for t in (p, m, v)])
    shift = 4 * 300 + 2  # the same values further along a tensor of 4096 + 1 elements
    big = [np.zeros(4097, np.float32) for _ in range(4)]
    for b, a in zip(big, (p0, m0, v0, g)):
        b[shift:shift + n] = a
    p, m, v, gd = (dev(b) for b in big)
    apply(lib, p, m, v, gd, state)
    moved = [t.cpu().numpy()[shift:shift + n] for t in (p, m, v)]
    for a, b, c in zip(outs[0], outs[1], moved):
        assert same(a, b[:1023]) and same(b, c)


def test_zero_gradient_leaves_p_alone_and_subnormal_squares_survive(lib):
    n = 1027
    p0 = np.random.RandomState(13).standard_normal(n).astype(np.float32)
    z = np.zeros(n, np.float32)
    state = new_state()
    alpha = advance(lib, state)[3]
    p, m, v = dev(p0), dev(z), dev(z)
    apply(lib, p, m, v, dev(z), state)
    assert same(p.cpu().numpy(), p0) and not m.any().item() and not v.any().item()
    # g = 1e-20: g * g = 1e-40 and v = 1e-43 are subnormal floats; a flush to zero anywhere changes v's bits
    g = np.full(n, 1e-20, np.float32)
    p, m, v = dev(p0), dev(z), dev(z)
    apply(lib, p, m, v, dev(g), state)
    q32, m32, v32 = R.step32(p0, z, z, g, alpha, OMB1, OMB2, EPS)
    assert v32[0] > 0 and v32[0] < np.finfo(np.float32).tiny
    assert same(p.cpu().numpy(), q32) and same(m.cpu().numpy(), m32) and same(v.cpu().numpy(), v32)


def test_three_steps_in_a_graph_give_the_eager_bits(lib):
    n = 4099
    rng = np.random.RandomState(17)
    p0 = rng.standard_normal(n).astype(np.float32)
    z = np.zeros(n, np.float32)
    g = dev(grads(n, 18))

    def three(p, m, v, state):
        for _ in range(3):
            _lib.check(lib.hpe_adam_advance(state.data_ptr(), LR, B1, B2, stream()))
            apply(lib, p, m, v, g, state)

    pe, me, ve, se = dev(p0), dev(z), dev(z), new_state()
    three(pe, me, ve, se)
    pg, mg, vg, sg = dev(p0), dev(z), dev(z), new_state()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        three(pg, mg, vg, sg)
    assert same(pg.cpu().numpy(), p0) and sg.cpu().numpy()[0] == 0.0  # a capture runs nothing
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(se, sg) and se[0].item() == 3.0
    for a, b in ((pe, pg), (me, mg), (ve, vg)):
        assert same(a.cpu().numpy(), b.cpu().numpy())


def test_refusals(lib):
    t = torch.zeros(8, dtype=torch.float32, device="cuda")
    st = new_state()
    before = t.clone()
    for args in ((None, t, t, t, 8, st), (t, None, t, t, 8, st), (t, t, None, t, 8, st), (t, t, t, None, 8, st), (t, t, t, t, 8, None),
                 (t, t, t, t, -1, st)):
        ptrs = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args]
        with pytest.raises(hpe_amd.HpeError):
            _lib.check(lib.hpe_adam_apply(ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[4], ptrs[5], float(OMB1), float(OMB2), EPS, stream()))
    _lib.check(lib.hpe_adam_apply(t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), 0, st.data_ptr(), float(OMB1), float(OMB2), EPS, stream()))
    with pytest.raises(hpe_amd.HpeError):
        _lib.check(lib.hpe_adam_advance(None, LR, B1, B2, stream()))
    with pytest.raises(hpe_amd.HpeError):
        _lib.check(lib.hpe_adam_set_step(st.data_ptr(), -1, B1, B2, stream()))
    torch.cuda.synchronize()
    assert torch.equal(t, before) and st.cpu().numpy().tolist() == [0.0, 1.0, 1.0, 0.0]


# ---------------------------------------------------------------------------------------------- KerasAdam
def _two_tensors(seed=21):
    rng = np.random.RandomState(seed)
    return rng.standard_normal(1025).astype(np.float32), rng.standard_normal(70).astype(np.float32)


def _opt(a0, b0):
    opt = hpe_amd.KerasAdam(LR, B1, B2, EPS)
    a = opt.add("a", torch.from_numpy(a0.copy()).cuda())
    b = opt.add("b", torch.from_numpy(b0.copy()).cuda())
    return opt, a, b


def test_keras_adam_two_tensors_share_one_step_count():
    a0, b0 = _two_tensors()
    opt, a, b = _opt(a0, b0)
    ref = {"a": (a0, np.zeros_like(a0), np.zeros_like(a0)), "b": (b0, np.zeros_like(b0), np.zeros_like(b0))}
    for t in (1, 2):
        gs = {"a": grads(a0.size, 30 + t), "b": grads(b0.size, 40 + t)}
        a.grad, b.grad = torch.from_numpy(gs["a"]).cuda(), torch.from_numpy(gs["b"]).cuda()
        opt.step()
        assert opt.iterations == t
        alpha = opt._state.cpu().numpy()[3]
        assert abs(alpha - R.alpha64(LR, B1, B2, t)) <= np.spacing(np.float32(alpha))
        for k, ten in (("a", a), ("b", b)):
            ref[k] = R.step32(*ref[k], gs[k], alpha, OMB1, OMB2, EPS)
            assert same(ten.cpu().numpy(), ref[k][0])
            assert same(opt.slots[k]["m"].cpu().numpy(), ref[k][1]) and same(opt.slots[k]["v"].cpu().numpy(), ref[k][2])
    a.grad = None
    with pytest.raises(RuntimeError):
        opt.step()
    assert opt.iterations == 2


def test_keras_adam_state_dict_resumes_bit_for_bit():
    a0, b0 = _two_tensors(22)
    opt, a, b = _opt(a0, b0)
    gs = [(torch.from_numpy(grads(a0.size, 50 + t)).cuda(), torch.from_numpy(grads(b0.size, 60 + t)).cuda()) for t in range(4)]
    for ga, gb in gs[:3]:
        a.grad, b.grad = ga, gb
        opt.step()
    sd = opt.state_dict()
    assert sd["iterations"] == 3 and set(sd["slots"]) == {"a", "b"}
    fresh, a2, b2 = _opt(a.detach().cpu().numpy(), b.detach().cpu().numpy())
    fresh.load_state_dict(sd)
    assert fresh.iterations == 3
    for o, x, y in ((opt, a, b), (fresh, a2, b2)):
        x.grad, y.grad = gs[3]
        o.step()
    assert torch.equal(opt._state, fresh._state) and fresh.iterations == 4
    assert same(a.cpu().numpy(), a2.cpu().numpy()) and same(b.cpu().numpy(), b2.cpu().numpy())
    for k in ("a", "b"):
        for s in ("m", "v"):
            assert same(opt.slots[k][s].cpu().numpy(), fresh.slots[k][s].cpu().numpy())
