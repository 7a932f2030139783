"""NumPy restatement of the guarded optimiser step of csrc/adam.hip (DESIGN.md "Guarded optimiser step"): the gradient statistics of
hpe_grad_stats in the kernel's order, the decision and the scale of hpe_adam_guard, and g * scale feeding adam_ref.step32 as
hpe_adam_apply_guarded does.

A record is three doubles per segment: (sum of squares, largest |g| over the finite elements, number of non-finite elements).  The order
of the sum is the contract.  A segment is cut into chunks of CHUNK elements counted from its own start, the last one padded with zeros;
element e = 1024 * k + 4 * t + j of a chunk belongs to lane t (of 256) as component j of its k-th 16-byte vector.  Squares are float64
(exact).  A lane adds a vector as (x0 + x2) + (x1 + x3), then its 16 vectors by halving (k with k + 8, then + 4, + 2, + 1); the 256 lanes
are added by halving (t with t + 128, ..., + 1): one binary tree of depth log2(CHUNK) = 14.  The chunk partials of a segment are added in
index order, from 0.0.  A non-finite element's square (inf or NaN) is part of the sum; the maximum skips it and the count counts it."""
import math

import numpy as np

import adam_ref

CHUNK = 16384
LANES, VEC = 256, 4
VECS = CHUNK // (LANES * VEC)  # 16 vectors per lane and chunk
DEPTH = 14  # additions between an element's square and its chunk's partial
RECORD = 3  # doubles per segment: sum of squares, max |g| over the finite, non-finite count
GUARD_DOUBLES = 8
NORM, SCALE, APPLIED, SKIPPED, CLIPPED, NONFINITE, MAXABS, SUMSQ = range(GUARD_DOUBLES)
assert LANES * VEC * VECS == CHUNK and 2 ** DEPTH == CHUNK


def _halve(v):
    """v[i] + v[i + h] down the first axis until one row is left"""
    while v.shape[0] > 1:
        h = v.shape[0] // 2
        v = v[:h] + v[h:]
    return v[0]


def chunk_partial(x):
    """(sum of squares, max |x| over the finite, non-finite count) of one chunk of at most CHUNK float32 values, in the kernel's tree"""
    x = np.asarray(x, np.float32)
    assert 0 < x.size <= CHUNK
    d = np.zeros(CHUNK, np.float64)
    d[:x.size] = x
    with np.errstate(invalid="ignore", over="ignore"):
        a = (d * d).reshape(VECS, LANES, VEC)
        q = (a[:, :, 0] + a[:, :, 2]) + (a[:, :, 1] + a[:, :, 3])  # [VECS, LANES]
        s = _halve(_halve(q))
    fin = np.isfinite(x)
    return float(s), float(np.abs(x[fin]).max()) if fin.any() else 0.0, float(x.size - fin.sum())


def chunks_of(length):
    return (int(length) + CHUNK - 1) // CHUNK


def segment_record(x):
    """the record of one segment: its chunk partials combined in index order"""
    x = np.asarray(x, np.float32).ravel()
    s, mx, bad = 0.0, 0.0, 0.0
    with np.errstate(invalid="ignore"):
        for lo in range(0, x.size, CHUNK):
            ps, pm, pb = chunk_partial(x[lo:lo + CHUNK])
            s = float(np.float64(s) + np.float64(ps))
            mx = max(mx, pm)
            bad += pb
    return s, mx, bad


def grad_stats(g, offsets=None):
    """records [S, 3] (float64) of the flat float32 gradient g cut by the S + 1 ascending offsets (default: one segment)"""
    g = np.asarray(g, np.float32).ravel()
    offsets = [0, g.size] if offsets is None else [int(o) for o in offsets]
    return np.array([segment_record(g[a:b]) for a, b in zip(offsets[:-1], offsets[1:])], np.float64).reshape(-1, RECORD)


def sumsq_bound(length):
    """a-priori relative error bound of a segment's sum of squares against the exact sum: every term is >= 0, the squares are exact, and
    a term passes DEPTH additions inside its chunk and at most c = chunks_of(length) in the combine: 1.01 * (d + c) * 2^-53"""
    return 1.01 * (DEPTH + chunks_of(length)) * 2.0 ** -53


def exact_sumsq(x):
    return math.fsum(float(v) * float(v) for v in np.asarray(x, np.float32).ravel().astype(np.float64))


def new_state():
    return np.array([0.0, 1.0, 1.0, 0.0], np.float64)


def new_guard():
    return np.zeros(GUARD_DOUBLES, np.float64)


def guard(state, block, records, lr, beta1, beta2, clip_norm=math.inf, skip_nonfinite=False):
    """hpe_adam_guard: records is the list of the participating tensors' [S, 3] records, in tensor order.  -> (state, block), new
    arrays.  Everything float64, one rounding per operation."""
    state, block = np.array(state, np.float64), np.array(block, np.float64)
    sumsq, mx, bad = np.float64(0.0), 0.0, 0.0
    with np.errstate(invalid="ignore"):
        for rec in records:
            for s, m, b in np.asarray(rec, np.float64).reshape(-1, RECORD):
                sumsq = sumsq + np.float64(s)
                mx = max(mx, float(m))
                bad += float(b)
        norm = np.sqrt(sumsq)
    block[SUMSQ], block[NORM], block[NONFINITE], block[MAXABS] = sumsq, norm, bad, mx
    if skip_nonfinite and bad > 0:
        block[APPLIED], block[SCALE] = 0.0, 0.0
        block[SKIPPED] += 1.0
        return state, block
    t = state[0] + 1.0
    p1, p2 = adam_ref.power(beta1, int(t)), adam_ref.power(beta2, int(t))
    state[:] = (t, p1, p2, lr * math.sqrt(1.0 - p2) / (1.0 - p1))
    clip = np.float64(clip_norm)
    with np.errstate(invalid="ignore"):
        scale = np.float32(clip / norm) if norm > clip else np.float32(1.0)  # = clip / fmax(norm, clip); 1.0f for norm <= clip
    block[APPLIED], block[SCALE] = 1.0, float(scale)
    if scale < 1:
        block[CLIPPED] += 1.0
    return state, block


def apply_guarded(p, m, v, g, state, block, omb1, omb2, eps):
    """hpe_adam_apply_guarded: nothing moves when applied == 0, else step32 on g * scale (one float32 multiply)"""
    if block[APPLIED] == 0.0:
        return tuple(np.array(a, np.float32) for a in (p, m, v))
    with np.errstate(invalid="ignore", over="ignore"):
        gs = np.asarray(g, np.float32) * np.float32(block[SCALE])
        assert gs.dtype == np.float32
        return adam_ref.step32(p, m, v, gs, state[3], omb1, omb2, eps)
