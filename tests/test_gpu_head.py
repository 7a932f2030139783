"""GPU tests of the head after the encoder -- average pool, the three Dense layers of the iterative regressor, the SMPL forward
pass, the keypoint regressor and its projection -- at every batch size where the library switches kernels, against the CPU oracle
evaluated in FLOAT64 on the same float32 inputs.

Dispatch forms covered (human-pose-estimation_amd/csrc):
  run_dense           M <= 2 dense_gemv_kernel<2>, M = 3, 4 dense_gemv_kernel<4>, M >= 5 the 64x64 dense GEMM (M = 64 / 65: tile edge)
  hpe_launch_smpl     B <= 8 smpl_skin_small_kernel + smpl_kp_finish_kernel, above it smpl_skin_kernel (8 images per thread, partial
                      tiles at B = 9 ... 15) + joint_regress_kernel; every combination of requested outputs that changes a launch
  hpe_launch_avgpool  B <= 16 avgpool_small_kernel (lane guard of a partial last group), above it avgpool_kernel
  hpe_tail            SMPL on theta rows of stride THETA_LD (hpe_smpl: 85)

Metric: rel of test_gpu_parity.py, max|a - b| / max|b|, taken PER IMAGE (the maximum over the batch of the per-row value), so that
a wrong row of small magnitude cannot hide behind a large one.  Bars: the project's single-kernel bars (BARS, REG_BAR, POOL_BAR),
applied against float64; the float32 oracle sits under a quarter of each in this metric on these inputs
(tests/test_head_inputs_cpu.py), which leaves room for another summation order and none for a wrong term.

Every test prints the errors it measured (pytest -s); DESIGN.md section 2, "Head coverage", lists the worst per output.
"""
import ctypes as C
import math

import numpy as np
import pytest

import hpe_amd
from hpe_amd import _lib, synthetic
from oracle import hmr_oracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-4  # the full-path bar of test_gpu_parity.py: chained stages (hpe_tail)
BARS = {"Rs": 2e-6, "J_transformed": 5e-6, "verts": 1e-5, "joints": 1e-5, "kp2d": 1e-5, "verts2d": 1e-5}
REG_BAR = 5e-6
POOL_BAR = 1e-6
ALL_OUTPUTS = _lib.OUTPUT_FIELDS  # verts, joints, cams, theta, J_transformed, kp2d, verts2d, Rs
MAX_BATCH = 72
SENTINEL = 12345.678  # finite, far from every output value
IM_SIZE = np.array([224.0, 224.0])


# ------------------------------------------------------------------------------------------- inputs (CPU only: imported by
# tests/test_head_inputs_cpu.py, which keeps them honest)
def make_edge_thetas(B, seed):
    """synthetic.make_thetas(B, seed) with nine kinds of edge row cycled over its rows; the cycle starts at kind seed % 9, so that
    small batches with different seeds see different kinds.  No pose entry equals -1e-8: batch_rodrigues divides by
    ||theta + 1e-8||, and the definition itself is NaN there."""
    th = synthetic.make_thetas(B, seed=seed)
    g = np.random.Generator(np.random.Philox(int(seed) + 7919))
    for i in range(B):
        kind = (i + int(seed)) % 9
        j = int(g.integers(1, 24))  # a non-root joint
        p = 3 + 3 * j
        if kind == 0:
            th[i, 3:75] = 0.0  # every rotation the identity (angle = sqrt(3) * 1e-8)
        elif kind == 1:
            th[i, p : p + 3] = 0.0
        elif kind == 2:
            th[i, 3:6] = (math.pi, 0.0, 0.0)
        elif kind == 3:
            th[i, p : p + 3] = (4.0, 4.0, 4.2)  # angle 7.05 > 2 pi
        elif kind == 4:
            th[i, p : p + 3] = (1e-4, -2e-4, 5e-5)
        elif kind == 5:
            th[i, 75:] = 3.0
        elif kind == 6:
            th[i, 75:] = -3.0
        elif kind == 7:
            th[i, 0] = -0.03
        else:
            th[i, 0] = 1e-3
    return th


def regress_features(M, seed=None):
    """the features of test_regress_stage, |N(0, 2)|, from the Philox stream M (or seed)"""
    g = np.random.Generator(np.random.Philox(int(M if seed is None else seed)))
    return np.abs(g.normal(0, 2, (M, 2048))).astype(np.float32)


POOL_CASES = [(16, 49, 2048), (17, 49, 2048), (3, 49, 20), (1, 7, 8), (33, 5, 12)]


def pool_input(B, HW, C):
    g = np.random.Generator(np.random.Philox(1000 * B + HW + C))
    return g.normal(0, 1, (B, HW, C)).astype(np.float32)


def rel_rows(a, b):
    """rel of test_gpu_parity.py per image: max over the rows of max|a - b| / max|b| of that row"""
    a = np.asarray(a, np.float64).reshape(len(a), -1)
    b = np.asarray(b, np.float64).reshape(len(b), -1)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((np.abs(a - b).max(1) / (np.abs(b).max(1) + 1e-30)).max())


def rel_rms(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.sqrt(np.mean(b * b)) + 1e-30))


def smpl_reference(osmpl, th):
    """the eight outputs of hpe_smpl from the oracle, in the oracle's own precision (osmpl.dtype), on the float32 rows th"""
    dt = osmpl.dtype
    th = np.asarray(th).astype(dt)
    verts, joints, Rs = osmpl(th[:, 75:], th[:, 3:75], get_skin=True)
    return {
        "verts": verts,
        "joints": joints,
        "cams": th[:, :3],
        "theta": th,
        "J_transformed": osmpl.J_transformed,
        "kp2d": O.batch_orth_proj_idrot(joints, th[:, :3]),
        "verts2d": O.reproject_vertices(verts, th[:, :3], IM_SIZE.astype(dt)),
        "Rs": Rs,
    }


def regress_reference(reg, feat, theta_prev):
    """one IEF step of the oracle in the precision of theta_prev"""
    dt = theta_prev.dtype
    return theta_prev + O.regression_network(np.concatenate([feat.astype(dt), theta_prev], 1), reg)


# ------------------------------------------------------------------------------------------- fixtures
def gpu(x):
    import torch

    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()


def cpu(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@pytest.fixture(scope="module")
def assets():
    a = dict(smpl=synthetic.make_smpl_model(), reg=synthetic.make_regressor_params(),
             reg_bounded=synthetic.make_regressor_params(variant="bounded"), mean=synthetic.make_mean_params())
    a["mean_var"] = O.load_mean_param(a["mean"])
    a["osmpl64"] = O.SMPL(a["smpl"], dtype=np.float64)
    return a


def _head_engine(assets, reg):
    """regressor + SMPL, no encoder: hpe_smpl, hpe_regress_stage, hpe_tail and the debug pools need no more"""
    e = hpe_amd.HpeEngine(device=0, max_batch=MAX_BATCH)
    e.load_smpl(assets["smpl"])
    e.load_regressor(assets[reg])
    e.load_mean_theta(assets["mean_var"])
    e.finalize()
    return e


@pytest.fixture(scope="module")
def engine(assets):
    e = _head_engine(assets, "reg")
    yield e
    e.close()


@pytest.fixture(scope="module")
def engine_bounded(assets):
    e = _head_engine(assets, "reg_bounded")
    yield e
    e.close()


_RUNS = {}  # B -> (theta rows, float64 reference, the all-outputs result of engine.smpl): computed once, never modified


def smpl_run(engine, assets, B):
    if B not in _RUNS:
        th = make_edge_thetas(B, seed=100 + B)
        out = {k: cpu(v) for k, v in engine.smpl(gpu(th), want=ALL_OUTPUTS).items()}
        _RUNS[B] = (th, smpl_reference(assets["osmpl64"], th), out)
    return _RUNS[B]


def check_against(out, ref, tag, bars=BARS):
    """every tensor of out against ref: the float64 bar, or bit for bit for the pass-through outputs"""
    worst = {}
    for k, v in out.items():
        if k in ("theta", "cams"):
            np.testing.assert_array_equal(bits(v), bits(ref[k]), err_msg="%s %s" % (tag, k))
        else:
            assert np.isfinite(v).all(), (tag, k)
            worst[k] = rel_rows(v, ref[k])
    print("HEAD %s: %s" % (tag, "  ".join("%s %.3g" % kv for kv in sorted(worst.items()))))
    for k, e in worst.items():
        assert e < bars[k], (tag, k, e, bars[k])
    return worst


# ------------------------------------------------------------------------------------------- 1. SMPL at each batch boundary
@pytest.mark.parametrize("B", [17, 16, 13, 9, 8, 7, 2, 1])
def test_smpl_matches_float64_at_batch_boundaries(engine, assets, B):
    """B = 1, 2, 7, 8: the small path up to its last size; 9, 13: one whole and one partial image tile of the large path; 16: whole
    tiles; 17: two tiles and one image.  DESCENDING B on the one engine, another seed per B: rows that a larger call left in pfT,
    betaT, A or kp_part would show in the smaller one."""
    th, ref, out = smpl_run(engine, assets, B)
    assert set(out) == set(ALL_OUTPUTS)
    check_against(out, ref, "smpl B=%d" % B)


# ------------------------------------------------------------------------------------------- 2. nothing past row B
@pytest.mark.parametrize("B", [9, 3])
def test_smpl_writes_nothing_past_row_B(engine, assets, B):
    """hpe_smpl into buffers of B + 8 rows: B = 9 is a partial image tile of smpl_skin_kernel (threads for images 9 ... 15 exist and
    are guarded), B = 3 the small path."""
    import torch

    th, _, want = smpl_run(engine, assets, B)
    shapes = engine._output_shapes(B + 8)
    bufs = {k: torch.full(shapes[k], SENTINEL, dtype=torch.float32, device="cuda") for k in ALL_OUTPUTS}
    o = _lib.HpeOutputs(*[bufs[k].data_ptr() for k in _lib.OUTPUT_FIELDS])
    tht = gpu(th)
    _lib.check(engine.lib.hpe_smpl(engine._h, tht.data_ptr(), B, C.byref(o), engine._stream()))
    torch.cuda.synchronize()
    sent = bits(np.float32(SENTINEL).reshape(1))[0]
    for k in ALL_OUTPUTS:
        got = cpu(bufs[k])
        assert (bits(got[B:]) == sent).all(), "%s: rows >= %d were written" % (k, B)
        np.testing.assert_array_equal(bits(got[:B]), bits(want[k]), err_msg=k)


# ------------------------------------------------------------------------------------------- 3. output subsets
SUBSETS = [("joints",), ("kp2d",), ("verts2d",), ("verts2d", "kp2d"), ("verts",), ("Rs", "J_transformed", "cams", "theta")]
# subsets whose launches are those of the all-outputs call (large path: the skin kernel's arithmetic into verts or verts_tmp, then
# joint_regress_kernel; no vertex output: smpl_pose_kernel alone) must reproduce it bit for bit
BITWISE = {(11, ("joints",)), (11, ("verts",)), (3, ("Rs", "J_transformed", "cams", "theta")), (11, ("Rs", "J_transformed", "cams", "theta"))}


@pytest.mark.parametrize("want", SUBSETS, ids=lambda w: "+".join(w))
@pytest.mark.parametrize("B", [3, 11])
def test_smpl_output_subsets(engine, assets, B, want):
    """Which outputs are requested selects the launches: the small kernel with verts == nullptr, with and without kp_part, W2D true
    and false; the large path into verts_tmp; the early return when no vertex output is wanted."""
    th, ref, full = smpl_run(engine, assets, B)
    out = {k: cpu(v) for k, v in engine.smpl(gpu(th), want=want).items()}
    assert set(out) == set(want)
    check_against(out, ref, "subset B=%d %s" % (B, "+".join(want)))
    same = {k: bool((bits(out[k]) == bits(full[k])).all()) for k in want}
    print("HEAD subset B=%d %s bitwise equal to the all-outputs call: %s" % (B, "+".join(want), same))
    if (B, want) in BITWISE:
        assert all(same.values()), same


# ------------------------------------------------------------------------------------------- 4. small and large path agree
def test_smpl_small_and_large_path_agree(engine, assets):
    th5 = make_edge_thetas(5, seed=41)
    th13 = make_edge_thetas(13, seed=42)
    th13[4:9] = th5
    small = {k: cpu(v) for k, v in engine.smpl(gpu(th5), want=ALL_OUTPUTS).items()}
    large = {k: cpu(v)[4:9] for k, v in engine.smpl(gpu(th13), want=ALL_OUTPUTS).items()}
    check_against(small, large, "small (B=5) vs rows 4..8 of large (B=13)")
    print("HEAD small vs large path: verts bitwise equal: %s" % bool((bits(small["verts"]) == bits(large["verts"])).all()))


# ------------------------------------------------------------------------------------------- 5. regressor stage
@pytest.mark.parametrize("variant", ["reg", "reg_bounded"])
@pytest.mark.parametrize("M", [1, 2, 3, 4, 5, 8, 64, 65])
def test_regress_stage_matches_float64(engine, engine_bounded, assets, M, variant):
    """M = 1, 2: dense_gemv_kernel<2> (2 = the full template); 3, 4: <4>; 5, 8: the first sizes of the 64x64 GEMM with split-K; 64,
    65: its tile edge.  Stage 1 from the tiled mean, stage 2 from the float32-rounded reference of stage 1."""
    e = engine_bounded if variant == "reg_bounded" else engine
    feat = regress_features(M)
    th0 = np.tile(assets["mean_var"].astype(np.float64), (M, 1))
    ref1 = regress_reference(assets[variant], feat, th0)
    t1 = cpu(e.regress_stage(gpu(feat)))
    prev = ref1.astype(np.float32)
    ref2 = regress_reference(assets[variant], feat, prev.astype(np.float64))
    t2 = cpu(e.regress_stage(gpu(feat), gpu(prev)))
    e1, e2 = rel_rows(t1, ref1), rel_rows(t2, ref2)
    print("HEAD regress %s M=%d: stage 1 %.3g  stage 2 %.3g" % (variant, M, e1, e2))
    assert np.isfinite(t1).all() and np.isfinite(t2).all()
    assert e1 < REG_BAR and e2 < REG_BAR, (e1, e2)


# ------------------------------------------------------------------------------------------- 6. hpe_tail
@pytest.mark.parametrize("B", [1, 4, 5, 9])
def test_tail_matches_float64(engine_bounded, assets, B):
    """hpe_tail hands SMPL theta rows of stride THETA_LD (hpe_smpl: 85) and runs the regressor on its own buffers: B = 1, 4 the GEMV,
    5, 9 the GEMM; SMPL small (1, 4, 5) and large with a partial tile (9).  Reference: three float64 regressor steps from the
    float64 mean, float64 SMPL and projection per stage.  Three chained stages amplify the first stage's rounding: the bar is the
    full-path TOL, on rel per image and, for kp2d and cams, on rel_rms; the bounded regressor keeps the camera scale, hence kp2d, well
    conditioned (asserted)."""
    feat = regress_features(B, seed=600 + B)
    stages = engine_bounded.tail(gpu(feat), all_stages=True, want=ALL_OUTPUTS)
    stages = [{k: cpu(v) for k, v in st.items()} for st in stages]
    assert len(stages) == 3
    th = np.tile(O.load_mean_param(assets["mean"], dtype=np.float64), (B, 1))
    for i in range(3):
        th = regress_reference(assets["reg_bounded"], feat, th)
        assert 0.5 <= th[:, 0].min() and th[:, 0].max() <= 1.2, th[:, 0]
        ref = smpl_reference(assets["osmpl64"], th)
        worst = {k: rel_rows(stages[i][k], ref[k]) for k in ALL_OUTPUTS}
        own = {k: rel_rms(stages[i][k], ref[k]) for k in ("kp2d", "cams")}
        print("HEAD tail B=%d stage %d: %s | rel_rms %s" % (B, i + 1, "  ".join("%s %.3g" % kv for kv in sorted(worst.items())),
                                                            "  ".join("%s %.3g" % kv for kv in sorted(own.items()))))
        for k, e in list(worst.items()) + list(own.items()):
            assert e < TOL, (B, i, k, e)
    for i in range(2):  # stage outputs are the stages', not aliases of the last one
        for k in ("theta", "verts", "joints", "kp2d"):
            assert not np.array_equal(stages[i][k], stages[2][k]), (i, k)


# ------------------------------------------------------------------------------------------- 7. average pool
@pytest.mark.parametrize("B,HW,C", POOL_CASES)
def test_avgpool_matches_float64(engine, B, HW, C):
    """(16, 49, 2048) / (17, 49, 2048): the last batch of avgpool_small_kernel and the first of avgpool_kernel at the encoder's
    shape; (3, 49, 20) and (1, 7, 8): B * C / 4 = 15 and 2 channel quads, a partial group of 32 -- the lane guard `ok`; (33, 5, 12):
    99 quads in a block of 256 -- the early return of avgpool_kernel.  Signed input; 8 sentinel floats behind the output."""
    import torch

    x = pool_input(B, HW, C)
    xt = gpu(x)
    y = torch.full((B * C + 8,), SENTINEL, dtype=torch.float32, device="cuda")
    _lib.check(engine.lib.hpe_debug_avgpool(xt.data_ptr(), B, HW, C, y.data_ptr(), None))
    torch.cuda.synchronize()
    got = cpu(y)
    assert (bits(got[B * C :]) == bits(np.float32(SENTINEL).reshape(1))[0]).all(), "wrote past the output"
    e = rel_rows(got[: B * C].reshape(B, C), x.astype(np.float64).mean(1))
    print("HEAD avgpool (%d, %d, %d): %.3g" % (B, HW, C, e))
    assert e < POOL_BAR


# ------------------------------------------------------------------------------------------- 8. max pool pad semantics
def maxpool_reference(x):
    """3x3 stride-2 max over the ZERO-padded input [B,H,H,C] (ZeroPadding2D + 'valid' MaxPooling2D): the pad takes part"""
    B, H, _, Cc = x.shape
    p = np.zeros((B, H + 2, H + 2, Cc), np.float32)
    p[:, 1:-1, 1:-1] = x
    Ho = H // 2
    out = np.full((B, Ho, Ho, Cc), -np.inf, np.float32)
    for dy in range(3):
        for dx in range(3):
            out = np.maximum(out, p[:, dy : dy + 2 * Ho : 2, dx : dx + 2 * Ho : 2])
    return out


@pytest.mark.parametrize("B,H,C", [(2, 6, 4), (1, 112, 64)])
def test_maxpool_zero_pad_takes_part(engine, B, H, C):
    """Signed input: a border window whose real entries are all negative gives 0, not their maximum (the kernel's header; with
    the non-negative data of test_pools the two readings cannot be told apart)."""
    import torch

    g = np.random.Generator(np.random.Philox(77 + H))
    x = g.normal(0, 1, (B, H, H, C)).astype(np.float32)
    x[0, :2, :2, 0] = -np.abs(x[0, :2, :2, 0]) - 0.5  # the top-left window of channel 0: four real entries, all negative
    x[-1, 1:4, 1:4, 1] = -np.abs(x[-1, 1:4, 1:4, 1]) - 0.5  # the interior window (1, 1), all negative: no pad, the result stays negative
    xt = gpu(x)
    y = torch.full((B, H // 2, H // 2, C), SENTINEL, dtype=torch.float32, device="cuda")
    _lib.check(engine.lib.hpe_debug_maxpool(xt.data_ptr(), B, H, C, y.data_ptr(), None))
    torch.cuda.synchronize()
    ref = maxpool_reference(x)
    assert ref[0, 0, 0, 0] == 0.0 and ref[-1, 1, 1, 1] < 0.0 and (ref < 0).any() and (ref[:, 0] == 0).any()
    np.testing.assert_array_equal(bits(cpu(y)), bits(ref))
