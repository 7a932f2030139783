"""GPU tests of the training-batch augmentation (run with -m gpu on an MI355X): hpe_augment_batch through ``augment_batch`` against the
NumPy float32 restatement that materialises every stage (tests/augment_ref.py), on random-noise uint8 frames so that a wrong tap
shows; both input forms, preallocated outputs, determinism, graph capture, error paths, and ``mocap_real``.

Bars (absolute).  images <= 2e-6: the resize's 1e-6 (three lerps of one product and two sums on values in [0,1]) doubled by
2 * (v - 0.5).  seg <= 1e-6.  kp_gt <= 2e-6: the kernel computes (kx - cx) + 112 where the restatement follows the reference's
(kx + 182) - (cx + 70); on coordinates below 1024 pixels that is one rounding of 6e-5 pixels, 5.4e-7 after 2 / 224, plus a few ulp
of 1.2e-7 from the last three operations (tests/test_augment_cpu.py holds the NumPy form of the kernel's rule to the same bar).
``seg > 0`` must equal the restatement's mask wherever the restatement's value is not in (0, 1e-6], and the fixture keeps that band
under 0.1 % of the pixels (asserted)."""
import ctypes as C

import numpy as np
import pytest
import torch

import hpe_amd
from hpe_amd import _lib, augment

import augment_ref as R
from smpl_torch_ref import make_theta

pytestmark = pytest.mark.gpu
IMG_BAR, SEG_BAR, KP_BAR = 2e-6, 1e-6, 2e-6
SENTINEL = 12345.678


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def check(got, want, what):
    errs = [float(np.abs(g.cpu().numpy().astype(np.float64) - w).max()) for g, w in zip(got, want)]
    print("%s: images %.3g (bar %.0e)  seg %.3g (bar %.0e)  kp_gt %.3g (bar %.0e)" % (what, errs[0], IMG_BAR, errs[1], SEG_BAR, errs[2], KP_BAR))
    assert tuple(got[0].shape) == want[0].shape and tuple(got[1].shape) == want[1].shape and tuple(got[2].shape) == want[2].shape
    assert all(g.dtype == torch.float32 and g.is_cuda for g in got)
    assert errs[0] <= IMG_BAR and errs[1] <= SEG_BAR and errs[2] <= KP_BAR


@pytest.fixture(scope="module")
def got5():
    frames, segs, kp, centers, draws = R.fixture()
    out = augment.augment_batch(frames, segs, kp, centers, draws=draws)
    torch.cuda.synchronize()
    return out


def test_b5_ragged(got5):
    want = R.reference()
    check(got5, want, "B = 5 ragged")
    band = (want[1] > 0) & (want[1] <= 1e-6)
    share = float(band.mean())
    print("mask pixels in (0, 1e-6]: %d of %d" % (int(band.sum()), band.size))
    assert share <= 1e-3
    mask = (got5[1] > 0).cpu().numpy()
    assert np.array_equal(mask[~band], (want[1] > 0)[~band])
    assert 0.2 < float(mask.mean()) < 0.95  # a mask with edges everywhere, not a constant


def test_b1():
    frames, segs, kp, centers, draws = R.fixture()
    one = {k: np.asarray(v)[1:2] for k, v in draws.items()}
    got = augment.augment_batch(frames[1:2], segs[1:2], kp[1:2], centers[1:2], draws=one)
    check(got, tuple(w[1:2] for w in R.reference()), "B = 1")


def _stack_case():
    """three 97 x 101 frames back to back: byte offsets 29391 b and 9797 b, odd"""
    g = np.random.RandomState(77)
    frames = g.randint(0, 256, (3, 97, 101, 3)).astype(np.uint8)
    segs = (g.randint(1, 256, (3, 97, 101)) * (g.rand(3, 97, 101) < 0.5)).astype(np.uint8)
    kp = R.fixture()[2][[4, 4, 0]]
    centers = np.array([[50, 48], [0, 96], [100, 0]], np.int32)
    draws = {"trans": np.array([[19, 19], [-20, 19], [3, -7]], np.int32), "scale": np.array([1.2299999, 0.8, 1.0], np.float32),
             "flip": np.array([True, False, True])}
    return frames, segs, kp, centers, draws


def test_single_tensor_form_equals_list_form():
    frames, segs, kp, centers, draws = _stack_case()
    as_list = augment.augment_batch(list(frames), list(segs), kp, centers, draws=draws)
    dev = augment.augment_batch(torch.from_numpy(frames).cuda(), torch.from_numpy(segs).cuda(), torch.from_numpy(kp).cuda(), centers, draws=draws)
    host = augment.augment_batch(torch.from_numpy(frames), segs, kp, torch.from_numpy(centers), draws={k: torch.from_numpy(v) for k, v in draws.items()})
    assert same_bits(dev, as_list) and same_bits(host, as_list)
    check(dev, R.augment_batch(frames, segs, kp, centers, draws), "B = 3 single tensor")


def test_preallocated_out(got5):
    frames, segs, kp, centers, draws = R.fixture()
    out = (torch.full((5, 224, 224, 3), SENTINEL, device="cuda"), torch.full((5, 224, 224), SENTINEL, device="cuda"),
           torch.full((5, 19, 3), SENTINEL, device="cuda"))
    ret = augment.augment_batch(frames, segs, kp, centers, draws=draws, out=out)
    assert all(r.data_ptr() == o.data_ptr() for r, o in zip(ret, out))
    assert same_bits(out, got5)


def test_determinism(got5):
    frames, segs, kp, centers, draws = R.fixture()
    other = augment.draw_augmentation(5, generator=torch.Generator().manual_seed(3))
    a = augment.augment_batch(frames, segs, kp, centers, draws=other, clamp=True)
    b = augment.augment_batch(frames, segs, kp, centers, draws=draws)
    assert same_bits(b, got5) and not torch.equal(a[0], b[0])
    c = augment.augment_batch(frames, segs, kp, centers, generator=torch.Generator().manual_seed(3), clamp=True)  # drawn inside
    assert same_bits(c, a)


def test_clamp_past_the_pad():
    """a window that leaves the 182-pixel pad: ValueError before any launch, and the kernel's clamp with clamp=True"""
    g = np.random.RandomState(5)
    img, seg = g.randint(0, 256, (60, 80, 3)).astype(np.uint8), g.randint(0, 256, (60, 80)).astype(np.uint8)
    kp = R.fixture()[2][:1]
    centers = np.array([[-150, 30]], np.int32)
    draws = {"trans": np.array([[-20, 0]], np.int32), "scale": np.array([1.1], np.float32), "flip": np.array([True])}
    with pytest.raises(ValueError):
        augment.augment_batch([img], [seg], kp, centers, draws=draws)
    got = augment.augment_batch([img], [seg], kp, centers, draws=draws, clamp=True)
    check(got, R.augment_batch([img], [seg], kp, centers, draws, fn=R.fused_sample), "clamped window")


def _raw_args(B=2):
    frames, segs, kp, centers, draws = _stack_case()
    f, s, k = torch.from_numpy(frames[:B]).cuda(), torch.from_numpy(segs[:B]).cuda(), torch.from_numpy(kp[:B]).cuda()
    table = augment.plan_augmentation([[97, 101]] * B, centers[:B], {n: v[:B] for n, v in draws.items()})
    tdev = torch.from_numpy(table.view(np.uint8)).cuda()
    out = (torch.full((B, 224, 224, 3), SENTINEL, device="cuda"), torch.full((B, 224, 224), SENTINEL, device="cuda"),
           torch.full((B, 19, 3), SENTINEL, device="cuda"))
    want = augment.augment_batch(f, s, k, centers[:B], draws={n: v[:B] for n, v in draws.items()})
    return f, s, k, table, tdev, out, want


def _call(f, s, table, tdev, k, B, out):
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    return _lib.load().hpe_augment_batch(f.data_ptr(), s.data_ptr(), table.ctypes.data_as(C.c_void_p), tdev.data_ptr(), k.data_ptr(), B,
                                         out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), st)


def test_graph_capture():
    """hpe_augment_batch captured once in a single-stream graph and replayed twice"""
    f, s, k, table, tdev, out, want = _raw_args()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert _call(f, s, table, tdev, k, 2, out) == 0
    torch.cuda.synchronize()
    assert float(out[0][0, 0, 0, 0]) == np.float32(SENTINEL)  # the capture enqueued nothing
    for _ in range(2):
        for o in out:
            o.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        assert same_bits(out, want)


def test_bad_arguments():
    frames, segs, kp, centers, draws = R.fixture()
    ab = augment.augment_batch
    with pytest.raises(ValueError):
        ab([f.astype(np.float32) for f in frames], segs, kp, centers, draws=draws)  # dtype
    with pytest.raises(ValueError):
        ab(frames, segs[:4], kp, centers, draws=draws)  # count
    with pytest.raises(ValueError):
        ab(frames, segs[1:] + segs[:1], kp, centers, draws=draws)  # sizes
    with pytest.raises(ValueError):
        ab(frames, segs, kp[:, :18], centers, draws=draws)  # kp shape
    with pytest.raises(ValueError):
        ab(frames, segs, kp, centers[:4], draws=draws)  # centers shape
    with pytest.raises(ValueError):
        ab(frames, segs, kp, torch.from_numpy(centers).cuda(), draws=draws)  # nothing reads the device
    with pytest.raises(ValueError):
        ab([f[:, :, :2] for f in frames], segs, kp, centers, draws=draws)  # channels
    with pytest.raises(ValueError):
        ab(torch.zeros((2, 50, 60, 3), dtype=torch.uint8).cuda()[:, :, ::2], torch.zeros((2, 50, 30), dtype=torch.uint8), kp[:2], centers[:2],
           draws={n: v[:2] for n, v in draws.items()})  # contiguity
    with pytest.raises(ValueError):
        ab(frames, segs, kp, centers, draws=draws, out=(torch.empty((5, 224, 224, 3), device="cuda"),) * 3)  # out shapes
    with pytest.raises(ValueError):
        ab([], [], kp, centers, draws=draws)  # empty
    # the library's own refusals: HPE_ERR_INVALID, and no launch (the outputs keep their sentinel)
    f, s, k, table, tdev, out, _ = _raw_args()
    lib = _lib.load()
    assert _call(f, s, table, tdev, k, 0, out) == 1 and b"B must be" in lib.hpe_last_error()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.hpe_augment_batch(None, s.data_ptr(), table.ctypes.data_as(C.c_void_p), tdev.data_ptr(), k.data_ptr(), 2, out[0].data_ptr(),
                                 out[1].data_ptr(), out[2].data_ptr(), st) == 1
    assert lib.hpe_augment_batch(f.data_ptr(), s.data_ptr(), table.ctypes.data_as(C.c_void_p), tdev.data_ptr(), k.data_ptr(), 2, out[0].data_ptr(),
                                 None, out[2].data_ptr(), st) == 1
    bad = table.copy()
    bad["newH"][1] = 0
    assert _call(f, s, bad, tdev, k, 2, out) == 1 and b"table entry 1" in lib.hpe_last_error()
    bad = table.copy()
    bad["newW"][0] = -3
    assert _call(f, s, bad, tdev, k, 2, out) == 1
    with pytest.raises(hpe_amd.HpeError):
        _lib.check(_call(f, s, bad, tdev, k, 2, out))
    torch.cuda.synchronize()
    assert all(bool((o == SENTINEL).all()) for o in out)


def test_mocap_real_and_seg_into_mesh_loss(smpl_model, got5):
    e = hpe_amd.HpeEngine(device=0, max_batch=2)
    try:
        e.load_smpl(smpl_model)
        e.finalize()
        th = torch.from_numpy(make_theta(3, seed=12).astype(np.float32)).cuda()
        joints, shapes, Rs = augment.mocap_real(e, th[:, 3:75].contiguous(), th[:, 75:].contiguous())
        assert tuple(joints.shape) == (3, 19, 3) and tuple(shapes.shape) == (3, 10) and tuple(Rs.shape) == (3, 24, 3, 3)
        assert torch.equal(bits(shapes), bits(th[:, 75:]))
        for lo, hi in ((0, 2), (2, 3)):  # engine.smpl on the rows, in the chunks max_batch = 2 gives: the same bits
            o = e.smpl(th[lo:hi], want=("joints", "Rs"))
            assert torch.equal(bits(joints[lo:hi]), bits(o["joints"])) and torch.equal(bits(Rs[lo:hi]), bits(o["Rs"]))
        for i in range(3):  # and one row at a time, with another camera: it does not enter joints or Rs (fp32 parity bar 1e-4)
            row = th[i : i + 1].clone()
            row[:, :3] = torch.tensor([0.7, 0.2, -0.1], device="cuda")
            o = e.smpl(row, want=("joints", "Rs"))
            assert float((joints[i : i + 1] - o["joints"]).abs().max()) <= 1e-4 and float((Rs[i : i + 1] - o["Rs"]).abs().max()) <= 1e-4
        with pytest.raises(ValueError):
            augment.mocap_real(e, th[:, 3:74], th[:, 75:])
        v2d = e.smpl(th[:2], want=("verts2d",))["verts2d"]
        loss = hpe_amd.mesh_reprojection_loss(e, got5[1][:2], v2d)
        want = hpe_amd.mesh_reprojection_loss(e, (got5[1][:2] > 0).float(), v2d)
        assert bool(torch.isfinite(loss)) and float(loss) > 0 and float(loss) == float(want)
    finally:
        e.close()
