"""Training-batch augmentation without a GPU: the NumPy restatement (tests/augment_ref.py) against torch's bilinear resize, the fused
read rule the kernel implements against the materialised restatement, hpe_augment_plan (host code of the built library) against the
restatement's integers and factors, the keypoint lines, and the window check.

Bounds.  Resize: 1e-6 absolute -- each of the three lerps has one product and two sums on values in [0,1], a few ulp of 6e-8; the
source coordinate is one fused multiply-add on both sides.  Fused
rule against the materialised stages: image and mask bit for bit (the same float32 operations on the same taps).  Keypoints: the fused
rule computes (kx - cx) + 112 where the reference computes (kx + 182) - (cx + 70); on coordinates below 1024 pixels the sums differ by
at most one rounding of 6e-5 pixels, 5.4e-7 after 2 / 224, under the 2e-6 bar the GPU test holds kp_gt to."""
import numpy as np
import pytest
import torch

import hpe_amd
from hpe_amd import augment

import augment_ref as R

F = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.int32)


RESIZE_CASES = [((37, 53), (45, 42)), ((301, 211), (240, 259))]


def _torch_resize(img, dst):
    t = torch.from_numpy(img).permute(2, 0, 1)[None]
    return torch.nn.functional.interpolate(t, size=dst, mode="bilinear", align_corners=False, antialias=False)[0].permute(1, 2, 0).numpy()


@pytest.mark.parametrize("src,dst", RESIZE_CASES)
def test_resize_rule_matches_torch_interpolate(src, dst):
    """The restatement's resize against torch.nn.functional.interpolate on float noise, 1e-6 absolute: each of the three lerps has one
    product and two sums on values in [0,1].  Measured 1.2e-7 at 37 x 53 -> 45 x 42 and 1.8e-7 at 301 x 211 -> 240 x 259.  This holds
    because the source coordinate (o + 0.5) * scale - 0.5 is ONE fused multiply-add in the restatement, as in torch's kernel: with the
    product rounded first the coordinates differ by up to half an ulp of the product and the same comparison gives 1.55e-6 and 1.39e-5."""
    img = np.random.RandomState(src[0]).rand(src[0], src[1], 3).astype(F)
    got = R.resize_bilinear(img, dst[0], dst[1])
    want = _torch_resize(img, dst)
    err = float(np.abs(got - want).max())
    print("resize %s -> %s: max abs err %.3g" % (src, dst, err))
    assert got.shape == want.shape and err <= 1e-6


def test_resize_to_same_size_is_identity():
    img = np.random.RandomState(1).rand(19, 23, 3).astype(F)
    assert np.array_equal(bits(R.resize_bilinear(img, 19, 23)), bits(img))


def test_fused_read_rule_equals_materialised_stages():
    fx = R.fixture()
    want = R.reference()
    got = R.augment_batch(*fx, fn=R.fused_sample)
    assert np.array_equal(bits(got[0]), bits(want[0])), "image"
    assert np.array_equal(bits(got[1]), bits(want[1])), "seg"
    err = float(np.abs(got[2] - want[2]).max())
    print("kp_gt fused vs reference order: max abs err %.3g" % err)
    assert err <= 2e-6
    assert np.array_equal(got[2][..., 2], want[2][..., 2])


def _near_integer_cases():
    """(H, W, scale) with H * scale within 1e-4 of an integer from both sides, and on it"""
    out = []
    for H, W, n in [(250, 333, 200), (301, 211, 370), (97, 101, 97), (480, 640, 500), (150, 151, 121)]:
        s = F(n) / F(H)
        for k in (-1, 0, 1):
            sc = s
            for _ in range(abs(k)):
                sc = np.nextafter(sc, F(np.inf) if k > 0 else F(0))
            assert abs(float(H) * float(sc) - n) < 1e-4
            out.append((H, W, F(sc)))
    return out


def test_host_plan_equals_restatement():
    cases = _near_integer_cases()
    g = np.random.RandomState(7)
    for H, W in R.SIZES + [(500, 150), (3, 2)]:
        for sc in g.uniform(0.8, 1.23, 3).astype(F):
            cases.append((H, W, sc))
    B = len(cases)
    sizes = np.array([(c[0], c[1]) for c in cases], np.int32)
    centers = np.stack([g.randint(-30, 700, B), g.randint(-30, 700, B)], 1).astype(np.int32)
    centers[::3] = g.randint(-19, 20, (len(centers[::3]), 2))  # with the jitter below: negative jittered centres
    draws = {"trans": g.randint(-20, 20, (B, 2)).astype(np.int32), "scale": np.array([c[2] for c in cases], F), "flip": g.rand(B) < 0.5}
    draws["trans"][::3] = -20
    tab = augment.plan_augmentation(sizes, centers, draws, clamp=True)
    assert tab.dtype == augment.TABLE_DTYPE and tab.shape == (B,)
    n_neg = 0
    for b in range(B):
        want = R.geometry(sizes[b, 0], sizes[b, 1], centers[b], draws["trans"][b], draws["scale"][b])
        for k in ("newH", "newW", "cx", "cy"):
            assert int(tab[k][b]) == want[k], (b, k, cases[b])
        for k in ("fx", "fy", "rx", "ry"):
            assert bits(tab[k][b]) == bits(want[k]), (b, k, cases[b])
        assert bool(tab["inside"][b]) == want["inside"] and bool(tab["flip"][b]) == bool(draws["flip"][b])
        assert (int(tab["H"][b]), int(tab["W"][b])) == tuple(sizes[b])
        n_neg += want["cx"] < 0 or want["cy"] < 0
    assert n_neg >= 3
    area = sizes[:, 0].astype(np.int64) * sizes[:, 1]
    assert np.array_equal(tab["seg_offset"], np.concatenate([[0], np.cumsum(area)[:-1]]))
    assert np.array_equal(tab["frame_offset"], 3 * tab["seg_offset"])


def test_host_plan_refuses_bad_arguments():
    ok = {"trans": [[0, 0]], "scale": [1.0], "flip": [False]}
    with pytest.raises(hpe_amd.HpeError):
        augment.plan_augmentation([[0, 5]], [[1, 1]], ok)
    with pytest.raises(hpe_amd.HpeError):  # newH = int(2 * 0.4) = 0
        augment.plan_augmentation([[2, 50]], [[1, 1]], dict(ok, scale=[0.4]))
    with pytest.raises(hpe_amd.HpeError):
        augment.plan_augmentation([[20, 50]], [[1, 1]], dict(ok, scale=[float("nan")]))
    with pytest.raises(hpe_amd.HpeError):
        augment.plan_augmentation([[20, 50]], [[1, 1]], ok, frame_offsets=[-1])
    with pytest.raises(ValueError):
        augment.plan_augmentation([[20, 50]], [[1, 1, 1]], ok)
    with pytest.raises(ValueError):
        augment.plan_augmentation([[20, 50]], [[1, 1]], {"trans": [[0, 0]], "scale": [1.0]})
    with pytest.raises(ValueError):
        augment.plan_augmentation([[20, 50]], [[1.5, 1.0]], ok)


def test_keypoint_flip_lines():
    assert tuple(R.SWAP_INDS) == augment.SWAP_INDS
    assert np.array_equal(R.SWAP_INDS[R.SWAP_INDS], np.arange(19))  # an involution
    g = np.random.RandomState(3)
    x = (g.randint(-8 * 300, 8 * 300, 19) / 8.0).astype(F)  # eighths of a pixel: 224 - x - 1 is exact
    y = g.uniform(-50, 300, 19).astype(F)
    vis = g.choice([0.0, 1.0], 19).astype(F)
    once = R.flip_keypoints(x, y, vis)
    assert not np.array_equal(once[0], x)
    twice = R.flip_keypoints(*once)
    for a, b in zip(twice, (x, y, vis)):
        assert np.array_equal(bits(a), bits(b))


def test_invisible_rows_are_zero():
    kp_in = R.fixture()[2]
    flip = R.DRAWS["flip"]
    n = 0
    for fn in (R.augment_sample, R.fused_sample):
        kp_gt = R.augment_batch(*R.fixture(), fn=fn)[2]
        for b in range(len(kp_in)):
            vis = kp_in[b, :, 2][R.SWAP_INDS] if flip[b] else kp_in[b, :, 2]
            assert np.array_equal(kp_gt[b, :, 2], (vis > 0).astype(F))
            assert np.all(kp_gt[b][vis <= 0] == 0)
            n += int((vis <= 0).sum())
    assert n >= 10


def test_window_past_the_pad_raises_or_clamps():
    g = np.random.RandomState(5)
    img = g.randint(0, 256, (60, 80, 3)).astype(np.uint8)
    seg = g.randint(0, 256, (60, 80)).astype(np.uint8)
    kp = np.zeros((19, 3), F)
    center, trans, scale = np.array([-150, 30]), np.array([-20, 0]), F(1.0)  # start_x = -170 + 182 - 112 < 0
    draws = {"trans": trans[None], "scale": [scale], "flip": [False]}
    with pytest.raises(ValueError):
        R.augment_sample(img, seg, kp, center, trans, scale, False)
    with pytest.raises(ValueError):
        augment.plan_augmentation([[60, 80]], center[None], draws)
    tab = augment.plan_augmentation([[60, 80]], center[None], draws, clamp=True)
    assert tab["inside"][0] == 0 and tab["cx"][0] == -170
    # clamping on = a wider pad: the materialised stages with a margin that holds the window give the fused rule's bits
    wide = R.augment_sample(img, seg, kp, center, trans, scale, False, trans_max=200)
    got = R.fused_sample(img, seg, kp, center, trans, scale, False)
    assert np.array_equal(bits(got[0]), bits(wide[0])) and np.array_equal(bits(got[1]), bits(wide[1]))
    assert np.array_equal(got[0][:, :, 0], np.broadcast_to(got[0][:, :1, 0], (224, 224)))  # every column reads column 0
    inside = augment.plan_augmentation([[60, 80]], [[40, 30]], draws)
    assert inside["inside"][0] == 1


def test_draw_augmentation_ranges():
    g = torch.Generator().manual_seed(0)
    d = augment.draw_augmentation(4096, generator=g)
    assert d["trans"].dtype == torch.int32 and tuple(d["trans"].shape) == (4096, 2)
    assert int(d["trans"].min()) == -20 and int(d["trans"].max()) == 19
    assert d["scale"].dtype == torch.float32 and float(d["scale"].min()) >= 0.8 and float(d["scale"].max()) <= 1.23
    assert d["flip"].dtype == torch.bool and 0.4 < float(d["flip"].float().mean()) < 0.6
    d2 = augment.draw_augmentation(4096, generator=torch.Generator().manual_seed(0))
    assert all(torch.equal(d[k], d2[k]) for k in d)
    with pytest.raises(ValueError):
        augment.draw_augmentation(0)
