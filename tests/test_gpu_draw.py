"""GPU tests of the drawing (run with -m gpu on an MI355X): ``draw_panels`` at n = 2, T = 2, S = 224 and ``draw_skeleton`` at 32 x 48
against the NumPy restatement (tests/draw_ref.py), bit for bit -- integer raster rules, no tolerance -- on joints at the corners, outside
the panel on each side, coincident, invisible, on exact half pixels and NaN."""
import numpy as np
import pytest
import torch

import hpe_amd
from hpe_amd import draw

import draw_ref as D

pytestmark = pytest.mark.gpu
S, N, T = 224, 2, 2


@pytest.fixture(scope="module")
def inputs():
    rng = np.random.RandomState(11)
    images = rng.uniform(-1.0, 1.0, (N, S, S, 3)).astype(np.float32)
    images[0, :4, :4] = [[-1.0, 1.0, 0.0]]          # the ends of the range, exactly
    images[0, 4, :3, 0] = [1.5, -1.5, np.nan]        # outside it: clamped; a NaN reads 0
    images[1, 5, 5] = np.float32(2.0 / 255.0 - 1.0)  # products that sit next to an integer
    gt, pred = D.joint_cases(S)
    rend_img = rng.randint(0, 256, (N * T, S, S, 3)).astype(np.uint8)
    rend_seg = rng.randint(0, 256, (N * T, S, S, 3)).astype(np.uint8)
    return images, gt, pred, rend_img, rend_seg


@pytest.fixture(scope="module")
def want(inputs):
    return D.panels(*inputs)


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def assert_same(got, want, what):
    diff = (got != want).any(axis=-1)
    assert got.shape == want.shape and not diff.any(), "%s: %d pixels differ, first at %s: got %s want %s" % (
        what, int(diff.sum()), np.argwhere(diff)[0].tolist(), got[tuple(np.argwhere(diff)[0])].tolist(), want[tuple(np.argwhere(diff)[0])].tolist())


def test_panels_equal_the_restatement(inputs, want):
    got = hpe_amd.draw.draw_panels(*[cuda(a) for a in inputs])
    assert got.dtype == torch.uint8 and tuple(got.shape) == (N, T * S, 3 * S, 3)
    got = got.cpu().numpy()
    assert_same(got[:, :, S:], want[:, :, S:], "the rendered columns")
    assert_same(got[:, :, :S], want[:, :, :S], "the skeleton column")
    assert (want[0, :S, :S] != want[0, S:, :S]).any()  # the stages differ: each row block drew its own prediction


def test_one_panel_alone_equals_its_slice(inputs, want):
    images, gt, pred, ri, rs = inputs
    got = draw.draw_panels(cuda(images[1:]), cuda(gt[1:]), cuda(pred[1:, 1:]), cuda(ri[3:]), cuda(rs[3:])).cpu().numpy()
    assert_same(got[0], want[1, S:], "image 1, stage 1")


@pytest.mark.parametrize("draw_edges", [True, False])
def test_draw_skeleton_32x48_equals_the_restatement(draw_edges):
    H, W = 32, 48
    rng = np.random.RandomState(3)
    img = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    j = rng.uniform(2, 30, (19, 2)).astype(np.float32)
    j[:, 0] *= 1.5
    j[0], j[5] = (0, 0), (W - 1, H - 1)
    j[6], j[11], j[13], j[3] = (-3, 10), (W + 2, 12), (20, -4), (25, H + 1)  # outside on each side
    j[2] = j[1]  # coincident child and parent
    j[7], j[8] = (10.5, 11.5), (20.5, 3.5)  # -> (10, 12), (20, 4)
    j[15] = (np.nan, 9)
    j[12] = (1e9, -1e9)
    vis = np.ones(19, np.uint8)
    vis[4] = 0  # an invisible child (its parent 3 stays), and the invisible parent of child 5
    vis[9] = 0  # the invisible parent of children 3 and 10
    orig = img.copy()
    for v in (None, vis):
        want = D.draw_skeleton(img, j, draw_edges=draw_edges, vis=v)
        got = hpe_amd.draw_skeleton(img, j, draw_edges=draw_edges, vis=v)
        assert isinstance(got, np.ndarray) and got.dtype == np.uint8
        assert_same(got, want, "draw_edges=%s vis=%s" % (draw_edges, v is not None))
        assert (want != img).any() and (img == orig).all()  # drawn on a copy
    got = hpe_amd.draw_skeleton(cuda(img), torch.from_numpy(j.T.copy()), draw_edges=draw_edges, radius=3)  # a tensor in, [2,19] joints
    assert got.is_cuda
    assert_same(got.cpu().numpy(), D.draw_skeleton(img, j, draw_edges=draw_edges, radius=3), "radius 3")


def test_draw_skeleton_on_a_float_image():
    H, W = 32, 48
    img = np.random.RandomState(4).uniform(0, 1, (H, W, 3)).astype(np.float32)
    j = np.random.RandomState(5).uniform(0, 32, (19, 2)).astype(np.float32)
    got = hpe_amd.draw_skeleton(img, j)
    u8 = np.clip(np.trunc(img * np.float32(255)), 0, 255).astype(np.uint8)
    assert got.dtype == np.float32 and np.array_equal(got, D.draw_skeleton(u8, j).astype(np.float32) / np.float32(255))


def test_arguments_are_refused():
    with pytest.raises(ValueError, match="radius"):
        hpe_amd.draw_skeleton(np.zeros((8, 8, 3), np.uint8), np.zeros((19, 2), np.float32), radius=257)
    with pytest.raises(ValueError, match="joints"):
        hpe_amd.draw_skeleton(np.zeros((8, 8, 3), np.uint8), np.zeros((14, 2), np.float32))
    with pytest.raises(ValueError, match="rend_img"):
        draw.draw_panels(torch.zeros(1, 8, 8, 3).cuda(), torch.zeros(1, 19, 3), torch.zeros(1, 2, 19, 2), torch.zeros(1, 8, 8, 3, dtype=torch.uint8).cuda(),
                         torch.zeros(2, 8, 8, 3, dtype=torch.uint8).cuda())
