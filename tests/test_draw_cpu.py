"""CPU tests of the drawing's definition (no GPU): hand-checked pixels of one disc, one ring and one edge under the raster rules of
DESIGN.md "Training summaries" as tests/draw_ref.py restates them; the rounding of joint coordinates; the paint order; and that the
tables hpe_amd/draw.py hands the kernels are the restatement's."""
import numpy as np

from hpe_amd import draw

import draw_ref as D


def pts(mask):
    return sorted((int(x), int(y)) for y, x in np.argwhere(mask))


def test_disc_pixels():
    """r = 2 at (3, 3): d2 <= 4 -- the 3 x 3 block (d2 <= 2) and the four axis points at distance 2; (1, 2) has d2 = 5: out"""
    m = D.disc_mask(7, 7, 3, 3, 2)
    assert pts(m) == sorted([(x, y) for x in (2, 3, 4) for y in (2, 3, 4)] + [(1, 3), (5, 3), (3, 1), (3, 5)])
    assert pts(D.disc_mask(7, 7, 3, 3, 0)) == [(3, 3)]
    assert pts(D.disc_mask(4, 4, -1, -1, 2)) == [(0, 0)]  # a centre outside clips: d2 = 2; (1, 0) has d2 = 5


def test_ring_pixels():
    """r = 3 at (4, 4): 25 <= 4 * d2 < 49, i.e. d2 in 7 .. 12: (+-3, 0) d2 = 9, (+-3, +-1) d2 = 10, (+-2, +-2) d2 = 8 and their
    mirrors; (+-2, +-1) d2 = 5 is inside the hole, (+-3, +-2) d2 = 13 outside"""
    m = D.ring_mask(9, 9, 4, 4, 3)
    want = set()
    for dx, dy in ((3, 0), (3, 1), (2, 2)):
        for sx in (1, -1):
            for sy in (1, -1):
                want |= {(4 + sx * dx, 4 + sy * dy), (4 + sy * dy, 4 + sx * dx)}
    assert pts(m) == sorted(want) and len(want) == 16
    assert not m[4, 4] and not m[5, 6] and not m[6, 7]


def test_edge_pixels():
    """th = 2 from (1, 1) to (5, 1): 4 * dist2 <= 4, distance at most 1 -- rows 0 .. 2 over x = 1 .. 5 and the two cap points (0, 1),
    (6, 1); the corners (0, 0), (6, 2) have dist2 = 2: out.  A diagonal of th = 2 from (0, 0) to (4, 4): the pixels with |x - y| <= 1
    between the ends (dist2 = (x - y)^2 / 2 <= 1), and past the end (4, 5) and (5, 4) at distance 1 but not (5, 5) at dist2 = 2"""
    m = D.edge_mask(3, 8, 1, 1, 5, 1, 2)
    assert pts(m) == sorted([(x, y) for x in range(1, 6) for y in range(3)] + [(0, 1), (6, 1)])
    d = D.edge_mask(6, 6, 0, 0, 4, 4, 2)
    assert pts(d) == sorted((x, y) for x in range(6) for y in range(6) if abs(x - y) <= 1 and (x, y) != (5, 5))  # (4, 5), (5, 4): the cap
    # b.b == 0: the first branch, 4 * d2 <= 9, d2 <= 2: the 3 x 3 block; with th = 2, d2 <= 1: the plus
    assert pts(D.edge_mask(5, 5, 2, 2, 2, 2, 3)) == sorted((x, y) for x in (1, 2, 3) for y in (1, 2, 3))
    assert pts(D.edge_mask(5, 5, 2, 2, 2, 2, 2)) == [(1, 2), (2, 1), (2, 2), (2, 3), (3, 2)]


def test_edge_with_far_end_points_is_exact():
    """an end point at -32768: |a|^2 * (b.b) leaves 64 bits; the restatement's Python integers still see the line y = x"""
    m = D.edge_mask(8, 8, 3, 3, -32768, -32768, 1)
    assert pts(m) == [(0, 0), (1, 1), (2, 2), (3, 3)]


def test_joint_pixels_round_half_to_even_clamp_and_nan():
    got = D.joint_pixels(np.array([0.5, 1.5, 2.5, -0.5, -1.5, 1e9, -1e9, np.nan, np.inf, 32768.4], np.float32))
    assert got.tolist() == [0, 2, 2, 0, -2, 32768, -32768, -32768, 32768, 32768]
    gt, pred = D.joint_cases()
    to_px = ((pred[0, 1, [7, 8]] + np.float32(1)) * np.float32(0.5)) * np.float32(224)
    assert to_px.tolist() == [[10.5, 17.5], [24.5, 101.5]]  # exact halves reach the rounding
    assert D.joint_pixels(to_px).tolist() == [[10, 18], [24, 102]]


def test_paint_order_last_paint_wins():
    """the chain 2 -> 8 -> 12 (light pink, light blue, purple) along y = 20, radius 5: per child a white disc r = 5, its disc r = 4, the
    parent's disc r = 4, then the edge of thickness 3 (|dy| <= 1); children in the order 2, 8, 12"""
    img = np.zeros((40, 60, 3), np.uint8)
    j = np.full((19, 2), -1000.0, np.float32)
    j[2], j[8], j[12] = (10, 20), (30, 20), (50, 20)
    vis = np.zeros(19, bool)
    vis[[2, 8, 12]] = True  # 12's parent 14 is invisible: no disc there and no edge
    out = D.draw_skeleton(img, j, vis=vis, radius=5)
    at = lambda x, y: tuple(out[y, x].tolist())  # noqa: E731
    assert at(10, 20) == D.LPINK and at(10, 15) == D.WHITE  # the joint (the edge starts over it), the white rim at distance 5
    assert at(20, 20) == D.LPINK and at(20, 21) == D.LPINK and at(20, 22) == (0, 0, 0)  # edge 2 -> 8
    assert at(26, 20) == D.LBLUE  # inside joint 8's disc, painted over the end of edge 2
    assert at(25, 20) == D.WHITE  # child 8's white rim, painted AFTER child 2's edge ...
    assert at(35, 20) == D.LBLUE  # ... and BEFORE its own edge, which runs over the rim
    assert at(45, 20) == D.WHITE  # child 12's rim over edge 8
    assert at(50, 20) == D.PURPLE and at(55, 20) == D.WHITE and at(57, 20) == (0, 0, 0)
    rings = D.draw_skeleton(img, j, draw_edges=False, vis=vis, radius=5)  # rings of radius 4: d2 in 13 .. 20
    assert tuple(rings[20, 14]) == D.LPINK and tuple(rings[20, 34]) == D.LBLUE and not rings[20, 10].any() and not rings[20, 20].any()
    assert not rings[20, 13].any() and tuple(rings[23, 13]) == D.LPINK  # d2 = 9: the hole; d2 = 18: the ring


def test_tables_of_draw_py_are_the_restatements():
    t = draw.skeleton_table()
    assert t.shape == (19, 8) and t.dtype == np.int32
    assert t[:, 0].tolist() == D.PARENTS and [tuple(r) for r in t[:, 1:4].tolist()] == D.JCOLORS
    for j in range(19):
        assert tuple(t[j, 4:7].tolist()) == (D.ECOLORS[j] if D.PARENTS[j] >= 0 else (0, 0, 0))
    assert set(D.ECOLORS) == {j for j in range(19) if D.PARENTS[j] >= 0}
    assert draw.default_radius(224, 224) == 4 and draw.default_radius(1000, 600) == 8
