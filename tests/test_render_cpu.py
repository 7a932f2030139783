"""The CPU reference of the mesh renderer (tests/render_ref.py) against known answers, the face-list loaders and the ABI struct of the
renderer.  No GPU."""
import ctypes as C
import os
import pickle
import re

import numpy as np
import pytest

import render_ref as R
from hpe_amd import _lib, assets, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rec(xy_px, iz=None):
    """vertex records straight from pixel positions (snapped to 1/256 px)"""
    xy = np.asarray(xy_px, np.float64)
    n = len(xy)
    return {"U": np.rint(256 * xy[:, 0]).astype(np.int64), "V": np.rint(256 * xy[:, 1]).astype(np.int64), "valid": np.ones(n, bool),
            "iz": np.ones(n) if iz is None else np.asarray(iz, np.float64), "rgb": np.full((n, 3), 0.5)}


@pytest.mark.parametrize("lo,hi", [(10.0, 50.0), (10.5, 50.5), (10.25, 50.25)])
@pytest.mark.parametrize("flip", [False, True])
def test_square_covers_expected_pixels(lo, hi, flip):
    """an axis-aligned square of two triangles covers exactly 40 x 40 pixels, also when its edges run through the samples (x.5)"""
    rec = _rec([(lo, lo + 10), (hi, lo + 10), (hi, hi + 10), (lo, hi + 10)])
    faces = np.array([[0, 1, 2], [0, 3, 2] if flip else [0, 2, 3]])
    cnt = R.coverage_count(rec, faces, 80, 80)
    assert cnt.max() == 1
    assert cnt.sum() == 40 * 40
    ys, xs = np.nonzero(cnt)
    assert xs.max() - xs.min() == 39 and ys.max() - ys.min() == 39


@pytest.mark.parametrize("seed", range(6))
def test_fans_cover_each_sample_once(seed):
    """fans of triangles around a centre that sits on a sample (shared edges and a shared vertex through samples, both windings):
    every sample strictly inside the convex outline is covered exactly once, and none twice"""
    g = np.random.default_rng(seed)
    H = W = 64
    n = int(g.integers(3, 12))
    ang = np.sort(g.uniform(0, 2 * np.pi, n))
    rad = 25.0
    c = (32.5, 31.5)  # a pixel centre
    pts = [c] + [(c[0] + rad * np.cos(a), c[1] + rad * np.sin(a)) for a in ang]
    # snap outer points onto sample rows / columns now and then, so that edges pass through samples
    pts = [pts[0]] + [(np.floor(x) + 0.5 if g.random() < 0.3 else x, y) for x, y in pts[1:]]
    rec = _rec(pts)
    faces = np.array([[0, 1 + i, 1 + (i + 1) % n] for i in range(n)])
    flip = g.random(n) < 0.5
    faces[flip] = faces[flip][:, [0, 2, 1]]
    cnt = R.coverage_count(rec, faces, H, W)
    assert cnt.max() <= 1
    # samples strictly inside a fan triangle, or on a spoke between two of them when the centre is inside the outline
    yy, xx = np.mgrid[0:H, 0:W]
    sx, sy = 256 * xx + 128, 256 * yy + 128
    strict = np.zeros((H, W), bool)
    U, V = rec["U"], rec["V"]
    for f in faces:
        a, b, d = f
        e = [R._edge(U[p], V[p], U[q], V[q], sx, sy) for p, q in ((b, d), (d, a), (a, b))]
        area = R._edge(U[a], V[a], U[b], V[b], U[d], V[d])
        if area == 0:
            continue
        sgn = np.sign(area)
        strict |= (sgn * e[0] > 0) & (sgn * e[1] > 0) & (sgn * e[2] > 0)
    ang_ok = np.all(np.diff(np.concatenate([ang, [ang[0] + 2 * np.pi]])) < np.pi)  # centre strictly inside the outline
    if ang_ok:
        on_spoke = np.zeros((H, W), bool)
        for i in range(n):
            p = 1 + i
            e = R._edge(U[0], V[0], U[p], V[p], sx, sy)
            dot = (sx - U[0]) * (U[p] - U[0]) + (sy - V[0]) * (V[p] - V[0])
            L2 = (U[p] - U[0]) ** 2 + (V[p] - V[0]) ** 2
            on_spoke |= (e == 0) & (dot >= 0) & (dot < L2)
        strict |= on_spoke
        assert cnt[32, 32] == 1  # the centre sample (on every spoke)
    assert (cnt[strict] == 1).all(), int((cnt[strict] != 1).sum())


def test_nearer_square_wins():
    """two overlapping squares at z = 5 and z = 10 through the whole pipeline: the nearer one owns the overlap"""
    H = W = 96

    def square(z, x0, x1, y0, y1):  # camera-space corners projecting to the given pixel box with f = 500, pp = (48, 48)
        return [((x - 48) * z / 500.0, (y - 48) * z / 500.0, z) for x, y in ((x0, y0), (x1, y0), (x1, y1), (x0, y1))]

    verts = np.array(square(10.0, 10, 70, 10, 70) + square(5.0, 30, 90, 30, 90))
    faces = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]])
    rec = R.vertex_records(verts, faces, H, W)
    face, z = R.raster_ids(rec, faces, H, W)
    assert set(np.unique(face[30:70, 30:70])) <= {2, 3}
    assert set(np.unique(face[10:30, 10:30])) <= {0, 1} and (face[10:30, 10:30] >= 0).all()
    np.testing.assert_allclose(z[40, 40], 5.0, rtol=1e-12)
    np.testing.assert_allclose(z[15, 15], 10.0, rtol=1e-12)
    assert (face >= 0).sum() == 60 * 60 + 60 * 60 - 40 * 40
    # and with the faces listed in the other order (depth decides, not order)
    f2 = faces[[2, 3, 0, 1]]
    face2, _ = R.raster_ids(rec, f2, H, W)
    assert ((face2 >= 0) == (face >= 0)).all()
    assert set(np.unique(face2[30:70, 30:70])) <= {0, 1}


@pytest.mark.parametrize("bad", ["nan", "behind_near", "far"])
def test_face_with_bad_vertex_is_dropped(bad):
    H = W = 64
    verts = np.array([[-1.0, -1.0, 10.0], [1.0, -1.0, 10.0], [1.0, 1.0, 10.0], [-1.0, 1.0, 10.0]])
    faces = np.array([[0, 1, 2], [0, 2, 3]])
    far = None
    if bad == "nan":
        verts[1, 0] = np.nan
    elif bad == "behind_near":
        verts[1, 2] = 0.05  # < 0.1 = the default near for this mesh
    else:
        far = 10.0
        verts[1, 2] = 10.5
    rec = R.vertex_records(verts, faces, H, W, far=far)
    face, _ = R.raster_ids(rec, faces, H, W)
    assert set(np.unique(face)) == {-1, 1}  # face 0 (uses vertex 1) dropped, face 1 drawn
    img = R.shade(rec, faces, face)
    assert (img[face < 0] == 255).all()


def test_lambert_known_answer():
    """one camera-facing triangle far from the lights: vertex colour = albedo * sum_k colour_k * max(0, n . l_k) by hand"""
    verts = np.array([[0.0, 0.0, 5.0], [1.0, 0.0, 5.0], [0.0, 1.0, 5.0]])
    faces = np.array([[0, 1, 2]])
    rec = R.vertex_records(verts, faces, 64, 64, color_id=1)
    n = np.array([0.0, 0.0, 1.0])  # (v1 - v0) x (v2 - v0) = +z
    a = np.radians(120)
    ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    want = 0.0
    for pos, col in (([-200, -100, -100], 1.0), ([800, 10, 300], 1.0), ([-500, 500, 1000], 0.7)):
        L = np.array(pos, float) @ ry - verts[0]
        want += col * max(0.0, n @ L / np.linalg.norm(L))
    np.testing.assert_allclose(rec["rgb"][0], np.array([0.9, 0.7, 0.7]) * want, rtol=1e-12)


def test_rodrigues_matches_right_multiplication():
    """V' = (V - c) . R + c with cv2.Rodrigues' matrix: a +90 degree turn about y sends the row vector +x to +z"""
    R_ = R.rodrigues(2, 90.0)
    np.testing.assert_allclose(np.array([1.0, 0, 0]) @ R_, [0, 0, 1.0], atol=1e-12)
    np.testing.assert_allclose(R.rodrigues(3, 90.0) @ np.array([1.0, 0, 0]), [0, 1.0, 0], atol=1e-12)


def test_load_smpl_faces_formats(tmp_path):
    f = synthetic.make_faces(0)
    np.save(tmp_path / "smpl_faces.npy", f.astype(np.int64))
    np.savez(tmp_path / "model.npz", f=f.astype(np.uint32), v_template=np.zeros((6890, 3), np.float32))
    with open(tmp_path / "model.pkl", "wb") as fh:
        pickle.dump({"f": f.astype(np.uint32), "v_template": np.zeros((6890, 3))}, fh, protocol=2)
    for name in ("smpl_faces.npy", "model.npz", "model.pkl"):
        got = assets.load_smpl_faces(str(tmp_path / name))
        assert got.dtype == np.int32 and got.shape == (13776, 3)
        np.testing.assert_array_equal(got, f)
    bad = f.copy()
    bad[5, 1] = 6890
    np.save(tmp_path / "bad.npy", bad)
    with pytest.raises(assets.AssetError, match="outside"):
        assets.load_smpl_faces(str(tmp_path / "bad.npy"))
    bad[5, 1] = -1
    np.save(tmp_path / "neg.npy", bad)
    with pytest.raises(assets.AssetError):
        assets.load_smpl_faces(str(tmp_path / "neg.npy"))
    np.save(tmp_path / "shape.npy", f[:, :2])
    with pytest.raises(assets.AssetError):
        assets.load_smpl_faces(str(tmp_path / "shape.npy"))
    np.savez(tmp_path / "nof.npz", v=np.zeros(3))
    with pytest.raises(assets.AssetError):
        assets.load_smpl_faces(str(tmp_path / "nof.npz"))


def test_make_faces_deterministic_and_in_range():
    a, b = synthetic.make_faces(0), synthetic.make_faces(0)
    assert a.shape == (13776, 3) and a.dtype == np.int32
    np.testing.assert_array_equal(a, b)
    assert a.min() >= 0 and a.max() < 6890
    assert (a[:, 0] != a[:, 1]).all() and (a[:, 1] != a[:, 2]).all() and (a[:, 0] != a[:, 2]).all()
    assert len(np.unique(a)) == 6890
    assert not np.array_equal(a, synthetic.make_faces(1))


def test_render_params_struct_matches_header():
    txt = open(os.path.join(ROOT, "include", "hpe.h")).read()
    body = txt[txt.index("typedef struct HpeRenderParams {"):txt.index("} HpeRenderParams;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(int|float)\s+([a-z_0-9]+)\s*;", body)
    assert [n for _, n in fields] == [f[0] for f in _lib.HpeRenderParams._fields_]
    ctypes_of = {"int": C.c_int, "float": C.c_float}
    assert [ctypes_of[t] for t, _ in fields] == [f[1] for f in _lib.HpeRenderParams._fields_]
    assert C.sizeof(_lib.HpeRenderParams) == 4 * len(fields)


def test_render_params_init_and_checks_without_gpu():
    """defaults come from the library; a wrong struct_size is refused before anything touches a device"""
    from hpe_amd import build as hbuild

    hbuild.build()
    lib = _lib.load()
    p = _lib.HpeRenderParams()
    lib.hpe_render_params_init(C.byref(p))
    assert p.struct_size == C.sizeof(_lib.HpeRenderParams)
    assert (p.color_id, p.do_alpha, p.rot_axis, p.near, p.far) == (0, 0, 0, -1.0, -1.0)
    f = synthetic.make_faces(0)
    h = C.c_void_p()
    bad = f.copy()
    bad[7, 2] = 6890
    assert lib.hpe_renderer_create(0, bad.ctypes.data_as(C.c_void_p), len(bad), 6890, 4, C.byref(h)) == 1 and not h.value
    assert b"outside [0, 6890)" in lib.hpe_last_error()
    assert lib.hpe_renderer_create(0, f.ctypes.data_as(C.c_void_p), len(f), 6890, 0, C.byref(h)) == 1
    assert lib.hpe_render(None, None, None, 1, 8, 8, None, C.byref(p), None, None) == 1
