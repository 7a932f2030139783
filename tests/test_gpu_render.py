"""The mesh renderer on the GPU (hpe_render, csrc/render.hip) against the CPU reference tests/render_ref.py."""
import ctypes as C

import numpy as np
import pytest

import render_ref as R

pytestmark = pytest.mark.gpu

P = 6890


@pytest.fixture(scope="module")
def torch():
    import torch as t

    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


@pytest.fixture(scope="module")
def lib(torch):
    from hpe_amd import _lib, build as hbuild

    hbuild.build()
    return _lib.load()


@pytest.fixture(scope="module")
def faces():
    from hpe_amd import synthetic

    return synthetic.make_faces(0)


class _Handle(object):
    def __init__(self, lib, faces, P, max_batch):
        self.lib = lib
        self.h = C.c_void_p()
        rc = lib.hpe_renderer_create(0, faces.ctypes.data_as(C.c_void_p), len(faces), P, max_batch, C.byref(self.h))
        assert rc == 0, lib.hpe_last_error()

    def __del__(self):
        self.lib.hpe_renderer_destroy(self.h)


def _params(lib, **kw):
    from hpe_amd import _lib

    p = _lib.HpeRenderParams()
    lib.hpe_render_params_init(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.fixture(scope="module")
def meshes(torch, faces, tmp_path_factory):
    """synthetic SMPL meshes through the real path: Predictor.predict -> get_original on a 480 x 640 frame (the preview.py case).
    The "bounded" regressor keeps the camera scale near the mean (s ~ 0.69): the meshes sit in front of the camera."""
    import hpe_amd
    from hpe_amd import synthetic

    face_path = str(tmp_path_factory.mktemp("faces") / "smpl_faces.npy")
    np.save(face_path, faces)

    class Cfg(object):
        img_size = 224
        num_stage = 3
        batch_size = 4
        data_format = "NHWC"
        checkpoint_dir = None
        smpl_model_path = None
        smpl_face_path = face_path

    p = hpe_amd.Predictor(Cfg(), smpl_model=synthetic.make_smpl_model(), mean_params=synthetic.make_mean_params(),
                          encoder_params=synthetic.make_encoder_params(), regressor_params=synthetic.make_regressor_params(variant="bounded"))
    frame = (np.random.default_rng(3).random((480, 640, 3)) * 255).astype(np.uint8)
    crop, proc, _ = hpe_amd.preprocess_image(frame)
    imgs = torch.cat([crop[None]] + [torch.as_tensor(synthetic.make_images(3, seed=9)).cuda()], 0)
    r = p.predict(imgs)
    out = []
    for b in range(4):
        cfr, vs, _ = hpe_amd.get_original(proc, r["generated_verts"][b], r["generated_cams"][b], r["generated_kp2d"][b])
        out.append((vs.contiguous(), cfr))
    return {"frame": frame, "meshes": out, "predictor": p, "face_path": face_path}


def _gpu_records(torch, lib, h, verts, cams, H, W, **kw):
    B = verts.shape[0]
    rec = torch.empty((B, verts.shape[1], 8), dtype=torch.int32, device="cuda")
    cam = None if cams is None else torch.as_tensor(np.asarray(cams, np.float32)).reshape(B, 3).cuda()
    rc = lib.hpe_debug_render_vertices(h.h, verts.data_ptr(), None if cam is None else cam.data_ptr(), B, H, W, C.byref(_params(lib, **kw)),
                                       rec.data_ptr(), None)
    assert rc == 0, lib.hpe_last_error()
    torch.cuda.synchronize()
    return rec.cpu().numpy()


def _gpu_ids(torch, lib, h, verts, cams, H, W, **kw):
    B = verts.shape[0]
    face = torch.empty((B, H, W), dtype=torch.int32, device="cuda")
    z = torch.empty((B, H, W), dtype=torch.float32, device="cuda")
    cam = None if cams is None else torch.as_tensor(np.asarray(cams, np.float32)).reshape(B, 3).cuda()
    rc = lib.hpe_debug_render_ids(h.h, verts.data_ptr(), None if cam is None else cam.data_ptr(), B, H, W, C.byref(_params(lib, **kw)),
                                  face.data_ptr(), z.data_ptr(), None)
    assert rc == 0, lib.hpe_last_error()
    torch.cuda.synchronize()
    return face.cpu().numpy(), z.cpu().numpy()


@pytest.mark.parametrize("rot", [(0, 0.0), (1, 60.0), (2, 60.0), (3, -35.0)])
def test_vertex_records_vs_float64(torch, lib, faces, meshes, rot):
    h = _Handle(lib, faces, P, 4)
    vs, cfr = meshes["meshes"][0]
    rec = _gpu_records(torch, lib, h, vs[None], cfr, 480, 640, rot_axis=rot[0], rot_deg=rot[1], color_id=rot[0])
    ref = R.vertex_records(vs.cpu().numpy(), faces, 480, 640, cfr, rot[0], rot[1], color_id=rot[0])
    g = R.records_from_gpu(rec[0])
    assert g["valid"].all() and ref["valid"].all()
    np.testing.assert_allclose(g["U"] / 256.0, ref["u"], rtol=1e-5, atol=1.0 / 512 + 1e-6)
    np.testing.assert_allclose(g["V"] / 256.0, ref["v"], rtol=1e-5, atol=1.0 / 512 + 1e-6)
    np.testing.assert_allclose(g["iz"], 1.0 / ref["verts"][:, 2], rtol=1e-5)
    # colours where the normal is well conditioned: a vertex whose face normals nearly cancel has a direction that float32 rounding
    # of the sum decides (the synthetic face list has a few; float64 differs there by design, not by error)
    good = R.normal_condition(ref["verts"], faces) < 100
    assert good.mean() > 0.99
    np.testing.assert_allclose(g["rgb"][good], ref["rgb"][good], rtol=0, atol=1e-5)


def _check_ids(face_g, z_g, rec, faces, H, W):
    face_r, z_r = R.raster_ids(rec, faces, H, W)
    np.testing.assert_array_equal(face_g >= 0, face_r >= 0)  # coverage: bitwise
    assert (face_r >= 0).sum() > 0.01 * H * W, "mesh barely in view: the test would be vacuous"
    diff = np.nonzero(face_g != face_r)
    if len(diff[0]):  # a different winner only where the two candidates are at the same depth
        zg = R.depth_of(rec, faces, face_g[diff], diff[0], diff[1])
        np.testing.assert_allclose(zg, z_r[diff], rtol=1e-5)
    cov = face_r >= 0
    np.testing.assert_allclose(z_g[cov], z_r[cov], rtol=1e-5)
    assert len(diff[0]) <= 0.02 * cov.sum()  # near-ties: faces meeting at a shared vertex or edge at equal depth


@pytest.mark.parametrize("B,H,W", [(1, 224, 224), (3, 224, 224), (1, 480, 640)])
def test_ids_vs_reference(torch, lib, faces, meshes, B, H, W):
    h = _Handle(lib, faces, P, 4)
    if (H, W) == (480, 640):
        verts = meshes["meshes"][0][0][None].contiguous()
        cams = meshes["meshes"][0][1][None]
    else:  # the crop-space meshes: camera (500, 112, 112) looking at vert_shifted of a 224 x 224 frame
        verts = torch.stack([m[0] for m in meshes["meshes"][1 : 1 + B]]).contiguous()
        cams = None
    rec = _gpu_records(torch, lib, h, verts, cams, H, W)
    face_g, z_g = _gpu_ids(torch, lib, h, verts, cams, H, W)
    for b in range(B):
        _check_ids(face_g[b], z_g[b], R.records_from_gpu(rec[b]), faces, H, W)


@pytest.mark.parametrize("bg,do_alpha,color_id", [(True, True, 0), (True, False, 1), (False, True, 1), (False, False, 0)])
def test_images_vs_reference(torch, lib, faces, meshes, bg, do_alpha, color_id):
    from hpe_amd import SMPLRenderer

    vs, cfr = meshes["meshes"][0]
    frame = meshes["frame"]
    r = SMPLRenderer(faces=faces)
    img = r(vs.cpu().numpy(), cfr, frame if bg else None, do_alpha, color_id=color_id, img_size=(480, 640))
    assert isinstance(img, np.ndarray) and img.dtype == np.uint8 and img.shape == (480, 640, 4 if do_alpha else 3)
    h = _Handle(lib, faces, P, 1)
    rec = R.records_from_gpu(_gpu_records(torch, lib, h, vs[None], cfr, 480, 640, color_id=color_id)[0])
    face_g, _ = _gpu_ids(torch, lib, h, vs[None], cfr, 480, 640)
    face_r, _ = R.raster_ids(rec, faces, 480, 640)
    ref = R.shade(rec, faces, face_r, frame if bg else None, do_alpha)
    cov = face_r >= 0
    assert cov.sum() > 1000
    same = face_g[0] == face_r
    d = np.abs(img.astype(int) - ref.astype(int))
    assert d[same].max() <= 1
    np.testing.assert_array_equal(img[~cov][:, :3], (frame[~cov] if bg else np.full(((~cov).sum(), 3), 255, np.uint8)))
    if do_alpha:
        np.testing.assert_array_equal(img[..., 3], 255 if bg else np.where(cov, 255, 0))


def test_rotated_image_vs_reference(torch, lib, faces, meshes):
    from hpe_amd import SMPLRenderer

    vs, cfr = meshes["meshes"][0]
    r = SMPLRenderer(faces=faces)
    img = r.rotated(vs.cpu().numpy(), 60, cam=cfr, img_size=(480, 640))  # preview.py:85, do_alpha=True by default
    assert img.shape == (480, 640, 4)
    h = _Handle(lib, faces, P, 1)
    rec = R.records_from_gpu(_gpu_records(torch, lib, h, vs[None], cfr, 480, 640, rot_axis=2, rot_deg=60.0)[0])
    face_r, _ = R.raster_ids(rec, faces, 480, 640)
    face_g, _ = _gpu_ids(torch, lib, h, vs[None], cfr, 480, 640, rot_axis=2, rot_deg=60.0)
    ref = R.shade(rec, faces, face_r, None, True)
    same = face_g[0] == face_r
    assert np.abs(img.astype(int) - ref.astype(int))[same].max() <= 1
    np.testing.assert_array_equal(img[..., 3], np.where(face_r >= 0, 255, 0))


def _quad(z, x0, x1, y0, y1, W, H):
    return [((x - W / 2) * z / 500.0, (y - H / 2) * z / 500.0, z) for x, y in ((x0, y0), (x1, y0), (x1, y1), (x0, y1))]


@pytest.mark.parametrize("lo,hi", [(10.0, 50.0), (10.5, 50.5)])
def test_analytic_square_pixel_count(torch, lib, lo, hi):
    verts = np.array(_quad(5.0, lo, hi, lo + 7, hi + 7, 96, 80), np.float32)
    faces = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    h = _Handle(lib, faces, 4, 1)
    face, _ = _gpu_ids(torch, lib, h, torch.as_tensor(verts)[None].cuda(), None, 80, 96)
    assert (face >= 0).sum() == 40 * 40


def test_full_frame_quad_cooperative_path(torch, lib):
    """one quad close to the camera covering the whole 480 x 640 frame (every tile takes the workgroup-wide path), with a small
    square in front of it"""
    W, H = 640, 480
    verts = np.array(_quad(0.5, -200, W + 200, -150, H + 150, W, H) + _quad(0.4, 100, 140, 100, 130, W, H), np.float32)
    faces = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]], np.int32)
    h = _Handle(lib, faces, 8, 1)
    face, z = _gpu_ids(torch, lib, h, torch.as_tensor(verts)[None].cuda(), None, H, W)
    assert (face >= 0).all()
    assert (np.isin(face[0, 100:130, 100:140], (2, 3))).all() and ((face[0] >= 2).sum() == 40 * 30)
    np.testing.assert_allclose(z[0][face[0] < 2], 0.5, rtol=1e-5)


def test_batch_invariance_and_determinism(torch, lib, faces, meshes):
    from hpe_amd import SMPLRenderer

    base = torch.stack([m[0] for m in meshes["meshes"]])  # 4 meshes
    g = np.random.default_rng(5)
    B = 256
    verts = base[torch.as_tensor(g.integers(0, 4, B)).cuda()].clone()
    verts += torch.as_tensor(g.normal(0, 0.02, (B, 1, 3)).astype(np.float32)).cuda()
    cams = np.tile(np.array([[500.0, 112.0, 112.0]], np.float32), (B, 1))
    cams[:, 1:] += g.uniform(-10, 10, (B, 2)).astype(np.float32)
    r = SMPLRenderer(faces=faces, max_batch=B)
    bg = torch.as_tensor(g.integers(0, 256, (B, 224, 224, 3), dtype=np.uint8)).cuda()
    full = r(verts, torch.as_tensor(cams), bg).cpu().numpy()
    for k in (0, 1, 77, 255):
        one = r(verts[k : k + 1], torch.as_tensor(cams[k : k + 1]), bg[k : k + 1]).cpu().numpy()
        np.testing.assert_array_equal(one[0], full[k])
    for _ in range(20):
        np.testing.assert_array_equal(r(verts, torch.as_tensor(cams), bg).cpu().numpy(), full)
    # B = 37 with per-image cameras, through a renderer that splits into chunks of 8
    r8 = SMPLRenderer(faces=faces, max_batch=8)
    out37 = r8(verts[:37], torch.as_tensor(cams[:37]), bg[:37])
    assert out37.is_cuda and tuple(out37.shape) == (37, 224, 224, 3)
    np.testing.assert_array_equal(out37.cpu().numpy(), full[:37])


def test_errors(torch, lib, faces):
    t = torch
    h = C.c_void_p()
    bad = faces.copy()
    bad[100, 0] = P
    assert lib.hpe_renderer_create(0, bad.ctypes.data_as(C.c_void_p), len(bad), P, 4, C.byref(h)) == 1
    assert b"outside" in lib.hpe_last_error()
    hh = _Handle(lib, faces, P, 4)
    v = t.zeros((5, P, 3), device="cuda")
    out = t.empty((5, 64, 64, 4), dtype=t.uint8, device="cuda")
    p = _params(lib)
    for Hh, Ww in ((0, 64), (64, 0), (4097, 64), (64, 4097)):
        assert lib.hpe_render(hh.h, v.data_ptr(), None, 1, Hh, Ww, None, C.byref(p), out.data_ptr(), None) == 1
        assert b"outside [1, 4096]" in lib.hpe_last_error()
    assert lib.hpe_render(hh.h, v.data_ptr(), None, 5, 64, 64, None, C.byref(p), out.data_ptr(), None) == 1  # B > max_batch
    assert b"max_batch" in lib.hpe_last_error()
    p.struct_size -= 4
    assert lib.hpe_render(hh.h, v.data_ptr(), None, 1, 64, 64, None, C.byref(p), out.data_ptr(), None) == 1
    assert b"struct_size" in lib.hpe_last_error()
    p = _params(lib, rot_axis=7)
    assert lib.hpe_render(hh.h, v.data_ptr(), None, 1, 64, 64, None, C.byref(p), out.data_ptr(), None) == 1
    # an all-NaN mesh renders as the background
    from hpe_amd import SMPLRenderer

    nan = t.full((2, P, 3), float("nan"), device="cuda")
    bg = t.randint(0, 256, (2, 64, 64, 3), dtype=t.uint8, device="cuda")
    img = SMPLRenderer(faces=faces)(nan, t.tensor([500.0, 32.0, 32.0]), bg, True)
    torch.cuda.synchronize()
    assert t.equal(img[..., :3], bg) and bool((img[..., 3] == 255).all())


def test_predictor_renderer_matches_standalone(torch, meshes):
    """Predictor.renderer is built on first access from config.smpl_face_path (reference: src/predictor.py:57-59)"""
    import hpe_amd

    p = meshes["predictor"]
    vs, cfr = meshes["meshes"][0]
    a = p.renderer(vs, cfr, meshes["frame"], True)
    assert p.renderer is p.renderer
    b = hpe_amd.SMPLRenderer(img_size=224, face_path=meshes["face_path"])(vs, cfr, meshes["frame"], True)
    assert isinstance(a, np.ndarray) and a.shape == (480, 640, 4)
    np.testing.assert_array_equal(a, b)
    c = p.renderer.rotated(vs[None], 60, cam=cfr, img_size=(480, 640))  # a batch of one: CUDA tensor out
    assert c.is_cuda and tuple(c.shape) == (1, 480, 640, 4)
    p.smpl_face_path = None
    p._renderer = None
    with pytest.raises(FileNotFoundError):
        p.renderer
