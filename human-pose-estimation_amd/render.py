"""SMPLRenderer -- drop-in for the reference's mesh renderer (reference: src/util/renderer.py:23-112) on the GPU.

The reference draws the predicted body with OpenDR (OpenGL, 8x MSAA) and cv2; neither is needed here: the mesh is rasterised by the
HIP kernels of ``csrc/render.hip`` (``hpe_render`` in include/hpe.h), with the reference's camera, near/far defaults, view rotation,
three Lambertian point lights, colours and alpha conventions.  What is computed is defined in DESIGN.md "Renderer"; it differs from
OpenDR in three places: no anti-aliasing (one sample per pixel centre), no clipping at the near plane (a face with a vertex in front
of it is dropped), and ``do_alpha`` without a background marks covered pixels instead of "not pure white" ones.

    r = SMPLRenderer(face_path="smpl_faces.npy")
    img = r(vert_shifted, cam_for_render, frame, True)             # one mesh, numpy frame -> numpy uint8 [H,W,4]
    imgs = r(verts_bp3, cams_b3, frames_cuda)                      # a batch of torch tensors -> CUDA uint8 [B,H,W,3]
    side = r.rotated(vert_shifted, 60, cam=cam_for_render, img_size=frame.shape[:2])
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib, assets

_AXES = {"x": 1, "y": 2, "z": 3}


class SMPLRenderer(object):
    def __init__(self, img_size=256, flength=500.0, face_path=None, faces=None, max_batch=8, device=None):
        """faces: int [F,3] array, or face_path: ``smpl_faces.npy`` / an SMPL ``.pkl`` / ``.npz`` with an ``f`` field.
        max_batch: images per library call (larger batches are rendered in chunks of this size)."""
        if faces is None:
            if face_path is None:
                raise ValueError("SMPLRenderer needs the mesh faces: pass faces= or face_path= (smpl_faces.npy, or an SMPL .pkl / .npz)")
            faces = assets.load_smpl_faces(face_path, num_verts=np.iinfo(np.int32).max)
        faces = np.asarray(faces)
        if faces.ndim != 2 or faces.shape[1] != 3 or faces.shape[0] < 1:
            raise ValueError("faces must be [F,3], got %s" % (faces.shape,))
        self.faces = np.ascontiguousarray(faces, dtype=np.int32)
        self.w = self.h = int(img_size)
        self.flength = float(flength)
        self.max_batch = int(max_batch)
        self.device = device
        self._h = None  # library handle, built for the vertex count of the first call
        self._P = None
        self._dev = None

    def __del__(self):
        if getattr(self, "_h", None):
            _lib.load().hpe_renderer_destroy(self._h)
            self._h = None

    def _handle(self, P, dev):
        if self._h is not None and self._P == P and self._dev == dev:
            return self._h
        lib = _lib.load()
        if self._h is not None:
            lib.hpe_renderer_destroy(self._h)
            self._h = None
        h = C.c_void_p()
        _lib.check(lib.hpe_renderer_create(dev, self.faces.ctypes.data_as(C.c_void_p), self.faces.shape[0], P, self.max_batch, C.byref(h)))
        self._h, self._P, self._dev = h, P, dev
        return h

    def __call__(self, verts, cam=None, img=None, do_alpha=False, far=None, near=None, color_id=0, img_size=None):
        """cam is [f, px, py] (renderer.py:42-44)."""
        return self._render(verts, cam, img, do_alpha, far, near, color_id, img_size, 0, 0.0)

    def rotated(self, verts, deg, cam=None, axis="y", img=None, do_alpha=True, far=None, near=None, color_id=0, img_size=None):
        """the mesh rotated by ``deg`` degrees about ``axis`` through its vertex mean (renderer.py:84-112)"""
        return self._render(verts, cam, img, do_alpha, far, near, color_id, img_size, _AXES.get(axis, 3), float(deg))

    def _render(self, verts, cam, img, do_alpha, far, near, color_id, img_size, rot_axis, rot_deg):
        import torch

        single = verts.dim() == 2 if isinstance(verts, torch.Tensor) else np.ndim(verts) == 2
        if isinstance(verts, torch.Tensor):
            dev = verts.device if verts.is_cuda else torch.device("cuda", self.device if self.device is not None else torch.cuda.current_device())
        else:
            dev = torch.device("cuda", self.device if self.device is not None else torch.cuda.current_device())
        v = torch.as_tensor(verts).to(dev, torch.float32)
        v = (v[None] if single else v).contiguous()
        if v.dim() != 3 or v.shape[2] != 3:
            raise ValueError("verts must be [P,3] or [B,P,3], got %s" % (tuple(v.shape),))
        B, P = v.shape[0], v.shape[1]
        # image size (renderer.py:45-51)
        if img is not None:
            H, W = int(img.shape[-3]), int(img.shape[-2])
        elif img_size is not None:
            H, W = int(img_size[0]), int(img_size[1])
        else:
            H, W = self.h, self.w
        if cam is None:
            cam = [self.flength, W / 2.0, H / 2.0]  # renderer.py:53-54
        c = torch.as_tensor(np.asarray(cam.detach().cpu() if isinstance(cam, torch.Tensor) else cam, np.float32)).reshape(-1, 3)
        if c.shape[0] == 1:
            c = c.expand(B, 3)
        if c.shape[0] != B:
            raise ValueError("cam must be [3] or [B,3] with B = %d, got %s" % (B, tuple(c.shape)))
        c = c.to(dev).contiguous()
        bg = None
        if img is not None:
            bg = _background(img, dev)
            bg = (bg[None] if bg.dim() == 3 else bg).contiguous()
            if bg.shape[0] == 1 and B > 1:
                bg = bg.expand(B, H, W, 3).contiguous()
            if tuple(bg.shape) != (B, H, W, 3):
                raise ValueError("img must be [H,W,3] or [B,H,W,3] matching %d meshes, got %s" % (B, tuple(img.shape)))
        p = _lib.HpeRenderParams()
        lib = _lib.load()
        lib.hpe_render_params_init(C.byref(p))
        p.color_id = int(color_id or 0)
        p.do_alpha = 1 if do_alpha else 0
        p.rot_axis, p.rot_deg = rot_axis, rot_deg
        p.near = -1.0 if near is None else float(near)
        p.far = -1.0 if far is None else float(far)
        out = torch.empty((B, H, W, 4 if do_alpha else 3), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            h = self._handle(P, dev.index)
            st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            for lo in range(0, B, self.max_batch):
                n = min(self.max_batch, B - lo)
                _lib.check(lib.hpe_render(h, v[lo].data_ptr(), c[lo].data_ptr(), n, H, W, None if bg is None else bg[lo].data_ptr(),
                                          C.byref(p), out[lo].data_ptr(), st))
        if single:
            return out[0].cpu().numpy()
        return out


def _background(img, dev):
    """uint8 as is; a float frame in [0, 1] as round(255 x) (renderer.py:217 hands OpenDR img / 255 when img.max() > 1, else img)"""
    import torch

    t = torch.as_tensor(img) if not isinstance(img, torch.Tensor) else img
    t = t.to(dev)
    if t.dtype == torch.uint8:
        return t
    t = t.float()
    if float(t.max()) <= 1.0:
        t = t * 255.0
    return torch.round(t).clamp_(0, 255).to(torch.uint8)
