"""3-D supervision without a GPU (DESIGN.md "3-D supervision"): the mirror rule of the labels in both formats, the float64 reference of
hpe_loss3d checked against itself, the masks ``gt3d_real`` builds, the draws ``load_training_batch_3d`` makes, the Trainer's new config
keys, and the argument refusals of the two C calls (they come before any HIP call)."""
import ctypes as C
import sys
import types

import numpy as np
import pytest
import torch

import hpe_amd

import loss3d_ref as LR

# the package's own modules, by the functions it exports (``hpe_amd`` is an alias of a package whose name is no identifier: a dotted
# import through the alias elsewhere in the suite makes second copies of submodules, and the attributes of the alias may name those)
augment, records = sys.modules[hpe_amd.gt3d_real.__module__], sys.modules[hpe_amd.load_training_batch_3d.__module__]


def rodrigues64(v):
    """[N,3] float64 axis-angle -> [N,3,3]"""
    v = np.asarray(v, np.float64)
    out = np.empty((v.shape[0], 3, 3))
    for i, w in enumerate(v):
        a = np.linalg.norm(w)
        k = w / a if a > 0 else np.zeros(3)
        Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        out[i] = np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * (Kx @ Kx)
    return out


random_case = LR.random_case


# ---------------------------------------------------------------------------------------------- the mirror
def test_the_permutations_are_involutions_and_the_kernels_own():
    assert tuple(augment.SWAP14) == tuple(augment.SWAP_INDS[:14]) == tuple(LR.SWAP14)
    assert tuple(augment.PERM24) == tuple(LR.PERM24) == (0, 2, 1, 3, 5, 4, 6, 8, 7, 9, 11, 10, 12, 14, 13, 15, 17, 16, 19, 18, 21, 20, 23, 22)
    for p in (augment.SWAP14, augment.PERM24):
        assert [p[p[i]] for i in range(len(p))] == list(range(len(p)))


def test_reflect_pose_is_the_rotation_space_rule():
    g = np.random.RandomState(0)
    M = np.diag([-1.0, 1.0, 1.0])
    for scale in (0.3, 2.0):
        pose = scale * g.randn(5, 72)
        R = rodrigues64(pose.reshape(-1, 3)).reshape(5, 24, 3, 3)
        Rm = rodrigues64(augment.reflect_pose(pose).reshape(-1, 3)).reshape(5, 24, 3, 3)
        for j in range(24):
            assert np.abs(Rm[:, j] - M @ R[:, augment.PERM24[j]] @ M).max() <= 1e-12
        # M R M negates exactly the entries (0,1), (0,2), (1,0), (2,0): what the kernel does
        sign = np.ones((3, 3))
        sign[0, 1] = sign[0, 2] = sign[1, 0] = sign[2, 0] = -1
        assert np.array_equal(M @ R[0, 3] @ M, sign * R[0, 3])
        assert np.array_equal(augment.reflect_pose(augment.reflect_pose(pose)), pose)
    assert augment.reflect_pose(np.zeros(72, np.float32)).dtype == np.float32
    with pytest.raises(ValueError):
        augment.reflect_pose(np.zeros(71))


def test_reflect_joints3d():
    g = np.random.RandomState(1)
    j = g.randn(3, 14, 3).astype(np.float32)
    m = augment.reflect_joints3d(j)
    assert np.array_equal(augment.reflect_joints3d(m), j) and m.dtype == np.float32
    assert np.array_equal(m[:, 0], j[:, 5] * np.float32([-1, 1, 1])) and np.array_equal(m[:, 12], j[:, 12] * np.float32([-1, 1, 1]))
    # the reference's mirror of the ground truth is this function and reflect_pose's rule
    gj, gR = LR.mirror_gt(torch.from_numpy(j), torch.zeros(3, 24, 3, 3), np.array([True, False, True]))
    assert np.array_equal(gj.numpy()[0], m[0]) and np.array_equal(gj.numpy()[1], j[1])
    with pytest.raises(ValueError):
        augment.reflect_joints3d(np.zeros((14, 2)))


# ---------------------------------------------------------------------------------------------- the reference against itself
def test_reference_gradient_by_finite_differences():
    c = random_case(2)
    c["w_joints"][3] = 0.0
    c["w_smpl"][2] = 0.0
    sj, ss = 0.37, 1.9
    out = LR.run(**c, scale_j=sj, scale_s=ss)

    def value(**changed):
        o = LR.run(**dict(c, **changed))["parts"]
        return sj * o[0] + ss * (o[1] + o[2])

    g = np.random.RandomState(3)
    h = 1e-6
    for name, key in (("joints", "grad_joints"), ("Rs", "grad_Rs"), ("betas", "grad_betas")):
        for _ in range(3):
            d = g.randn(*c[name].shape)
            fd = (value(**{name: c[name].astype(np.float64) + h * d}) - value(**{name: c[name].astype(np.float64) - h * d})) / (2 * h)
            assert abs(fd - (out[key] * d).sum()) <= 1e-7 * max(1.0, abs(fd)), name
    # the hip term: the gradient of a hip joint is NOT 2 s w e, and the closed form of include/hpe_loss3d.h is what autograd gives
    gj, _ = LR.mirror_gt(torch.from_numpy(c["joints_gt"]).double(), torch.zeros(4, 24, 3, 3, dtype=torch.float64), c["flip"])
    p, gj = c["joints"][:, :14].astype(np.float64), gj.numpy()
    e = (p - 0.5 * (p[:, 2:3] + p[:, 3:4])) - (gj - 0.5 * (gj[:, 2:3] + gj[:, 3:4]))
    want = e.copy()
    want[:, 2:4] -= 0.5 * e.sum(1, keepdims=True)
    want *= 2 * sj * c["w_joints"].astype(np.float64)[:, None, None]
    assert np.abs(out["grad_joints"][:, :14] - want).max() <= 1e-12 and (out["grad_joints"][:, 14:] == 0).all()
    assert np.abs(out["grad_joints"][0, 2] - 2 * sj * c["w_joints"][0] * e[0, 2]).max() > 1e-3  # leaving the hip term out is visible
    assert (out["grad_joints"][3] == 0).all() and (out["grad_Rs"][2] == 0).all() and (out["grad_betas"][2] == 0).all()


def test_reference_with_all_weights_zero_and_nan_labels():
    c = random_case(4)
    c["w_joints"][:] = 0
    c["w_smpl"][:] = 0
    c["joints_gt"][:] = np.nan
    c["Rs_gt"][:] = np.nan
    c["shape_gt"][:] = np.nan
    out = LR.run(**c)
    assert all((v == 0).all() for v in out.values())
    lj, ls = LR.losses_of(torch.from_numpy(out["parts"]))
    assert float(lj) == 0.0 and float(ls) == 0.0


# ---------------------------------------------------------------------------------------------- gt3d_real
class FakeEngine(object):
    """engine.smpl faked: joints and Rs that name the row's pose, so the test can tell where a value came from"""
    tdev, max_batch = torch.device("cpu"), 2

    def __init__(self):
        self.calls = []

    def smpl(self, theta, want):
        assert tuple(want) == ("joints", "Rs") and not torch.is_grad_enabled() and theta.shape[0] <= self.max_batch
        self.calls.append(theta.clone())
        B = theta.shape[0]
        return {"joints": theta[:, 3:4, None].expand(B, 19, 3) + 100.0, "Rs": theta[:, 3:4, None, None].expand(B, 24, 3, 3) + 200.0}


def test_gt3d_real_masks():
    g = np.random.RandomState(5)
    j = g.randn(5, 14, 3).astype(np.float32)
    pose, shape = g.randn(5, 72).astype(np.float32), g.randn(5, 10).astype(np.float32)
    recs = [{"gt3d": j[0], "pose": pose[0], "shape": shape[0]},  # all three
            {},  # none
            {"gt3d": j[2]},  # joints only
            {"pose": pose[3], "shape": shape[3]},  # SMPL only: the joints come from the same engine.smpl pass
            {"gt3d": j[4], "pose": pose[4]}]  # a pose without a shape is no SMPL label
    eng = FakeEngine()
    flip = torch.tensor([True, False, False, True, False])
    gt = augment.gt3d_real(eng, recs, flip)
    assert isinstance(gt, hpe_amd.Gt3D)
    assert gt.w_joints.tolist() == [1, 0, 1, 1, 1] and gt.w_smpl.tolist() == [1, 0, 0, 1, 0]
    assert [c.shape[0] for c in eng.calls] == [2, 2, 1]  # one pass, in chunks of max_batch
    theta = torch.cat(eng.calls)
    assert torch.equal(theta[:, :3], torch.tensor([[1.0, 0, 0]]).expand(5, 3)) and np.array_equal(theta[0, 3:75].numpy(), pose[0])
    assert np.array_equal(theta[3, 75:].numpy(), shape[3]) and (theta[1, 3:] == 0).all() and (theta[4, 3:] == 0).all()
    assert np.array_equal(gt.joints[0].numpy(), j[0]) and (gt.joints[1] == 0).all() and np.array_equal(gt.joints[2].numpy(), j[2])
    assert (gt.joints[3] == np.float32(pose[3, 0]) + np.float32(100.0)).all() and gt.joints.shape == (5, 14, 3)
    assert (gt.Rs[0] == np.float32(pose[0, 0]) + np.float32(200.0)).all() and gt.Rs.shape == (5, 24, 3, 3)
    assert np.array_equal(gt.shape[3].numpy(), shape[3]) and (gt.shape[4] == 0).all()
    assert gt.flip.dtype == torch.bool and gt.flip.tolist() == flip.tolist()  # the labels stay unflipped: the draw travels with them
    assert [t.dtype for t in gt[:5]] == [torch.float32] * 5
    # no record holds a pose: engine.smpl is not called at all
    eng = FakeEngine()
    gt = augment.gt3d_real(eng, [{"gt3d": j[0]}, {}])
    assert not eng.calls and gt.flip is None and gt.w_joints.tolist() == [1, 0] and gt.w_smpl.tolist() == [0, 0] and (gt.Rs == 0).all()
    # stacked arrays
    gt = augment.gt3d_real(FakeEngine(), {"pose": pose[:2], "shape": shape[:2]})
    assert gt.w_joints.tolist() == [1, 1] and gt.w_smpl.tolist() == [1, 1] and (gt.joints[1] == np.float32(pose[1, 0]) + np.float32(100.0)).all()
    with pytest.raises(ValueError):
        augment.gt3d_real(FakeEngine(), [])


# ---------------------------------------------------------------------------------------------- load_training_batch_3d
def test_load_training_batch_3d_draws_as_load_training_batch_does(monkeypatch):
    seen = {}

    def fake_load(recs, draws=None, generator=None, threads=None, **kw):
        assert generator is None  # the draws are made before: augment_batch must not draw again
        seen["draws"], seen["kw"] = draws, kw
        return "images", "segs", "kp"

    def fake_gt(engine, recs, flip):
        seen["flip"], seen["engine"] = flip, engine
        return "gt"

    monkeypatch.setattr(records, "load_training_batch", fake_load)
    monkeypatch.setattr(augment, "gt3d_real", fake_gt)
    recs = [{"kp": None}] * 3
    for kw in ({}, {"trans_max": 7, "scale_range": (0.9, 1.1)}, {"trans_max": 0}):
        g1, g2 = torch.Generator().manual_seed(11), torch.Generator().manual_seed(11)
        out = records.load_training_batch_3d(recs, "engine", generator=g1, **kw)
        want = augment.draw_augmentation(3, generator=g2, **{k: kw[k] for k in ("trans_max", "scale_range") if k in kw})  # augment_batch's own call
        assert out == ("images", "segs", "kp", "gt") and seen["engine"] == "engine" and seen["kw"] == kw
        assert all(torch.equal(seen["draws"][k], want[k]) for k in ("trans", "scale", "flip")) and seen["flip"] is seen["draws"]["flip"]
        assert torch.equal(g1.get_state(), g2.get_state())  # the generator is left where load_training_batch would leave it
    mine = augment.draw_augmentation(3, generator=torch.Generator().manual_seed(2))
    g1 = torch.Generator().manual_seed(11)
    records.load_training_batch_3d(recs, "engine", draws=mine, generator=g1)
    assert seen["draws"] is mine and torch.equal(g1.get_state(), torch.Generator().manual_seed(11).get_state())
    with pytest.raises(ValueError):
        records.load_training_batch_3d([], "engine")


# ---------------------------------------------------------------------------------------------- Trainer
def bare_trainer(**cfg):
    """the part of Trainer.__init__ that reads the 3-D keys, on an object that never built an engine"""
    tr = hpe_amd.Trainer.__new__(hpe_amd.Trainer)
    g = lambda name, default: cfg.get(name, default)  # noqa: E731
    tr.joints3d_loss_weight, tr.smpl_loss_weight = float(g("joints3d_loss_weight", 0.0)), float(g("smpl_loss_weight", 0.0))
    tr.use_3d_loss = tr.joints3d_loss_weight > 0.0 or tr.smpl_loss_weight > 0.0
    tr.engine, tr._aug = "engine", torch.Generator().manual_seed(0)
    return tr


def test_trainer_reads_the_keys_and_selects_the_loader(monkeypatch):
    import inspect

    src = inspect.getsource(hpe_amd.Trainer.__init__)
    assert 'g("joints3d_loss_weight", 0.0)' in src and 'g("smpl_loss_weight", 0.0)' in src  # read from the config, default 0
    assert 'self.use_3d_loss = self.joints3d_loss_weight > 0.0 or self.smpl_loss_weight > 0.0' in src
    calls = []
    monkeypatch.setattr(records, "load_training_batch", lambda recs, **kw: calls.append(("2d", sorted(kw))) or (1, 2, 3))
    monkeypatch.setattr(records, "load_training_batch_3d", lambda recs, eng, **kw: calls.append(("3d", eng, sorted(kw))) or (1, 2, 3, 4))
    recs = [b"x", b"y"]
    off = bare_trainer()
    assert off._load_images(recs, with_3d=True) == (1, 2, 3) and off._load_images(recs, augment=False, with_3d=True) == (1, 2, 3)
    assert calls == [("2d", ["generator"]), ("2d", ["draws"])]  # both weights 0: the old loader, whatever the caller asks for
    del calls[:]
    for kw in ({"joints3d_loss_weight": 0.5}, {"smpl_loss_weight": 2.0}):
        on = bare_trainer(**kw)
        assert on._load_images(recs, with_3d=True) == (1, 2, 3, 4) and on._load_images(recs) == (1, 2, 3)  # scoring passes load no 3-D labels
    assert calls == [("3d", "engine", ["generator"]), ("2d", ["generator"])] * 2
    ready = tuple(types.SimpleNamespace(is_cuda=True) for _ in range(3))
    assert on._load_images(ready, with_3d=True) == ready + (None,) and on._load_images(ready + ("gt",), with_3d=True)[3] == "gt"
    assert off._load_images(ready + ("gt",), with_3d=True) == ready


def test_generator_trainer_has_the_weights_and_the_argument():
    import inspect

    sig = inspect.signature(hpe_amd.GeneratorTrainer.__init__).parameters
    assert sig["joints3d_loss_weight"].default == 0.0 and sig["smpl_loss_weight"].default == 0.0
    assert inspect.signature(hpe_amd.GeneratorTrainer.step).parameters["gt3d"].default is None
    for name in ("Gt3D", "joints3d_loss", "smpl_param_loss", "loss3d_counts", "gt3d_real", "reflect_pose", "reflect_joints3d",
                 "load_training_batch_3d", "Loss3DFunction"):
        assert hasattr(hpe_amd, name), name


# ---------------------------------------------------------------------------------------------- the C ABI
def test_extension_header_binding_and_library_agree():
    """include/hpe_loss3d.h, the binding's table of it and the library name the same functions with the same argument counts; hpe.h
    includes the header, and the core list of entry points is not touched by it"""
    import os
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "hpe_loss3d.h")).read(), flags=re.S)
    decls = dict(re.findall(r"\bint\s+(hpe_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", txt))
    _lib = hpe_amd._lib
    assert sorted(decls) == _lib.loss3d_symbols() == sorted(re.findall(r"\b(hpe_[a-z0-9_]+)\s*\(", txt))
    lib = _lib.load()
    for name, args in decls.items():
        fn = getattr(lib, name)  # exported
        assert fn.restype is C.c_int and len(fn.argtypes) == len(args.split(",")), name
        for ctype, decl in zip(fn.argtypes, args.split(",")):
            want = C.c_int if re.match(r"\s*int\s+\w+$", decl) else C.POINTER(C.c_void_p) if "* const*" in decl else C.c_void_p
            assert ctype is want, (name, decl)
    core = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "hpe.h")).read(), flags=re.S)
    assert re.search(r'^#include "hpe_loss3d.h"$', core, flags=re.M)
    assert not set(decls) & set(_lib.declared_symbols())


# ---------------------------------------------------------------------------------------------- the C calls' refusals
def test_argument_errors_need_no_device():
    lib = hpe_amd._lib.load()
    assert hpe_amd._lib.loss3d_symbols() == ["hpe_loss3d", "hpe_loss3d_backward"]
    one = (C.c_void_p * 1)(8)
    d = 8  # never dereferenced: every refusal comes before the launch

    def fwd(joints=one, Rs=one, betas=one, stride=10, gj=d, gR=d, gs=d, wj=d, ws=d, n=1, B=2, K=19, parts=d):
        return lib.hpe_loss3d(joints, Rs, betas, stride, gj, gR, gs, wj, ws, None, n, B, K, parts, None, None)

    def bwd(joints=one, stride=85, n=1, B=2, K=14, sj=d, ss=d, out=(one, one, one)):
        return lib.hpe_loss3d_backward(joints, one, one, stride, d, d, d, d, d, None, n, B, K, sj, ss, *out, None)

    null_entry = (C.c_void_p * 1)(None)
    cases = [(fwd, dict(joints=None), "NULL"), (fwd, dict(betas=null_entry), r"\[0\]"), (fwd, dict(gR=None), "NULL"), (fwd, dict(ws=None), "NULL"),
             (fwd, dict(n=0), "n_stage 0"), (fwd, dict(n=17), "n_stage 17"), (fwd, dict(B=0), "batch 0"), (fwd, dict(K=13), "K 13"),
             (fwd, dict(K=25), "K 25"), (fwd, dict(stride=9), "betas_stride 9"), (fwd, dict(parts=None), "parts_dev"),
             (bwd, dict(out=(None, None, None)), "every output"), (bwd, dict(out=(one, None, None), sj=None), "scale_j"),
             (bwd, dict(out=(None, one, None), ss=None), "scale_s"), (bwd, dict(out=(null_entry, None, None)), "stage 0"),
             (bwd, dict(K=30), "K 30"), (bwd, dict(stride=0), "betas_stride 0"), (bwd, dict(joints=None), "NULL")]
    import re

    for f, kw, pattern in cases:
        rc = f(**kw)
        msg = lib.hpe_last_error().decode()
        assert rc == 1 and msg.startswith(f is fwd and "hpe_loss3d:" or "hpe_loss3d_backward:") and re.search(pattern, msg), (kw, rc, msg)
