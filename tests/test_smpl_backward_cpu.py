"""CPU checks behind the SMPL backward: the torch restatement used as the gradient reference equals the numpy oracle, its
gradients are finite at the mean pose, and the C ABI carries hpe_smpl_backward / hpe_kp_loss_backward."""
import ctypes as C

import numpy as np
import torch

from hpe_amd import _lib, build as hbuild
from oracle import hmr_oracle as O

from smpl_torch_ref import SmplTorch, make_theta


def test_restatement_forward_equals_oracle(smpl_model):
    th = make_theta(4, seed=0).astype(np.float64)
    ref = O.SMPL(smpl_model, dtype=np.float64)
    verts, joints, Rs = ref(th[:, 75:], th[:, 3:75], get_skin=True)
    kp2d = O.batch_orth_proj_idrot(joints, th[:, :3])
    out = SmplTorch(smpl_model, torch.float64)(torch.from_numpy(th))
    # the restatement holds the float32-rounded constants, as the oracle does for a float32 model dict
    for name, want in (("verts", verts), ("joints", joints), ("J_transformed", ref.J_transformed), ("kp2d", kp2d), ("Rs", Rs)):
        got = out[name].numpy()
        rel = np.abs(got - want).max() / np.abs(want).max()
        assert rel <= 1e-12, (name, rel)


def test_restatement_gradients_finite_at_mean_pose(smpl_model):
    th = torch.from_numpy(make_theta(3, seed=1))
    assert float(th[0, 6:75].abs().max()) == 0.0  # 23 joints exactly zero
    for dtype in (torch.float64, torch.float32):
        x = th.to(dtype).requires_grad_(True)
        out = SmplTorch(smpl_model, dtype)(x)
        g = torch.Generator().manual_seed(2)
        sum((out[k] * torch.randn(out[k].shape, generator=g, dtype=torch.float64).to(dtype)).sum() for k in sorted(out)).backward()
        assert torch.isfinite(x.grad).all()
        assert float(x.grad[0, 6:75].abs().max()) > 0.0


def test_backward_symbols_and_state_error():
    """hpe_smpl_backward / hpe_kp_loss_backward are exported with the declared signatures; where a ctx can be created (a GPU is
    visible) a ctx that was not finalized answers HPE_ERR_STATE, and argument errors are refused before any launch."""
    hbuild.build()
    lib = _lib.load()
    assert "hpe_smpl_backward" in _lib.declared_symbols() and "hpe_kp_loss_backward" in _lib.declared_symbols()
    assert lib.hpe_smpl_backward.argtypes == [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(_lib.HpeOutputs), C.c_void_p, C.c_void_p]
    assert lib.hpe_kp_loss_backward.argtypes == [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    assert lib.hpe_smpl_backward.restype == C.c_int and lib.hpe_kp_loss_backward.restype == C.c_int
    o = _lib.HpeOutputs()
    assert lib.hpe_smpl_backward(None, None, 1, C.byref(o), None, None) == 1  # HPE_ERR_INVALID: null ctx
    assert lib.hpe_kp_loss_backward(None, None, 1, 19, None, None, None) == 1
    cfg = _lib.HpeConfig()
    lib.hpe_config_init(C.byref(cfg))
    h = C.c_void_p()
    rc = lib.hpe_create(C.byref(cfg), C.byref(h))
    assert rc in (0, 4), rc  # 4 = HPE_ERR_NO_DEVICE (no GPU visible)
    if rc == 0:
        try:
            dummy = C.c_void_p(16)  # never dereferenced: the state check comes first
            assert lib.hpe_smpl_backward(h, dummy, 1, C.byref(o), dummy, None) == 3  # HPE_ERR_STATE
        finally:
            lib.hpe_destroy(h)
