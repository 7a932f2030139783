"""Restatement of the reference's get_kcs + CriticNetwork (src/models.py:97-202) in numpy float64 and in torch: the yardstick of the
critic tests, as smpl_torch_ref.py is for the SMPL backward.  Weights are the Keras-layout dict of ``synthetic.make_critic_params`` /
``tf_checkpoint.load_critic_weights`` (``critic/<layer name>/kernel`` [in,out], ``critic/<layer name>/bias`` [out]).

    scores = [combined_dense([lrelu(kcs_dense(flat KCS)) | lrelu(joints_dense(flat J))]),
              shapes_dense_3(relu(shapes_dense_2(relu(shapes_dense_1(betas))))),
              rotation_dense_3(lrelu(rotation_dense_2(lrelu(rotation_dense_1(flat Rs[1:])))))]
    KCS = B^T B,  B = J^T C,  J = the first 14 joints,  C[b, b] = +1,  C[BONE_MINUS[b], b] = -1
    lrelu(z) = z if z > 0 else 0.2 z (tf.nn.leaky_relu's default alpha), relu(z) = max(z, 0)
"""
import numpy as np
import torch

BONE_MINUS = (1, 2, 8, 9, 3, 4, 7, 8, 12, 12, 9, 10, 13)
# (Keras layer name, in, out, activation): the table of the C ABI (hpe_critic_layer_name / hpe_critic_layer_shape)
LAYERS = (("kcs_dense", 169, 100, "leaky"), ("joints_dense", 42, 100, "leaky"), ("combined_dense", 200, 1, None),
          ("shapes_dense_1", 10, 10, "relu"), ("shapes_dense_2", 10, 5, "relu"), ("shapes_dense_3", 5, 1, None),
          ("rotation_dense_1", 207, 300, "leaky"), ("rotation_dense_2", 300, 100, "leaky"), ("rotation_dense_3", 100, 1, None))
ALPHA = 0.2


def c_matrix():
    """precompute_C_matrix: [14, 13]"""
    C = np.zeros((14, 13))
    C[np.arange(13), np.arange(13)] = 1.0
    C[np.asarray(BONE_MINUS), np.arange(13)] = -1.0
    return C


def kcs_gram(joints):
    """per-row Gram form: joints [N,K>=14,3] float64 -> [N,13,13]"""
    B = np.einsum("njc,jb->ncb", np.asarray(joints, np.float64)[:, :14], c_matrix())
    return np.einsum("nca,ncb->nab", B, B)


def kcs_literal(joints):
    """get_kcs as the reference writes it: the N x 13 x 13 x N tensordot and the diagonal over the two batch axes"""
    joints = np.asarray(joints, np.float64)[:, :14, :]
    joints_tr = np.transpose(joints, (0, 2, 1))
    B = np.tensordot(joints_tr, c_matrix(), 1)
    B_tr = np.transpose(B, (0, 2, 1))
    kcs_long = np.tensordot(B_tr, np.transpose(B_tr), 1)  # [N,13,13,N]
    kcs_diag = np.diagonal(np.transpose(kcs_long, (1, 2, 0, 3)), axis1=-2, axis2=-1)  # diag_part over the last two axes
    return np.transpose(kcs_diag, (2, 0, 1))


def kcs_grad_fold(joints, G):
    """closed form of the KCS path: G = dL/dKCS [N,13,13] -> dL/dJ [N,14,3]:  dL/dB = B (G + G^T),  dL/dJ = (dL/dB C^T)^T"""
    C = c_matrix()
    B = np.einsum("njc,jb->ncb", np.asarray(joints, np.float64)[:, :14], C)
    dB = np.einsum("nca,nab->ncb", B, G + np.transpose(G, (0, 2, 1)))
    return np.einsum("ncb,jb->njc", dB, C)


def _act_np(z, act):
    if act == "leaky":
        return np.where(z > 0, z, ALPHA * z)
    if act == "relu":
        return np.maximum(z, 0.0)
    return z


def critic_np(params, joints, betas, Rs):
    """float64 forward -> dict(scores [N,3], kcs [N,13,13], pre {layer name: pre-activation [N,out]})"""
    P = {k: np.asarray(v, np.float64) for k, v in params.items()}
    joints, betas, Rs = (np.asarray(a, np.float64) for a in (joints, betas, Rs))
    N = joints.shape[0]
    kcs = kcs_gram(joints)
    pre = {}

    def dense(i, x):
        name, _fi, _fo, act = LAYERS[i]
        z = x @ P["critic/%s/kernel" % name] + P["critic/%s/bias" % name]
        pre[name] = z
        return _act_np(z, act)

    h = np.concatenate([dense(0, kcs.reshape(N, 169)), dense(1, joints[:, :14].reshape(N, 42))], 1)
    s0 = dense(2, h)
    s1 = dense(5, dense(4, dense(3, betas)))
    s2 = dense(8, dense(7, dense(6, Rs[:, 1:].reshape(N, 207))))
    return dict(scores=np.concatenate([s0, s1, s2], 1), kcs=kcs, pre=pre)


def kink_distance(pre):
    """per row, the smallest |pre-activation| over the six layers that have a kink at 0"""
    return np.min(np.concatenate([np.abs(pre[name]) for name, _i, _o, act in LAYERS if act is not None], 1), 1)


class CriticTorch(object):
    def __init__(self, params, dtype=torch.float64, device="cpu"):
        self.dtype = dtype
        self.P = {k: torch.as_tensor(np.asarray(v), dtype=dtype, device=device) for k, v in params.items()}
        self.C = torch.as_tensor(c_matrix(), dtype=dtype, device=device)
        self.side = None

    def kcs(self, joints):
        B = torch.einsum("njc,jb->ncb", joints[:, :14], self.C)
        return torch.einsum("nca,ncb->nab", B, B)

    def _dense(self, i, x):
        name, _fi, _fo, act = LAYERS[i]
        z = x @ self.P["critic/%s/kernel" % name] + self.P["critic/%s/bias" % name]
        if act is None:
            return z
        pos = z > 0
        if self.side is not None and name in self.side:  # one-sided derivative at a kink: the caller says which side each unit is on
            pos = torch.as_tensor(self.side[name], dtype=torch.bool)
        return torch.where(pos, z, (ALPHA if act == "leaky" else 0.0) * z)

    def __call__(self, joints, betas, Rs, kcs=None, side=None):
        """kcs=None: KCS is computed from the joints (their gradient is then the total one); a kcs tensor is used as an independent input.
        side: {layer name: bool [N,out]} overrides ``z > 0`` in the named layers, which gives the one-sided gradients at a kink."""
        self.side = side
        N = joints.shape[0]
        if kcs is None:
            kcs = self.kcs(joints)
        h = torch.cat([self._dense(0, kcs.reshape(N, 169)), self._dense(1, joints[:, :14].reshape(N, 42))], 1)
        s0 = self._dense(2, h)
        s1 = self._dense(5, self._dense(4, self._dense(3, betas)))
        s2 = self._dense(8, self._dense(7, self._dense(6, Rs[:, 1:].reshape(N, 207))))
        return torch.cat([s0, s1, s2], 1)
