"""Restatement of the encoder's training backward with frozen BatchNorm statistics (DESIGN.md "Encoder training"), in torch on the CPU, in
the dtype of its inputs (float64: the reference; float32: the error budget).  Tensors are NHWC, kernels HWIO, as in the library.

Per layer, s = gamma / sqrt(var + eps):  y = act(s * (conv(x, W) + b - mean) + beta (+ residual)),  dz = dy * [y > 0],
G = A^T dz (A = im2col of x),  dW = s * G,  dshift = sum_m dz,  dbeta = dshift,  db = s * dshift,
dgamma = (<W[:,n], G[:,n]> + (b - mean) * dshift) / sqrt(var + eps),  dx = (dz * s) . W^T."""
import numpy as np
import torch
import torch.nn.functional as F

from hpe_amd.resnet_spec import CONV_SPECS, ENCODER_PARAM_FLOATS, ENCODER_PARAM_OFFSETS, STAGE_BLOCKS

EPS = 1e-3


def layer_tensors(params, s, dtype=torch.float64):
    keys = (s.name + "/kernel", s.name + "/bias", s.bn_name + "/gamma", s.bn_name + "/beta", s.bn_name + "/moving_mean", s.bn_name + "/moving_variance")
    return [torch.as_tensor(np.asarray(params[k])).to(dtype) for k in keys]


def im2col(s, x):
    """x [B,H,H,C] -> A [B*Ho*Ho, kh*kw*C], k = (kh, kw, c) with c fastest; SAME-style pad (k - 1) / 2"""
    B = x.shape[0]
    u = F.unfold(x.permute(0, 3, 1, 2), (s.kh, s.kw), padding=(s.kh - 1) // 2, stride=s.stride)  # [B, C*kh*kw, L]
    u = u.reshape(B, s.cin, s.kh * s.kw, -1).permute(0, 3, 2, 1)
    return u.reshape(B * s.hout * s.hout, s.kh * s.kw * s.cin)


def layer_forward(s, x, lt, residual=None, relu=True):
    W, b, gamma, beta, mean, var = lt
    sc = gamma / torch.sqrt(var + EPS)
    z = im2col(s, x) @ W.reshape(-1, s.cout)
    y = (sc * (z + b - mean) + beta).reshape(x.shape[0], s.hout, s.hout, s.cout)
    if residual is not None:
        y = y + residual
    return torch.relu(y) if relu else y


def layer_backward(s, x, y, dy, lt, want_dx=True, gated=True):
    """y: the layer's output (only its sign is used; gated False: no activation) -> dict dx, dW, db, dgamma, dbeta, dz"""
    W, b, gamma, beta, mean, var = lt
    istd = 1.0 / torch.sqrt(var + EPS)
    sc = gamma * istd
    dz = dy * (y > 0).to(dy.dtype) if gated else dy
    dzm = dz.reshape(-1, s.cout)
    G = im2col(s, x).t() @ dzm
    dshift = dzm.sum(0)
    Wm = W.reshape(-1, s.cout)
    out = {"dW": (sc * G).reshape(W.shape), "db": sc * dshift, "dbeta": dshift, "dgamma": ((Wm * G).sum(0) + (b - mean) * dshift) * istd, "dz": dz}
    if want_dx and s.kh != 7:
        dzs = dz * sc
        B = x.shape[0]
        if s.kh == 1:
            lo = (dzs.reshape(-1, s.cout) @ Wm.t()).reshape(B, s.hout, s.hout, s.cin)
            if s.stride == 1:
                out["dx"] = lo
            else:
                hi = torch.zeros(B, s.hin, s.hin, s.cin, dtype=dy.dtype)
                hi[:, ::2, ::2, :] = lo
                out["dx"] = hi
        else:  # SAME convolution with the spatially flipped, channel-transposed kernel
            wf = torch.flip(W, (0, 1)).permute(2, 3, 0, 1)  # [cin][cout][kh][kw] = OIHW of the transposed convolution
            out["dx"] = F.conv2d(dzs.permute(0, 3, 1, 2), wf, padding=1).permute(0, 2, 3, 1)
    return out


def layer_grad_flat(r):
    return torch.cat([r["dW"].reshape(-1), r["db"], r["dgamma"], r["dbeta"]])


def maxpool_winners(x):
    """x [B,H,H,C] -> (wy, wx) [B,H/2,H/2,C]: the first maximum of every zero-padded 3x3 / stride 2 window in row-major order; -1 where the
    pad wins"""
    B, H, _, C = x.shape
    Ho = H // 2
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    best = None
    for dy in range(3):
        for dx in range(3):
            v = xp[:, dy:dy + 2 * Ho:2, dx:dx + 2 * Ho:2, :]
            yy = (2 * torch.arange(Ho) - 1 + dy).view(1, Ho, 1, 1).expand(B, Ho, Ho, C)
            xx = (2 * torch.arange(Ho) - 1 + dx).view(1, 1, Ho, 1).expand(B, Ho, Ho, C)
            inb = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < H)
            yy, xx = torch.where(inb, yy, -1), torch.where(inb, xx, -1)
            if best is None:
                best, wy, wx = v.clone(), yy.clone(), xx.clone()
            else:
                m = v > best
                best, wy, wx = torch.where(m, v, best), torch.where(m, yy, wy), torch.where(m, xx, wx)
    return wy, wx


def maxpool_backward(winners, dy, H):
    wy, wx = winners
    B, Ho, _, C = dy.shape
    dx = torch.zeros(B * H * H * C, dtype=dy.dtype)
    ok = wy >= 0
    b = torch.arange(B).view(B, 1, 1, 1).expand_as(wy)
    c = torch.arange(C).view(1, 1, 1, C).expand_as(wy)
    idx = ((b * H + wy) * H + wx) * C + c
    dx.index_add_(0, idx[ok], dy[ok])
    return dx.reshape(B, H, H, C)


def avgpool_backward(dy, HW):
    return (dy / HW).unsqueeze(1).expand(dy.shape[0], HW, dy.shape[1]).contiguous()


def blocks():
    """[(i2a, i2b, i2c, i1 or None)] in network order"""
    out, ci = [], 1
    for stage in (2, 3, 4, 5):
        for b in range(STAGE_BLOCKS[stage]):
            out.append((ci, ci + 1, ci + 2, ci + 3 if b == 0 else None))
            ci += 4 if b == 0 else 3
    return out


def network_backward(params, images, stash, pooled, winners, grad_features, dtype=torch.float64):
    """the whole-network backward driven by the stash: stash[i] the output of layer i (its sign is the gate), pooled the max-pooled map,
    winners = maxpool_winners(stash[0]) -> the flat gradient [ENCODER_PARAM_FLOATS] and the per-layer results"""
    flat = torch.zeros(ENCODER_PARAM_FLOATS, dtype=dtype)

    def put(i, r):
        o = ENCODER_PARAM_OFFSETS[i][0]
        v = layer_grad_flat(r)
        flat[o:o + v.numel()] = v

    lt = [layer_tensors(params, s, dtype) for s in CONV_SPECS]
    B = images.shape[0]
    g = avgpool_backward(grad_features.to(dtype), 49).reshape(B, 7, 7, 2048)
    bl = blocks()
    for k in range(len(bl) - 1, -1, -1):
        i2a, i2b, i2c, i1 = bl[k]
        xin = (pooled if k == 0 else stash[bl[k - 1][2]]).to(dtype)
        rc = layer_backward(CONV_SPECS[i2c], stash[i2b].to(dtype), stash[i2c], g, lt[i2c])
        put(i2c, rc)
        rb = layer_backward(CONV_SPECS[i2b], stash[i2a].to(dtype), stash[i2b], rc["dx"], lt[i2b])
        put(i2b, rb)
        ra = layer_backward(CONV_SPECS[i2a], xin, stash[i2a], rb["dx"], lt[i2a])
        put(i2a, ra)
        if i1 is None:
            g = ra["dx"] + rc["dz"]
        else:
            r1 = layer_backward(CONV_SPECS[i1], xin, None, rc["dz"], lt[i1], gated=False)
            put(i1, r1)
            g = ra["dx"] + r1["dx"]
    g = maxpool_backward(winners, g, 112)
    put(0, layer_backward(CONV_SPECS[0], images.to(dtype), stash[0], g, lt[0], want_dx=False))
    return flat


def rel(a, b):
    a, b = torch.as_tensor(a).double().reshape(-1), torch.as_tensor(b).double().reshape(-1)
    return float(torch.linalg.norm(a - b) / torch.linalg.norm(b))


def split_layer_grad(s, v):
    kn = s.kh * s.kw * s.cin * s.cout
    return {"dW": v[:kn], "db": v[kn:kn + s.cout], "dgamma": v[kn + s.cout:kn + 2 * s.cout], "dbeta": v[kn + 2 * s.cout:kn + 3 * s.cout]}
