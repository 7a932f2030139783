"""Restatement of encoder training with batch statistics (DESIGN.md "Encoder training with batch statistics"), in torch on the CPU, in the
dtype of its inputs (float64: the reference; float32: the error budget).  Tensors are NHWC, kernels HWIO, as in the library.

Per layer, M = B * hout * hout rows:  z = conv(x, W) + b,  mu = mean_m z,  var = mean_m (z - mu)^2,  r = 1 / sqrt(var + eps),
xhat = (z - mu) * r,  y = act(gamma * xhat + beta (+ residual)).
dz = dy * [y > 0],  dbeta = sum_m dz,  dgamma = sum_m dz * xhat,  dzraw = gamma * r * (dz - dbeta / M - xhat * dgamma / M),
dW = A^T dzraw,  dx = dzraw . W^T,  db = 0 (the bias cancels in z - mu)."""
import torch
import torch.nn.functional as F

from encoder_train_ref import EPS, avgpool_backward, blocks, im2col, layer_grad_flat, layer_tensors, maxpool_backward, rel  # noqa: F401
from hpe_amd.resnet_spec import CONV_SPECS, ENCODER_PARAM_FLOATS, ENCODER_PARAM_OFFSETS, ENCODER_STAT_CHANNELS, ENCODER_STAT_OFFSETS


def batch_stats(z):
    """z [..., N] -> (mu, var) over every axis but the last; the biased variance"""
    zm = z.reshape(-1, z.shape[-1])
    mu = zm.mean(0)
    return mu, ((zm - mu) ** 2).mean(0)


def layer_raw(s, x, lt):
    W, b = lt[0], lt[1]
    return (im2col(s, x) @ W.reshape(-1, s.cout) + b).reshape(x.shape[0], s.hout, s.hout, s.cout)


def layer_apply(z, mu, var, gamma, beta, residual=None, relu=True):
    y = gamma * ((z - mu) * (1.0 / torch.sqrt(var + EPS))) + beta
    if residual is not None:
        y = y + residual
    return torch.relu(y) if relu else y


def layer_forward(s, x, lt, residual=None, relu=True):
    """-> (y, z, mu, var)"""
    z = layer_raw(s, x, lt)
    mu, var = batch_stats(z)
    return layer_apply(z, mu, var, lt[2], lt[3], residual, relu), z, mu, var


def layer_backward(s, x, z, y, dy, lt, want_dx=True, gated=True):
    """z: the layer's raw output (the statistics and xhat come from it), y: its activated output (only its sign is used; gated False: no
    activation) -> dict dx, dW, db, dgamma, dbeta, dz"""
    W, gamma = lt[0], lt[2]
    mu, var = batch_stats(z)
    r = 1.0 / torch.sqrt(var + EPS)
    xhat = ((z - mu) * r).reshape(-1, s.cout)
    dz = dy * (y > 0).to(dy.dtype) if gated else dy
    dzm = dz.reshape(-1, s.cout)
    M = dzm.shape[0]
    dbeta = dzm.sum(0)
    dgamma = (dzm * xhat).sum(0)
    dzraw = gamma * r * (dzm - dbeta / M - xhat * dgamma / M)
    Wm = W.reshape(-1, s.cout)
    out = {"dW": (im2col(s, x).t() @ dzraw).reshape(W.shape), "db": torch.zeros_like(dbeta), "dbeta": dbeta, "dgamma": dgamma, "dz": dz}
    if want_dx and s.kh != 7:
        B = x.shape[0]
        dzr = dzraw.reshape(B, s.hout, s.hout, s.cout)
        if s.kh == 1:
            lo = (dzraw @ Wm.t()).reshape(B, s.hout, s.hout, s.cin)
            if s.stride == 1:
                out["dx"] = lo
            else:
                hi = torch.zeros(B, s.hin, s.hin, s.cin, dtype=dy.dtype)
                hi[:, ::2, ::2, :] = lo
                out["dx"] = hi
        else:  # SAME convolution with the spatially flipped, channel-transposed kernel
            wf = torch.flip(W, (0, 1)).permute(2, 3, 0, 1)
            out["dx"] = F.conv2d(dzr.permute(0, 3, 1, 2), wf, padding=1).permute(0, 2, 3, 1)
    return out


def network_forward(params, images, dtype=torch.float64):
    """-> (features [B,2048], mu | var of every layer in the statistics layout)"""
    lt = [layer_tensors(params, s, dtype) for s in CONV_SPECS]
    stats = torch.zeros(2 * ENCODER_STAT_CHANNELS, dtype=dtype)

    def run(i, x, residual=None, relu=True):
        y, _, mu, var = layer_forward(CONV_SPECS[i], x, lt[i], residual, relu)
        om, ov = ENCODER_STAT_OFFSETS[i]
        stats[om:om + mu.numel()], stats[ov:ov + mu.numel()] = mu, var
        return y

    x = run(0, images.to(dtype))
    x = F.max_pool2d(F.pad(x.permute(0, 3, 1, 2), (1, 1, 1, 1)), 3, 2).permute(0, 2, 3, 1)
    for i2a, i2b, i2c, i1 in blocks():
        t = run(i2b, run(i2a, x))
        x = run(i2c, t, run(i1, x, relu=False) if i1 is not None else x)
    return x.mean((1, 2)), stats


def network_backward(params, images, zstash, stash, pooled, winners, grad_features, dtype=torch.float64):
    """the whole-network backward driven by the stash: zstash[i] the raw output of layer i (its statistics and xhat), stash[i] its activated
    output (its sign is the gate and it is the next layer's input), pooled the max-pooled map, winners = maxpool_winners(stash[0])
    -> the flat gradient [ENCODER_PARAM_FLOATS]"""
    flat = torch.zeros(ENCODER_PARAM_FLOATS, dtype=dtype)

    def back(i, x, dy, gated=True, want_dx=True):
        r = layer_backward(CONV_SPECS[i], x.to(dtype), zstash[i].to(dtype), stash[i], dy, lt[i], want_dx=want_dx, gated=gated)
        o = ENCODER_PARAM_OFFSETS[i][0]
        v = layer_grad_flat(r)
        flat[o:o + v.numel()] = v
        return r

    lt = [layer_tensors(params, s, dtype) for s in CONV_SPECS]
    B = images.shape[0]
    g = avgpool_backward(grad_features.to(dtype), 49).reshape(B, 7, 7, 2048)
    bl = blocks()
    for k in range(len(bl) - 1, -1, -1):
        i2a, i2b, i2c, i1 = bl[k]
        xin = pooled if k == 0 else stash[bl[k - 1][2]]
        rc = back(i2c, stash[i2b], g)
        rb = back(i2b, stash[i2a], rc["dx"])
        ra = back(i2a, xin, rb["dx"])
        g = ra["dx"] + (rc["dz"] if i1 is None else back(i1, xin, rc["dz"], gated=False)["dx"])
    g = maxpool_backward(winners, g, 112)
    back(0, images, g, want_dx=False)
    return flat


def momentum_update(stats, batch, B, momentum, unbiased):
    """stats, batch: flat tensors in the statistics layout -> momentum * stats + (1 - momentum) * batch, each layer's batch variance times
    M / (M - 1) when unbiased, M = B * hout * hout"""
    batch = batch.clone()
    if unbiased:
        for s, (_, ov) in zip(CONV_SPECS, ENCODER_STAT_OFFSETS):
            M = B * s.hout * s.hout
            batch[ov:ov + s.cout] *= M / (M - 1.0)
    return momentum * stats + (1.0 - momentum) * batch
