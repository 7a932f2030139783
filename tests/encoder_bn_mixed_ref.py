"""Restatement of the mixed-precision encoder walk with batch statistics (DESIGN.md "Mixed-precision encoder training with batch
statistics"), in torch on the CPU: tests/encoder_bn_train_ref.py operation for operation in float32, with a rounding to bf16 (RNE,
tests/encoder_mixed_ref.rne) at exactly the rounding points of the contract and nowhere else.  With the roundings switched off
(``rounding=False``) these functions give encoder_bn_train_ref's float32 results bit for bit.

Points 1, 3, 4 and 7 of encoder_mixed_ref (W16, the pad, the pools, g, the scatter) hold unchanged.  Per layer, M = B * hout * hout:

  1. z16 = RNE(acc + b), acc the fp32 accumulation of exact bf16 products.
  2. mu, var (biased), r: the statistics OF z16.
  3. y16 = RNE(act(gamma * ((z16 - mu) * r) + beta (+ res16))), the residual added in fp32 before the one rounding.
  4. dz = dy16 * [y16 > 0] exact; xhat = (z16 - mu) * r; dbeta = sum dz, dgamma = sum dz * xhat, fp32 results, never rounded to bf16; db = 0.
  5. dzraw16 = RNE(gamma * r * (dz - dbeta / M - xhat * dgamma / M)).
  6. dW = A^T dzraw16 stays fp32; dx = RNE(acc (+ block cotangent))."""
import torch
import torch.nn.functional as F

import encoder_bn_train_ref as RB
import encoder_mixed_ref as X
import encoder_train_ref as R
from hpe_amd.resnet_spec import CONV_SPECS, ENCODER_PARAM_FLOATS, ENCODER_PARAM_OFFSETS, ENCODER_STAT_CHANNELS, ENCODER_STAT_OFFSETS

rne = X.rne


def layer_raw_mixed(s, x, lt, rounding=True):
    """x: bf16 values in float32 (conv1: the float32 images, rounded here) -> z16 = RNE(conv(x, W16) + b)"""
    assert x.dtype == torch.float32
    q = X._q(rounding)
    if s.kh == 7:
        x = q(x)
    return q(RB.layer_raw(s, x, X.weights16(lt, rounding)))


def layer_forward_mixed(s, x, lt, residual=None, relu=True, rounding=True):
    """-> (y16, z16, mu, var): rounding points 1 to 3"""
    z = layer_raw_mixed(s, x, lt, rounding)
    mu, var = RB.batch_stats(z)
    return X._q(rounding)(RB.layer_apply(z, mu, var, lt[2], lt[3], residual, relu)), z, mu, var


def layer_backward_mixed(s, x, z, y, dy, lt, want_dx=True, gated=True, rounding=True, res=None):
    """x, z, y, dy: bf16 values in float32 (idx 0: x the float32 images, rounded here); lt: float32 layer tensors.  res: the running block
    cotangent added to the data gradient before its rounding -> dict dx, dW, db, dgamma, dbeta, dz, dzraw: rounding points 4 to 6"""
    assert x.dtype == torch.float32 and dy.dtype == torch.float32 and z.dtype == torch.float32
    q = X._q(rounding)
    W, gamma = X.weights16(lt, rounding)[0], lt[2]
    if s.kh == 7:
        x = q(x)
    mu, var = RB.batch_stats(z)
    r = 1.0 / torch.sqrt(var + R.EPS)
    xhat = ((z - mu) * r).reshape(-1, s.cout)
    dz = dy * (y > 0).to(dy.dtype) if gated else dy
    dzm = dz.reshape(-1, s.cout)
    M = dzm.shape[0]
    dbeta = dzm.sum(0)
    dgamma = (dzm * xhat).sum(0)
    dzraw = q(gamma * r * (dzm - dbeta / M - xhat * dgamma / M))
    out = {"dW": (R.im2col(s, x).t() @ dzraw).reshape(W.shape), "db": torch.zeros_like(dbeta), "dbeta": dbeta, "dgamma": dgamma, "dz": dz,
           "dzraw": dzraw}
    if want_dx and s.kh != 7:
        B = x.shape[0]
        out["dx"] = X.data_grad_mixed(s, dzraw.reshape(B, s.hout, s.hout, s.cout), W, B, res, rounding)
    return out


def network_forward_mixed(params, images, rounding=True):
    """float32 images -> (features [B,2048], mu | var of every layer in the statistics layout); the pools are exact, the features the
    fp32 mean of the 49 values of the last layer"""
    dtype = torch.float32
    lt = [R.layer_tensors(params, s, dtype) for s in CONV_SPECS]
    stats = torch.zeros(2 * ENCODER_STAT_CHANNELS, dtype=dtype)

    def run(i, x, residual=None, relu=True):
        y, _, mu, var = layer_forward_mixed(CONV_SPECS[i], x, lt[i], residual, relu, rounding)
        om, ov = ENCODER_STAT_OFFSETS[i]
        stats[om:om + mu.numel()], stats[ov:ov + mu.numel()] = mu, var
        return y

    x = run(0, images.to(dtype))
    x = F.max_pool2d(F.pad(x.permute(0, 3, 1, 2), (1, 1, 1, 1)), 3, 2).permute(0, 2, 3, 1)
    for i2a, i2b, i2c, i1 in R.blocks():
        t = run(i2b, run(i2a, x))
        x = run(i2c, t, run(i1, x, relu=False) if i1 is not None else x)
    return x.mean((1, 2)), stats


def network_backward_mixed(params, images, zstash, stash, pooled, winners, grad_features, rounding=True):
    """encoder_bn_train_ref.network_backward in float32 with the roundings of the walk: zstash / stash / pooled hold bf16 values (any
    dtype), images and grad_features are float32 -> the flat float32 gradient"""
    dtype = torch.float32
    q = X._q(rounding)
    flat = torch.zeros(ENCODER_PARAM_FLOATS, dtype=dtype)
    lt = [R.layer_tensors(params, s, dtype) for s in CONV_SPECS]

    def back(i, x, dy, gated=True, want_dx=True, res=None):
        r = layer_backward_mixed(CONV_SPECS[i], x.to(dtype), zstash[i].to(dtype), stash[i], dy, lt[i], want_dx=want_dx, gated=gated,
                                 rounding=rounding, res=res)
        o = ENCODER_PARAM_OFFSETS[i][0]
        v = R.layer_grad_flat(r)
        flat[o:o + v.numel()] = v
        return r

    B = images.shape[0]
    g = q(R.avgpool_backward(grad_features.to(dtype), 49)).reshape(B, 7, 7, 2048)
    bl = R.blocks()
    for k in range(len(bl) - 1, -1, -1):
        i2a, i2b, i2c, i1 = bl[k]
        xin = pooled if k == 0 else stash[bl[k - 1][2]]
        rc = back(i2c, stash[i2b], g)
        rb = back(i2b, stash[i2a], rc["dx"])
        if i1 is None:  # the identity shortcut's cotangent is the block's dz: added before the data gradient's rounding
            g = back(i2a, xin, rb["dx"], res=rc["dz"])["dx"]
        else:
            ra = back(i2a, xin, rb["dx"])
            g = back(i1, xin, rc["dz"], gated=False, res=ra["dx"])["dx"]
    g = q(R.maxpool_backward(winners, g, 112))
    back(0, images.to(dtype), g, want_dx=False)
    return flat
