"""Restatement of the mixed-precision encoder walks (DESIGN.md "Mixed-precision encoder training"), in torch on the CPU: float32
arithmetic with a rounding to bf16 (RNE: round to nearest, ties to even) at exactly the rounding points of the contract, and nowhere else.
tests/encoder_train_ref.py is the float32 / float64 restatement these functions follow operation for operation: with the roundings
switched off (``rounding=False``) they give its float32 results bit for bit.

  1. W16 = RNE(W) per element of the master kernels; image pixels are RNE-rounded.
  2. y = RNE(act(s * acc + shift (+ res))), acc the fp32 accumulation of exact bf16 products, the residual added before the one rounding.
  3. the max pool is exact; features = (fp32 sum of 49 bf16 values) / 49.
  4. g = RNE(grad_features / 49).
  5. dz = dy * [y > 0] exact; dzs = RNE(dz * s): one fp32 multiply, one rounding.
  6. dx = RNE(acc (+ running block cotangent)), the sum in fp32 before the rounding.
  7. the stride-2 scatter is exact; the max-pool backward sums its at most four cotangents in fp32 and rounds once.
  8. G = A^T dz, dW = s * G, dshift, db, dbeta and dgamma = (<W16, G> + (b - mean) * dshift) / sqrt(var + eps) stay fp32."""
import numpy as np
import torch
import torch.nn.functional as F

import encoder_train_ref as R
from hpe_amd.resnet_spec import CONV_SPECS, ENCODER_PARAM_FLOATS, ENCODER_PARAM_OFFSETS


def rne(t):
    """float32 tensor -> the nearest bf16 value (ties to even), held in float32.  Integer arithmetic on the bits, not a cast: add half an
    ulp of the 8-bit significand minus one, plus the lowest kept bit, and cut the low 16 bits.  The largest finite float32 rounds to
    infinity, infinities stay, NaNs stay NaN (quietened, as the hardware conversion does)."""
    assert t.dtype == torch.float32, t.dtype
    bits = t.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    rounded = (bits + 0x7FFF + ((bits >> 16) & 1)) & 0xFFFF0000
    nan = (bits & 0x7FFFFFFF) > 0x7F800000
    rounded = torch.where(nan, (bits | 0x00400000) & 0xFFFF0000, rounded)
    rounded = torch.where(rounded >= 0x80000000, rounded - 0x100000000, rounded)  # back into the int32 range, same bits
    return rounded.to(torch.int32).view(torch.float32).reshape(t.shape)


def _q(rounding):
    return rne if rounding else (lambda t: t)


def folded_scale(lt, eps=R.EPS):
    """the fp32 BatchNorm scale the library's layers hold: gamma / sqrt(var + eps) in double (eps the float 1e-3), rounded once"""
    _, _, gamma, _, _, var = lt
    sd = np.sqrt(var.double().numpy() + np.float64(np.float32(eps)))
    return torch.from_numpy((gamma.double().numpy() / sd).astype(np.float32))


def weights16(lt, rounding=True):
    """the layer tensors with the kernel rounded (rounding point 1)"""
    return [_q(rounding)(lt[0])] + list(lt[1:])


def layer_forward_mixed(s, x, lt, residual=None, relu=True, rounding=True):
    """x, residual: bf16 values in float32; lt: float32 layer tensors (master weights) -> y = RNE(act(s * conv(x, W16) + shift (+ res)))"""
    assert x.dtype == torch.float32
    return _q(rounding)(R.layer_forward(s, x, weights16(lt, rounding), residual, relu))


def data_grad_mixed(s, dzs, W16, B, res=None, rounding=True):
    """dx = RNE(dzs . W16^T (+ res)): encoder_train_ref.layer_backward's data gradient, the residual (full resolution) added in fp32
    before the one rounding; a stride-2 layer's low-resolution product is spread first, which is exact"""
    q = _q(rounding)
    Wm = W16.reshape(-1, s.cout)
    if s.kh == 1:
        lo = (dzs.reshape(-1, s.cout) @ Wm.t()).reshape(B, s.hout, s.hout, s.cin)
        if s.stride == 1:
            dx = lo
        else:
            dx = torch.zeros(B, s.hin, s.hin, s.cin, dtype=dzs.dtype)
            dx[:, ::2, ::2, :] = lo
    else:
        wf = torch.flip(W16, (0, 1)).permute(2, 3, 0, 1)
        dx = F.conv2d(dzs.permute(0, 3, 1, 2), wf, padding=1).permute(0, 2, 3, 1)
    return q(dx if res is None else dx + res)


def layer_backward_mixed(s, x, y, dy, lt, want_dx=True, gated=True, rounding=True, res=None, scale=None):
    """x, y, dy: bf16 values in float32 (idx 0: x the float32 images, rounded here); lt: float32 layer tensors.  res: the running block
    cotangent added to the data gradient before its rounding.  scale: the fp32 scale of rounding point 5 (default: gamma / sqrt(var + eps)
    in float32, as encoder_train_ref; the library's is folded_scale).  -> dict dx, dW, db, dgamma, dbeta, dz, dzs"""
    assert x.dtype == torch.float32 and dy.dtype == torch.float32
    q = _q(rounding)
    lt16 = weights16(lt, rounding)
    if s.kh == 7:
        x = q(x)
    out = R.layer_backward(s, x, y, dy, lt16, want_dx=False, gated=gated)  # rounding point 8: all of it fp32, <W16, G> for dgamma
    if want_dx and s.kh != 7:
        _, _, gamma, _, _, var = lt
        sc = gamma * (1.0 / torch.sqrt(var + R.EPS)) if scale is None else scale
        out["dzs"] = q(out["dz"] * sc)
        out["dx"] = data_grad_mixed(s, out["dzs"], lt16[0], x.shape[0], res, rounding)
    return out


def network_backward_mixed(params, images, stash, pooled, winners, grad_features, rounding=True):
    """encoder_train_ref.network_backward in float32 with the roundings of the mixed walk: stash / pooled hold bf16 values (any dtype),
    images and grad_features are float32 -> the flat float32 gradient"""
    dtype = torch.float32
    q = _q(rounding)
    flat = torch.zeros(ENCODER_PARAM_FLOATS, dtype=dtype)

    def put(i, r):
        o = ENCODER_PARAM_OFFSETS[i][0]
        v = R.layer_grad_flat(r)
        flat[o:o + v.numel()] = v

    lt = [R.layer_tensors(params, s, dtype) for s in CONV_SPECS]
    B = images.shape[0]
    g = q(R.avgpool_backward(grad_features.to(dtype), 49)).reshape(B, 7, 7, 2048)
    bl = R.blocks()
    for k in range(len(bl) - 1, -1, -1):
        i2a, i2b, i2c, i1 = bl[k]
        xin = (pooled if k == 0 else stash[bl[k - 1][2]]).to(dtype)
        rc = layer_backward_mixed(CONV_SPECS[i2c], stash[i2b].to(dtype), stash[i2c], g, lt[i2c], rounding=rounding)
        put(i2c, rc)
        rb = layer_backward_mixed(CONV_SPECS[i2b], stash[i2a].to(dtype), stash[i2b], rc["dx"], lt[i2b], rounding=rounding)
        put(i2b, rb)
        if i1 is None:  # the identity shortcut's cotangent is the block's dz: added before the data gradient's rounding
            ra = layer_backward_mixed(CONV_SPECS[i2a], xin, stash[i2a], rb["dx"], lt[i2a], rounding=rounding, res=rc["dz"])
            put(i2a, ra)
            g = ra["dx"]
        else:
            ra = layer_backward_mixed(CONV_SPECS[i2a], xin, stash[i2a], rb["dx"], lt[i2a], rounding=rounding)
            put(i2a, ra)
            r1 = layer_backward_mixed(CONV_SPECS[i1], xin, None, rc["dz"], lt[i1], gated=False, rounding=rounding, res=ra["dx"])
            put(i1, r1)
            g = r1["dx"]
    g = q(R.maxpool_backward(winners, g, 112))
    put(0, layer_backward_mixed(CONV_SPECS[0], images.to(dtype), stash[0], g, lt[0], want_dx=False, rounding=rounding))
    return flat
