"""NumPy restatement of the optimiser update of csrc/adam.hip = TensorFlow's fused ResourceApplyAdam, which tf.keras.optimizers.Adam
runs (the reference: src/trainer.py:183-184):

    alpha = lr * sqrt(1 - beta2^t) / (1 - beta1^t)
    m += (g - m) * (1 - beta1);  v += (g * g - v) * (1 - beta2);  var -= (m * alpha) / (sqrt(v) + eps)

in float64 (the yardstick) and in float32 with the kernel's operation order (the bit reference: NumPy's float32 add, multiply, divide
and sqrt are correctly rounded and keep subnormals, as the kernel's are)."""
import math

import numpy as np


def power(beta, t):
    """beta^t by square-and-multiply in double, in the order of the library's helper"""
    r, b, t = 1.0, float(beta), int(t)
    while t:
        if t & 1:
            r *= b
        b *= b
        t >>= 1
    return r


def alpha64(lr, beta1, beta2, t):
    return lr * math.sqrt(1.0 - power(beta2, t)) / (1.0 - power(beta1, t))


def one_minus(beta):
    """1 - beta as Keras takes it for a float32 variable: both operands float32"""
    return np.float32(1.0) - np.float32(beta)


def step64(p, m, v, g, alpha, omb1, omb2, eps):
    p, m, v, g = (np.asarray(a, np.float64) for a in (p, m, v, g))
    m = m + (g - m) * float(omb1)
    v = v + (g * g - v) * float(omb2)
    p = p - (m * float(alpha)) / (np.sqrt(v) + float(eps))
    return p, m, v


def step32(p, m, v, g, alpha, omb1, omb2, eps):
    """every operand and every intermediate float32, one rounding per operation"""
    f = np.float32
    p, m, v, g = (np.asarray(a, f) for a in (p, m, v, g))
    alpha, omb1, omb2, eps = f(alpha), f(omb1), f(omb2), f(eps)
    m = m + (g - m) * omb1
    v = v + (g * g - v) * omb2
    p = p - (m * alpha) / (np.sqrt(v) + eps)
    assert p.dtype == m.dtype == v.dtype == np.float32
    return p, m, v


def rel_err(a, b):
    """norm-relative error of a against b (float64); 0 where both vanish"""
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    nb = np.linalg.norm(b)
    d = np.linalg.norm(a - b)
    return 0.0 if d == 0.0 else d / nb
