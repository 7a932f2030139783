"""The trainable tensors of the reference's RegressionNetwork (src/models.py:60-74) and ``mean_var`` (src/trainer.py:481-482) in the order
of the C ABI (hpe_regressor_param_offset): the host-side twin of the flat layout that hpe_regressor_backward /
hpe_regressor_get_params / hpe_regressor_set_params_dev use.  Tests check it against the library's."""

# (key as HpeEngine.load_regressor takes it, shape): kernel [in, out] (row-major), bias [out], in layer order; then mean theta
REGRESSOR_TENSORS = (("dense_0/kernel", (2133, 1024)), ("dense_0/bias", (1024,)), ("dense_1/kernel", (1024, 1024)), ("dense_1/bias", (1024,)),
                     ("dense_2/kernel", (1024, 85)), ("dense_2/bias", (85,)), ("mean_theta", (85,)))
NUM_STAGE = 3  # the reference's num_stage (src/config.py)


def _size(shape):
    n = 1
    for d in shape:
        n *= d
    return n


def flat_layout():
    """-> [(key, offset, shape)] for the seven tensors"""
    out, off = [], 0
    for key, shape in REGRESSOR_TENSORS:
        out.append((key, off, shape))
        off += _size(shape)
    return out


PARAM_FLOATS = sum(_size(shape) for _key, shape in REGRESSOR_TENSORS)  # hpe_regressor_param_floats() = 3,322,026


def params_to_flat(params, mean_theta, dtype="float32"):
    """Keras-layout dict of the three Dense layers + mean theta [85] -> one flat numpy vector [PARAM_FLOATS]"""
    import numpy as np

    src = dict(params)
    src["mean_theta"] = np.asarray(mean_theta).reshape(-1)
    flat = np.empty(PARAM_FLOATS, dtype)
    for key, off, shape in flat_layout():
        a = np.asarray(src[key])
        if a.shape != shape:
            raise ValueError("%s must be %s, got %s" % (key, shape, a.shape))
        flat[off : off + a.size] = a.reshape(-1)
    return flat


def flat_to_params(flat):
    """flat vector (numpy array or torch tensor, [PARAM_FLOATS]) -> dict of numpy arrays: the six ``dense_i/...`` tensors that
    ``load_regressor`` takes and ``mean_theta`` [85] for ``load_mean_theta``"""
    import numpy as np

    if hasattr(flat, "detach"):
        flat = flat.detach().cpu().numpy()
    flat = np.asarray(flat)
    if flat.shape != (PARAM_FLOATS,):
        raise ValueError("flat must have %d entries, got %s" % (PARAM_FLOATS, flat.shape))
    return {key: flat[off : off + _size(shape)].reshape(shape).copy() for key, off, shape in flat_layout()}
