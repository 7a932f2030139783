"""The Dense layers of the reference's CriticNetwork (src/models.py:158-202) in the order of the C ABI (hpe_critic_layer_name /
hpe_critic_layer_shape): the one host-side table; synthetic.py and tf_checkpoint.py derive theirs from it, tests check it against the
library's."""

# (Keras layer name, in, out): kernel [in, out], bias [out]; all nine kernel shapes differ
CRITIC_LAYERS = (("kcs_dense", 169, 100), ("joints_dense", 42, 100), ("combined_dense", 200, 1), ("shapes_dense_1", 10, 10),
                 ("shapes_dense_2", 10, 5), ("shapes_dense_3", 5, 1), ("rotation_dense_1", 207, 300), ("rotation_dense_2", 300, 100),
                 ("rotation_dense_3", 100, 1))


# ---- the flat parameter layout of hpe_critic_weight_grad / hpe_critic_get_params / hpe_critic_set_params_dev:
# kernel 0 [in, out] (row-major), bias 0, kernel 1, ... in CRITIC_LAYERS order (hpe_critic_param_offset)
def flat_layout():
    """-> [(key, offset, shape)] for the 18 tensors, keys as HpeEngine.load_critic takes them"""
    out, off = [], 0
    for name, fi, fo in CRITIC_LAYERS:
        out.append(("critic/%s/kernel" % name, off, (fi, fo)))
        off += fi * fo
        out.append(("critic/%s/bias" % name, off, (fo,)))
        off += fo
    return out


PARAM_FLOATS = sum(fi * fo + fo for _name, fi, fo in CRITIC_LAYERS)  # hpe_critic_param_floats()


def params_to_flat(params, dtype="float32"):
    """Keras-layout dict -> one flat numpy vector [PARAM_FLOATS]"""
    import numpy as np

    flat = np.empty(PARAM_FLOATS, dtype)
    for key, off, shape in flat_layout():
        a = np.asarray(params[key])
        if a.shape != shape:
            raise ValueError("%s must be %s, got %s" % (key, shape, a.shape))
        flat[off : off + a.size] = a.reshape(-1)
    return flat


def flat_to_params(flat):
    """flat vector (numpy array or torch tensor, [PARAM_FLOATS]) -> the Keras-layout dict of numpy arrays that ``load_critic`` and
    ``weights.npz`` take"""
    import numpy as np

    if hasattr(flat, "detach"):
        flat = flat.detach().cpu().numpy()
    flat = np.asarray(flat)
    if flat.shape != (PARAM_FLOATS,):
        raise ValueError("flat must have %d entries, got %s" % (PARAM_FLOATS, flat.shape))
    return {key: flat[off : off + int(np.prod(shape))].reshape(shape).copy() for key, off, shape in flat_layout()}
