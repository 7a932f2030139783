"""The Dense layers of the reference's CriticNetwork (src/models.py:158-202) in the order of the C ABI (hpe_critic_layer_name /
hpe_critic_layer_shape): the one host-side table; synthetic.py and tf_checkpoint.py derive theirs from it, tests check it against the
library's."""

# (Keras layer name, in, out): kernel [in, out], bias [out]; all nine kernel shapes differ
CRITIC_LAYERS = (("kcs_dense", 169, 100), ("joints_dense", 42, 100), ("combined_dense", 200, 1), ("shapes_dense_1", 10, 10),
                 ("shapes_dense_2", 10, 5), ("shapes_dense_3", 5, 1), ("rotation_dense_1", 207, 300), ("rotation_dense_2", 300, 100),
                 ("rotation_dense_3", 100, 1))
