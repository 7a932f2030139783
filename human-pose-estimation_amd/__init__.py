"""MI355X-native per-image forward hot path of maxpit/human-pose-estimation.

Host side mirrors the reference's interface for this path: ``Predictor`` (src/predictor.py), ``SMPL``
(src/tf_smpl/batch_smpl.py), ``batch_orth_proj_idrot`` / ``reproject_vertices`` (src/tf_smpl/projection.py),
``kp_reprojection_loss`` / ``mesh_reprojection_loss`` (src/ops.py), ``critic_scores`` /
``generator_critic_loss`` (CriticNetwork + get_kcs, src/models.py:97-202), ``critic_wgan_loss`` / ``CriticTrainer`` (the critic
update, src/trainer.py:508-583), ``regressor_thetas`` / ``GeneratorTrainer`` (the generator update after the encoder,
src/trainer.py:383-505).  All arithmetic runs in the C-ABI
library ``lib/libhpe_hip.so`` (include/hpe.h); there is no CPU fallback.
"""
import os as _os

# Batch-chunk streams + RCCL's own streams must not share hardware queues (DESIGN.md "Multi-GPU"); only effective when the
# package is imported before the first HIP call of the process, which is the normal order.
try:
    if int(_os.environ.get("GPU_MAX_HW_QUEUES", "0")) < 8:
        _os.environ["GPU_MAX_HW_QUEUES"] = "8"
except ValueError:
    _os.environ["GPU_MAX_HW_QUEUES"] = "8"

from . import critic_spec, regressor_spec, resnet_spec, synthetic  # noqa: F401,E402
from ._lib import HpeError  # noqa: F401
from .augment import augment_batch, draw_augmentation, gt3d_real, mocap_real, plan_augmentation, reflect_joints3d, reflect_pose  # noqa: F401
from .critic_train import CriticTrainer  # noqa: F401
from . import distributed  # noqa: F401
from .distributed import Reducer, ShardedPredictor  # noqa: F401
from .draw import draw_panels, draw_results, draw_skeleton  # noqa: F401
from .engine import HpeEngine  # noqa: F401
from .generator_train import GeneratorTrainer  # noqa: F401
from .fit import fit_keypoints, fit_reprojection  # noqa: F401
from .jpeg import DecodedBatch, decode_jpeg_batch, jpeg_info  # noqa: F401
from .png import decode_image_batch, decode_png_batch, png_info  # noqa: F401
from .png_encode import encode_png_batch  # noqa: F401
from .jpeg_encode import encode_jpeg_batch, forward_dct_batch, quant_tables  # noqa: F401
from . import mat5_lite  # noqa: F401
from .datasets import create_datasets, create_records, filename_pairs_lsp, filename_pairs_lspe, filename_pairs_mpii, image_record  # noqa: F401
from .records import (RecordDataset, RecordError, TFRecordWriter, image_example, load_training_batch, load_training_batch_3d, mocap_example, parse_example,  # noqa: F401
                      parse_image_example, parse_mocap_example, read_tfrecords, serialize_example, write_tfrecords)
from .metrics import Scores, Scores3D, eval_scores, pose3d_scores, procrustes_align  # noqa: F401
from .image import get_original, preprocess_batch, preprocess_image  # noqa: F401
from .ops import Gt3D, joints3d_loss, loss3d_counts, smpl_param_loss  # noqa: F401
from .ops import critic_gradient_penalty, critic_scores, critic_wgan_loss, generator_critic_loss, kp_reprojection_loss, mesh_reprojection_loss, regressor_thetas, encoder_features  # noqa: F401
from .optim import KerasAdam  # noqa: F401
from .predictor import Predictor  # noqa: F401
from .projection import batch_orth_proj_idrot, reproject_vertices  # noqa: F401
from .render import SMPLRenderer  # noqa: F401
from .smpl import SMPL  # noqa: F401
from .summary import SummaryWriter, read_events  # noqa: F401
from .trainer import Trainer  # noqa: F401


def __getattr__(name):
    # the autograd glue imports torch at module level, the package does not: Loss3DFunction is resolved on first use
    if name == "Loss3DFunction":
        from .autograd import Loss3DFunction

        return Loss3DFunction
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
