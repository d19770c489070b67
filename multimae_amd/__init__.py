"""multimae_amd -- MI355X (gfx950)-native engine for the MultiMAE pre-training hot path.

Public surface = the reference's ``multimae`` package surface for that path
(multimae/__init__.py): criterion, input adapters, MultiMAE / MultiViT + factories,
SpatialOutputAdapter; plus the engine controls (precision, parameter arena, fused optimiser,
data-parallel gradient reducer) and the batch stager (host batches copied on their own stream, decoded on the device).
"""
from . import engine  # noqa: F401
from .data_ops import mask_invalid_, robust_depth_standardize, robust_depth_standardize_, truncated_depth_standardize  # noqa: F401
from .criterion import (LabelSmoothingCrossEntropy, MaskedCrossEntropyLoss, MaskedL1Loss, MaskedMSELoss,  # noqa: F401
                        SegCrossEntropyLoss, SoftTargetCrossEntropy, masked_berhu_loss, masked_l1_loss, masked_mse_loss)
from .ema import ModelEma  # noqa: F401
from .mixup import Mixup  # noqa: F401
from .random_erasing import RandomErasing  # noqa: F401
from .rand_augment import RandAugment  # noqa: F401
from .metrics import ClsMetric, DepthMetric, SegMetric, cls_accuracy, depth_metrics, seg_argmax  # noqa: F401
from .input_adapters import PatchedInputAdapter, SemSegInputAdapter  # noqa: F401
from .multimae import (MultiMAE, MultiViT, multivit_base, multivit_large,  # noqa: F401
                       pretrain_multimae_base, pretrain_multimae_large)
from .output_adapters import LinearOutputAdapter, SpatialOutputAdapter  # noqa: F401
from .registry import create_model, register_model  # noqa: F401
from .staging import BatchStager, ClsStagedLoader, ClsStager, StagedLoader  # noqa: F401
from .task_balancing import NoWeightingStrategy, UncertaintyWeightingStrategy  # noqa: F401

__version__ = '0.1.0'
