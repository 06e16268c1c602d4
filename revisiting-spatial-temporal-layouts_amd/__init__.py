"""MI355X-native STLT forward hot path (drop-in for the reference's ``StltBackbone`` / ``Stlt``).

The directory name carries a hyphen, so import it with
``importlib.import_module("revisiting-spatial-temporal-layouts_amd")``.
"""
from . import _lib, collate, dist, frame_data, infer, layout_data, ops, synth, train, video  # noqa: F401
from ._lib import StltHipError  # noqa: F401
from .frame_data import DeviceAppearanceDataset, DeviceFrameStore, DeviceMultimodalDataset, appearance_indices  # noqa: F401
from .modelling.configs import AppearanceModelConfig, MultimodalModelConfig, StltModelConfig, model_configs_factory  # noqa: F401
from .modelling.fusion import CrossAttentionCentralNetFusion, CrossAttentionFusion, LateConcatenationFusion, TransformerResnet  # noqa: F401
from .modelling.resnet3d import Resnet3D  # noqa: F401
from .modelling.models import (  # noqa: F401
    CategoryBoxEmbeddings,
    ClassificationHead,
    FramesEmbeddings,
    SpatialTransformer,
    Stlt,
    StltBackbone,
    models_factory,
)
from .utils.evaluation import evaluators_factory  # noqa: F401
from .utils.model_utils import generate_square_subsequent_mask  # noqa: F401

__all__ = ["Stlt", "StltBackbone", "StltModelConfig", "models_factory", "model_configs_factory", "StltHipError",
           "ops", "synth", "dist", "infer", "train", "video", "layout_data", "frame_data",
           "DeviceFrameStore", "DeviceAppearanceDataset", "DeviceMultimodalDataset", "appearance_indices"]
