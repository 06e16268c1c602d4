"""Model configuration for the STLT path — same attribute surface as the reference's
``GeneralModelConfig`` / ``StltModelConfig`` (src/modelling/configs.py:92-111) so train.py / inference.py
constructor calls work unchanged."""


class StltModelConfig:
    _DEFAULTS = (
        ("hidden_size", 768),
        ("hidden_dropout_prob", 0.1),
        ("layer_norm_eps", 1e-12),
        ("num_attention_heads", 12),
        ("num_spatial_layers", 4),
        ("num_temporal_layers", 8),
        ("layout_num_frames", 256),
        ("load_backbone_path", None),
        ("freeze_backbone", False),
    )

    def __init__(self, **kwargs):
        self.num_classes = kwargs.pop("num_classes", None)
        assert self.num_classes, "num_classes must not be None!"
        self.unique_categories = kwargs.pop("unique_categories", None)
        assert self.unique_categories, "unique_categories must not be None!"
        for name, default in self._DEFAULTS:
            setattr(self, name, kwargs.pop(name, default))

    def __repr__(self):
        rows = [("Unique categories", self.unique_categories), ("Number of classes", self.num_classes),
                ("Hidden size", self.hidden_size), ("Hidden dropout probability", self.hidden_dropout_prob),
                ("Layer normalization epsilon", self.layer_norm_eps),
                ("Number of attention heads", self.num_attention_heads),
                ("Number of spatial layers", self.num_spatial_layers),
                ("Number of temporal layers", self.num_temporal_layers),
                ("Max number of layout frames", self.layout_num_frames),
                ("The backbone path is", self.load_backbone_path), ("Freezing the backbone", self.freeze_backbone)]
        return "\n".join(f"- {k}: {v}" for k, v in rows)


class MultimodalModelConfig:
    """Attribute surface of the reference's ``MultimodalModelConfig`` (src/modelling/configs.py:128-175) for CAF / CACNF
    on precomputed appearance features: ``stlt_config`` for the layout branch plus the appearance / fusion sizes.
    ``resnet_model_path`` is read only with ``appearance_trunk=True`` (then the R3D-50 trunk is part of the model and runs on
    ``video_frames``); by default the appearance branch starts from precomputed features and the path is ignored."""

    def __init__(self, **kwargs):
        self.stlt_config = StltModelConfig(**dict(kwargs))
        self.num_classes = self.stlt_config.num_classes
        self.hidden_size = self.stlt_config.hidden_size
        self.hidden_dropout_prob = self.stlt_config.hidden_dropout_prob
        self.layer_norm_eps = self.stlt_config.layer_norm_eps
        self.num_attention_heads = self.stlt_config.num_attention_heads
        self.appearance_num_frames = kwargs.pop("appearance_num_frames", None)
        assert self.appearance_num_frames, "appearance_num_frames must not be None!"
        self.resnet_model_path = kwargs.pop("resnet_model_path", None)
        self.num_appearance_layers = kwargs.pop("num_appearance_layers", 4)
        self.num_fusion_layers = kwargs.pop("num_fusion_layers", 4)
        self.load_backbone_path = kwargs.pop("load_backbone_path", None)
        self.freeze_backbone = kwargs.pop("freeze_backbone", False)
        # opt-in: the appearance branch carries the R3D-50 trunk (the reference's `appearance_branch.resnet.*` keys) and runs it on
        # `video_frames` when a batch has no `appearance_features`.  Off: the branch starts from precomputed features, as before.
        self.appearance_trunk = bool(kwargs.pop("appearance_trunk", False))
        # opt-in: a grad-enabled forward trains the trunk's 53 Conv3d weights (native Conv3d backward, modelling/resnet3d.py).
        # Off: a trainable trunk under autograd is an error, as before.
        self.train_trunk = bool(kwargs.pop("train_trunk", False))
        self.appearance_config = self
        self.stlt_config.load_backbone_path = None  # the fusion models build a fresh layout branch (models.py:439)


class AppearanceModelConfig:
    """Attribute surface of the reference's ``AppearanceModelConfig`` (src/modelling/configs.py:129-145).  ``resnet_model_path`` is
    optional here: without it the trunk keeps its fresh initialisation (load a state dict afterwards)."""

    def __init__(self, **kwargs):
        self.num_classes = kwargs.pop("num_classes", None)
        assert self.num_classes, "num_classes must not be None!"
        self.hidden_size = kwargs.pop("hidden_size", 768)
        self.hidden_dropout_prob = kwargs.pop("hidden_dropout_prob", 0.1)
        self.layer_norm_eps = kwargs.pop("layer_norm_eps", 1e-12)
        self.num_attention_heads = kwargs.pop("num_attention_heads", 12)
        self.appearance_num_frames = kwargs.pop("appearance_num_frames", None)
        assert self.appearance_num_frames, "appearance_num_frames must not be None!"
        self.resnet_model_path = kwargs.pop("resnet_model_path", None)
        self.num_appearance_layers = kwargs.pop("num_appearance_layers", 4)
        # opt-in: a grad-enabled forward trains the trunk's 53 Conv3d weights (native Conv3d backward, modelling/resnet3d.py).
        # Off: a trainable trunk under autograd is an error, as before.
        self.train_trunk = bool(kwargs.pop("train_trunk", False))

    def __repr__(self):
        rows = [("Number of classes", self.num_classes), ("Max number of appearance frames", self.appearance_num_frames),
                ("Hidden size", self.hidden_size), ("If Transformer: Number of attention heads", self.num_attention_heads),
                ("If Transformer: Number of layers", self.num_appearance_layers),
                ("If Transformer: Hidden dropout probability", self.hidden_dropout_prob)]
        return "\n".join(f"- {k}: {v}" for k, v in rows)


model_configs_factory = {
    "stlt": StltModelConfig,
    "resnet3d": AppearanceModelConfig,
    "resnet3d-transformer": AppearanceModelConfig,
    "lcf": MultimodalModelConfig,
    "caf": MultimodalModelConfig,
    "cacnf": MultimodalModelConfig,
}
