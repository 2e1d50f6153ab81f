"""neurovit_amd - MI355X (gfx950) native ViT3D / NeuroEncoder hot path of gillet-thomas/NeuroViT.

Drop-in nn.Modules (same constructors, forward signatures, state_dict keys and config.yaml keys as the
reference's src/models/vit_3d.py and src/models/NeuroEncoder.py) over hand-written HIP kernels reached
through a C-ABI shared library (include/neurovit_hip.h).  There is no CPU / eager fallback.
"""
__version__ = "0.1.0"


def __getattr__(name):
    # `from neurovit_amd import VolumeAugment` (or VolumeAffine, VolumeMix, ModelEma), resolved on first use: importing the package itself stays free of torch
    if name == "VolumeAugment":
        from .augment import VolumeAugment
        return VolumeAugment
    if name == "VolumeAffine":
        from .augment import VolumeAffine
        return VolumeAffine
    if name == "VolumeMix":
        from .augment import VolumeMix
        return VolumeMix
    if name == "ModelEma":
        from .optim import ModelEma
        return ModelEma
    if name in ("param_groups", "LRSchedule", "set_group_lrs"):      # the optimizer half of the fine-tuning recipe
        from . import optim
        return getattr(optim, name)
    if name in ("MaskedPretrainStep", "ReconstructionHead"):         # masked-volume pretraining of the 3D encoder
        from . import pretrain
        return getattr(pretrain, name)
    if name in ("FeatureBank", "GroupIndex", "knn_predict", "knn_evaluate", "LinearProbe", "linear_evaluate"):      # frozen-feature evaluation: the kNN and the linear probe of a (pre)trained encoder
        from . import features
        return getattr(features, name)
    if name == "permutation_test":      # group-level permutation tests with max-statistic FWE maps over attribution maps
        from .stats import permutation_test
        return permutation_test
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
