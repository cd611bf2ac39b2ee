from .abstract_classes import MCSamplerModule  # noqa: F401
from .utils import Hook, apply_dropout, get_mean_or_fullmean_ls_sample, get_std_ls_sample, get_variance_ls_sample  # noqa: F401
from .image_level import FastMCDSamplesExtractor  # noqa: F401
from .mcd import MCDSamplesExtractor, deeplabv3p_get_ls_mcd_samples, get_latent_representation_mcd_samples  # noqa: F401
from .object_level import _dropblock_rois_get_entropy, _reduce_features_to_rois, roi_align  # noqa: F401
from .detectors import (  # noqa: F401
    SUPPORTED_OBJECT_DETECTION_ARCHITECTURES,
    BoxFeaturesExtractor,
    Extractor,
    ImageLvlFeatureExtractor,
    ObjectDetectionExtractor,
)
from .aggregation import associate_precalculated_baselines_with_raw_predictions, get_aggregated_data_dict  # noqa: F401
