from .abstract_classes import (  # noqa: F401
    InferenceModule,
    ObjectDetectionInference,
    OodPostprocessor,
    Postprocessor,
    ProbabilisticInferenceModule,
    get_baselines_thresholds,
    get_method_threshold,
    record_time,
)
from .funcs import (  # noqa: F401
    RouteDICE,
    ash_s_conv_layer,
    ash_s_linear_layer,
    generalized_entropy,
    get_dice_feat_mean_react_percentile,
    get_mcd_pred_uncertainty_score,
    get_predictive_uncertainty_score,
    gmm_fit,
    mahalanobis_postprocess,
    mahalanobis_preprocess,
    normalizer,
)
from .image_level import LaRDInference, LaRExInference  # noqa: F401
from .object_level import BoxInferenceYolo, ObjectLevelInference  # noqa: F401
from .pipeline import LaREMPipeline  # noqa: F401
from .pixel_level import (  # noqa: F401
    get_pixel_mcd_uncertainty_maps,
    image_scores_from_maps,
    pixel_ood_metrics,
    pixel_uncertainty_maps,
)
from .pixel_features import (  # noqa: F401
    PixelMahalanobis,
    fit_pixel_mahalanobis,
    get_pixel_mahalanobis_maps,
    pixel_feature_rows,
)
from .pixel_knn import (  # noqa: F401
    PixelKNN,
    fit_pixel_knn,
    get_pixel_knn_maps,
    kcenter_greedy,
)
from .pixel_sml import (  # noqa: F401
    PIXEL_SML_OUTPUTS,
    PixelSML,
    PixelSMLAccumulator,
    fit_pixel_sml,
    get_pixel_sml_maps,
    suppress_and_smooth,
)
from .mask_level import (  # noqa: F401
    MASK_MAP_OUTPUTS,
    get_mask_anomaly_maps,
    mask_anomaly_maps,
)
from .postprocessors import (  # noqa: F401
    ASH,
    DDU,
    DICE,
    GEN,
    KNN,
    MSP,
    DICEReAct,
    ReAct,
    ViM,
    DetectorKDE,
    Energy,
    FlatL2Bank,
    GMMLatentSpace,
    KDELatentSpace,
    KNNLatentSpace,
    Mahalanobis,
    MDLatentSpace,
    cMDLatentSpace,
    postprocessor_input_dict,
    postprocessors_dict,
    register_postprocessor,
)
from .extended_postprocessors import (  # noqa: F401
    FDBD,
    KLMatching,
    MaxLogit,
    RelativeMahalanobis,
    TempScale,
    extended_postprocessor_input_dict,
    extended_postprocessors_dict,
    fdbd_inverse_distances,
)
