from .entropy import get_dl_h_z, single_image_entropy_calculation  # noqa: F401
from .metrics import get_auroc_results  # noqa: F401
from .metrics import log_evaluate_postprocessors, select_and_log_best_larex  # noqa: F401
from .latent_space import log_evaluate_larex  # noqa: F401
from .baselines import baseline_name_dict, calculate_all_baselines, get_labels_from_logits, remove_latent_features  # noqa: F401
from .open_set import (  # noqa: F401
    COCOParser,
    OpenSetEvaluator,
    convert_xywh_to_xyxy,
    evaluate_open_set_detection_methods,
    evaluate_open_set_detection_one_method,
    get_boxes_from_precalculated,
    get_boxes_gtu_and_uu_ood_dataset,
    get_gtu_uu_per_class,
    get_labels_and_scores_from_logits,
    get_n_unk_ood_dataset,
    get_overall_open_set_results,
    voc_ap,
    voc_eval,
)
from .box_subsets import get_gtu_uu_metrics, subset_boxes  # noqa: F401
from .calibration import (  # noqa: F401
    CalibrationResult,
    ReliabilityBins,
    TemperatureScaler,
    calibration_metrics,
    fit_temperature,
)
from .pixel_calibration import (  # noqa: F401
    PixelCalibrationAccumulator,
    PixelCalibrationResult,
    PixelTemperatureScaler,
    fit_pixel_temperature,
    get_pixel_calibration,
    pixel_calibration_metrics,
)
from .conformal import (  # noqa: F401
    ConformalClassifier,
    ConformalResult,
    PredictionSets,
    conformal_quantile,
    conformal_scores,
)
from .bootstrap import (  # noqa: F401
    BootstrapResult,
    ComparisonResult,
    bootstrap_ood_metrics,
    bootstrap_p_value,
    bootstrap_results_table,
    compare_ood_methods,
)
from .components import ComponentResult, component_metrics, label_components  # noqa: F401
from .selective import (  # noqa: F401
    RiskCoverageCurve,
    SelectiveResult,
    adaptive_calibration_error,
    selective_metrics,
    selective_metrics_from_logits,
    selective_results_table,
)
from .selective_bootstrap import (  # noqa: F401
    SelectiveBootstrapResult,
    SelectiveComparisonResult,
    bootstrap_selective_metrics,
    bootstrap_selective_metrics_from_logits,
    bootstrap_selective_table,
    compare_selective_methods,
)
from .shift import (  # noqa: F401
    ShiftDetector,
    ShiftTestResult,
    energy_test,
    median_bandwidth,
    mmd_test,
    shift_power_table,
)
from .shift_univariate import (  # noqa: F401
    MaxTAdjustment,
    UnivariateShiftDetector,
    UnivariateShiftResult,
    ks_asymptotic_p,
    ks_test,
    maxt_adjust,
)
