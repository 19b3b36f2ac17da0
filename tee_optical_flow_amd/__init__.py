"""tee_optical_flow_amd -- MI355X-native dense optical flow (DualTVL1) behind the reference's
OF_model.calc() / process_video() surface.  See DESIGN.md."""
from .config import OpticalFlowCalculationConfig, default_optical_flow_config
from .exceptions import (ConfigurationError, DICOMReadError, OpticalFlowCalculationError, OpticalFlowError,
                         WaveformLoadError, WaveformValidationError)
from .dense_flow import DenseFlow, HeldFrames, createOptFlow_DeepFlow, createOptFlow_DualTVL1, cuda_OpticalFlowDual_TVL1_create
from .analysis import (FlowStudy, HeldStudy, angle_mode_series, area_series, av_centroids, calculate_3dhist, calculate_3dhist_radlong, colormap_lut, param_radlong_stats,
                       radlong_overlay, visualize_radlong)

__all__ = ["DenseFlow", "HeldFrames", "createOptFlow_DualTVL1", "createOptFlow_DeepFlow", "cuda_OpticalFlowDual_TVL1_create", "OpticalFlowCalculationConfig",
           "default_optical_flow_config", "OpticalFlowError", "DICOMReadError", "WaveformLoadError",
           "WaveformValidationError", "OpticalFlowCalculationError", "ConfigurationError", "FlowStudy", "HeldStudy", "av_centroids",
           "calculate_3dhist_radlong", "param_radlong_stats", "calculate_3dhist", "angle_mode_series", "area_series", "radlong_overlay", "visualize_radlong",
           "colormap_lut"]
