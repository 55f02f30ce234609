"""Mirror of the reference's ``data`` package for the hot path: graph construction, tiling, synthetic training
noise, ground truth from a clean / noisy survey pair, feature labels from charted objects and from the slope, low-confidence regions for review, gridding a point cloud of soundings (streaming sums, the robust gridder: per-cell median, MAD and flags, and both at variable resolution: straight into the refinement records of a VR layout; depth hypotheses per cell from the robust gridders' sorted lists) and the ``BathymetricGrid`` container (file-format I/O -- GDAL / h5py -- is outside the path; VR BAGs enter as their two HDF5 arrays)."""
from .graph_construction import GraphBuilder, GraphData, Data
from .grid import BathymetricGrid
from .tiling import Tile, TileSpec, TileManager, TileMerger
from .vr_bag import RefinementGrid, VRBagHandler, VRBagWriter, SRBagHandler, SRBagWriter, SidecarBuilder, detect_bag_type
from .synthetic_noise import NoiseAugmentor, NoiseBatch, NoiseLabel, SyntheticNoiseGenerator, training_targets
from .ground_truth import Alignment, GroundTruth, align_survey_pair, compute_ground_truth, ground_truth_stats
from .noise_analysis import analyze_noise_patterns, print_analysis
from .feature_labels import (FEATURE_CLASSES, FeatureLabels, S57Feature, create_feature_labels, feature_pixel_table, feature_plan,
                             rasterize_features)
from .review_regions import ReviewRegions, export_review_regions
from .slope_features import add_feature_labels, create_feature_mask_from_slope, slope_cut, wreck_pixel_table
from .vr_ground_truth import NativeGroundTruth, VRPairTable, compute_ground_truth_native, vr_pair_table
from .sounding_grid import SoundingGrid, SoundingGridder, grid_soundings, plan_sounding_grid, sounding_extent
from .sounding_robust import RobustSoundingGrid, RobustSoundingGridder, grid_soundings_robust
from .sounding_vr import (RobustVRSoundingGrid, RobustVRSoundingGridder, VRLayout, VRLayoutPlanner, VRSoundingGrid, VRSoundingGridder,
                          plan_vr_base_grid, plan_vr_layout)
from .sounding_hypotheses import HypothesisGrid, VRHypothesisGrid
from .locale_guide import guide_from_coarser, locale_guide, locale_guide_planes

__all__ = ["GraphBuilder", "GraphData", "Data", "BathymetricGrid", "Tile", "TileSpec", "TileManager", "TileMerger",
           "RefinementGrid", "VRBagHandler", "VRBagWriter", "SRBagHandler", "SRBagWriter", "SidecarBuilder", "detect_bag_type",
           "SyntheticNoiseGenerator", "NoiseAugmentor", "NoiseLabel", "NoiseBatch", "training_targets",
           "Alignment", "GroundTruth", "align_survey_pair", "compute_ground_truth", "ground_truth_stats",
           "analyze_noise_patterns", "print_analysis",
           "FEATURE_CLASSES", "FeatureLabels", "S57Feature", "create_feature_labels", "feature_pixel_table", "feature_plan",
           "rasterize_features", "ReviewRegions", "export_review_regions",
           "add_feature_labels", "create_feature_mask_from_slope", "slope_cut", "wreck_pixel_table",
           "NativeGroundTruth", "VRPairTable", "compute_ground_truth_native", "vr_pair_table",
           "SoundingGrid", "SoundingGridder", "grid_soundings", "plan_sounding_grid", "sounding_extent",
           "RobustSoundingGrid", "RobustSoundingGridder", "grid_soundings_robust",
           "VRLayout", "VRLayoutPlanner", "VRSoundingGrid", "VRSoundingGridder", "RobustVRSoundingGrid", "RobustVRSoundingGridder",
           "plan_vr_base_grid", "plan_vr_layout", "HypothesisGrid", "VRHypothesisGrid",
           "guide_from_coarser", "locale_guide", "locale_guide_planes"]
