"""ctypes binding of ``libbgnn_hip.so`` (C ABI: ``include/bgnn.h``, training part ``include/bgnn_train.h``) and per-GPU contexts.

There is deliberately no CPU fallback: if the library is missing or no GPU is visible the
compute entry points raise.  PyTorch is used only as the container for device memory and
streams (``tensor.data_ptr()``, ``torch.cuda.Stream``).
"""
from __future__ import annotations

import ctypes as C
import os
import threading
from typing import Dict, Optional

import numpy as np
import torch

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG_DIR, "libbgnn_hip.so")

K_NAMES = ["scan", "stats", "features", "export", "gemm", "attcoef", "aggregate", "heads", "scatter", "fused"]
K_INDEX = {n: i for i, n in enumerate(K_NAMES)}

NODE_FEATURE_IDS = {"depth": 0, "local_mean": 1, "local_std": 2, "gradient_x": 3, "gradient_y": 4,
                    "gradient_magnitude": 5, "curvature": 6, "uncertainty": 7}
EDGE_FEATURE_IDS = {"distance": 0, "depth_difference": 1, "slope": 2}
EF_ZERO = 3

ERR_INVALID, ERR_HIP, ERR_NOMEM, ERR_UNSUPPORTED = -1, -2, -3, -4
ABI_VERSION = 7
MATRIX_PATHS = {"exact_f32": 0, "bf16x3": 1, "fp16x3": 2, "bf16": 3}
# every int option of a context (include/bgnn.h, bgnn_ctx_set_option; the "diag_*" / "gemm_diag" ones only take non-zero values in
# the diagnostic build)
OPTION_NAMES = ("matrix_path", "fused", "fold_extractor", "ragged_atlas", "features_tiled", "fused_front",
                "bf16_two_phase", "bf16_layer0_af", "stats_narrow", "diag_mask", "diag_stamps",
                "gemm_diag", "gemm_pair_major", "fused_light_form")


GNN_TYPES = {"GAT": 0, "GCN": 1, "GraphSAGE": 2, "GIN": 3}      # BGNN_GNN_*


class ModelDesc(C.Structure):
    _fields_ = [("in_channels", C.c_int32), ("hidden", C.c_int32), ("num_layers", C.c_int32),
                ("heads", C.c_int32), ("num_classes", C.c_int32), ("edge_dim", C.c_int32),
                ("predict_correction", C.c_int32), ("bn_eps", C.c_float), ("gnn_type", C.c_int32)]


class Tiles(C.Structure):
    _fields_ = [("n_tiles", C.c_int32), ("hw", C.POINTER(C.c_int32)), ("resolution", C.POINTER(C.c_double)),
                ("depth", C.c_void_p), ("mask", C.c_void_p), ("uncertainty", C.c_void_p)]


class GraphOpts(C.Structure):
    _fields_ = [("connectivity", C.c_int32), ("include_self_loops", C.c_int32),
                ("n_node_features", C.c_int32), ("node_features", C.c_int32 * 8),
                ("n_edge_features", C.c_int32), ("edge_features", C.c_int32 * 4)]


class Outputs(C.Structure):
    _fields_ = [("class_logits", C.c_void_p), ("class_probs", C.c_void_p), ("predicted_class", C.c_void_p),
                ("confidence", C.c_void_p), ("correction", C.c_void_p), ("action", C.c_void_p),
                ("needs_review", C.c_void_p), ("auto_correct", C.c_void_p), ("hidden", C.c_void_p)]


class Dropout(C.Structure):
    """bgnn_dropout: the four dropout probabilities of a training-mode forward and the seed of its counter-based draws."""
    _fields_ = [("p_extractor", C.c_float), ("p_attention", C.c_float), ("p_features", C.c_float), ("p_heads", C.c_float),
                ("seed", C.c_uint64)]


class OutputGrads(C.Structure):
    """bgnn_output_grads: device pointers of the gradients of the four differentiable outputs (any may be NULL)."""
    _fields_ = [("class_logits", C.c_void_p), ("class_probs", C.c_void_p), ("confidence", C.c_void_p), ("correction", C.c_void_p)]


# symbol -> (restype, argtypes); every symbol include/bgnn.h declares
_SIGNATURES = {
    "bgnn_abi_version": (C.c_int, []),
    "bgnn_last_error": (C.c_char_p, []),
    "bgnn_build_id": (C.c_char_p, []),
    "bgnn_ctx_create": (C.c_int, [C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]),
    "bgnn_ctx_destroy": (C.c_int, [C.c_void_p]),
    "bgnn_ctx_synchronize": (C.c_int, [C.c_void_p]),
    "bgnn_ctx_stream": (C.c_void_p, [C.c_void_p]),
    "bgnn_ctx_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    "bgnn_ctx_get_option": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_int)]),
    "bgnn_ctx_profile": (C.c_int, [C.c_void_p, C.c_uint32]),
    "bgnn_ctx_profile_read": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "bgnn_model_weight_count": (C.c_size_t, [C.POINTER(ModelDesc)]),
    "bgnn_model_create": (C.c_int, [C.c_void_p, C.POINTER(ModelDesc), C.POINTER(C.c_float), C.c_size_t,
                                    C.POINTER(C.c_void_p)]),
    "bgnn_model_destroy": (C.c_int, [C.c_void_p]),
    "bgnn_graph_build": (C.c_int, [C.c_void_p, C.POINTER(Tiles), C.POINTER(GraphOpts), C.POINTER(C.c_void_p)]),
    "bgnn_graph_from_edges": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p,
                                        C.c_int32, C.c_void_p, C.POINTER(C.c_void_p)]),
    "bgnn_graph_destroy": (C.c_int, [C.c_void_p]),
    "bgnn_graph_counts": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32),
                                    C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "bgnn_graph_export": (C.c_int, [C.c_void_p] + [C.c_void_p] * 8),
    "bgnn_graph_scatter": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]),
    "bgnn_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.POINTER(Outputs)]),
    "bgnn_feature_extractor": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "bgnn_heads": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_float, C.POINTER(Outputs)]),
    "bgnn_forward_train": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Outputs)]),
    "bgnn_forward_train_dropout": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Dropout), C.c_void_p, C.c_void_p,
                                             C.POINTER(Outputs)]),
    "bgnn_stitch_tiles": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 6 +
                          [C.c_int32] + [C.c_void_p] * 6 + [C.c_float] + [C.c_void_p] * 4),
    "bgnn_cut_tiles": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                 C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bgnn_tile_valid_counts": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                         C.c_int32, C.c_void_p]),
    "bgnn_vr_unpack": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_int32, C.c_void_p, C.c_double] +
                       [C.c_void_p] * 5),
    "bgnn_vr_apply": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 4 + [C.c_float, C.c_void_p, C.c_void_p]),
    "bgnn_infer_tiles": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Tiles), C.POINTER(GraphOpts), C.c_float,
                                   C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}

# symbol -> (restype, argtypes); every symbol include/bgnn_train.h declares (the backward pass, ABI 7)
_TRAIN_SIGNATURES = {
    "bgnn_tape_bytes": (C.c_size_t, [C.c_void_p, C.c_void_p]),
    "bgnn_forward_train_tape": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Dropout), C.c_void_p, C.c_void_p,
                                          C.POINTER(Outputs), C.c_void_p, C.c_size_t]),
    "bgnn_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(OutputGrads), C.c_void_p]),
}

# symbol -> (restype, argtypes); every symbol include/bgnn_sidecar.h declares (the VR BAG sidecar raster)
_SIDECAR_SIGNATURES = {
    "bgnn_sidecar_table_bytes": (C.c_size_t, [C.c_int32]),
    "bgnn_sidecar_table": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                     C.c_void_p]),
    "bgnn_sidecar_add": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32,
                                   C.c_int32, C.c_int32, C.c_int64] + [C.c_void_p] * 4 + [C.c_int64, C.c_void_p]),
    "bgnn_sidecar_finish": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
}
SIDECAR_MAX_PIXELS = 1 << 28       # BGNN_SIDECAR_MAX_PIXELS


class NoiseParams(C.Structure):
    """bgnn_noise_params: which noise terms run, and the generator parameters that are not drawn."""
    _fields_ = [("enable_gaussian", C.c_int32), ("enable_spikes", C.c_int32), ("enable_blobs", C.c_int32),
                ("enable_systematic", C.c_int32), ("complexity_correlation", C.c_double), ("spike_mag_min", C.c_double),
                ("spike_mag_max", C.c_double), ("seed", C.c_uint64)]


class NoiseBlob(C.Structure):
    """bgnn_noise_blob: centre (row < 0: the floor(centre_u * n_valid)-th valid cell), size, signed magnitude draw."""
    _fields_ = [("row", C.c_int32), ("col", C.c_int32), ("size", C.c_int32), ("pad", C.c_int32), ("centre_u", C.c_double),
                ("magnitude", C.c_double)]


class NoisePlan(C.Structure):
    """bgnn_noise_plan: the scalar draws of one tile and its slice of the blob list."""
    _fields_ = [("sample", C.c_uint64), ("intensity", C.c_double), ("gaussian_std_factor", C.c_double),
                ("spike_density", C.c_double), ("amplitude_factor", C.c_double), ("freq_a", C.c_double), ("freq_b", C.c_double),
                ("phase", C.c_double), ("artifact", C.c_int32), ("blob_first", C.c_int32), ("blob_count", C.c_int32),
                ("pad", C.c_int32)]


class NoiseFields(C.Structure):
    """bgnn_noise_fields: device pointers of supplied per-cell draws (any may be NULL)."""
    _fields_ = [("gaussian", C.c_void_p), ("uniform", C.c_void_p), ("sign", C.c_void_p), ("magnitude", C.c_void_p)]


# symbol -> (restype, argtypes); every symbol include/bgnn_noise.h declares (synthetic training noise)
_NOISE_SIGNATURES = {
    "bgnn_noise_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_void_p, C.c_int32]),
    "bgnn_noise_generate": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(NoiseParams),
                                      C.POINTER(NoisePlan), C.POINTER(NoiseBlob), C.c_int32, C.POINTER(NoiseFields), C.c_void_p,
                                      C.c_size_t] + [C.c_void_p] * 4),
}
NOISE_ARTIFACTS = ("none", "stripe_horizontal", "stripe_vertical", "wave", "gradient_x", "gradient_y", "gradient_diagonal")   # BGNN_NOISE_*



class LossParams(C.Structure):
    """bgnn_loss_params: what a BathymetricGNNLoss holds (class weights, smoothing, Huber delta, class ids, penalties, term weights)."""
    _fields_ = [("num_classes", C.c_int32), ("has_class_weights", C.c_int32), ("class_weights", C.c_double * 16),
                ("label_smoothing", C.c_double), ("delta", C.c_double), ("feature_class", C.c_int32),
                ("feature_noise_class", C.c_int32), ("seafloor_class", C.c_int32), ("shoal_noise_class", C.c_int32),
                ("penalty_weight", C.c_double), ("shoal_penalty", C.c_double), ("deep_penalty", C.c_double),
                ("term_weights", C.c_double * 5)]


class LossInputs(C.Structure):
    """bgnn_loss_inputs: device pointers of the model outputs and targets of one loss call (three may be NULL)."""
    _fields_ = [("logits", C.c_void_p), ("confidence", C.c_void_p), ("correction", C.c_void_p), ("predicted_class", C.c_void_p),
                ("labels", C.c_void_p), ("correction_targets", C.c_void_p), ("noise_mask", C.c_void_p)]


# symbol -> (restype, argtypes); every symbol include/bgnn_loss.h declares (the multi-task training loss)
_LOSS_SIGNATURES = {
    "bgnn_loss_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "bgnn_loss_forward": (C.c_int, [C.c_void_p, C.POINTER(LossParams), C.c_int64, C.POINTER(LossInputs), C.c_void_p, C.c_size_t,
                                    C.c_void_p, C.c_void_p]),
    "bgnn_loss_backward": (C.c_int, [C.c_void_p, C.POINTER(LossParams), C.c_int64, C.POINTER(LossInputs)] + [C.c_void_p] * 5),
}
# launch geometry and table layout of include/bgnn_loss.h (BGNN_LOSS_*)
LOSS_MAX_CLASSES = 16
LOSS_IGNORE_INDEX = -100
LOSS_ROWS_PER_WG = 1024        # rows behind one partial sum
LOSS_FINISH_WIDTH = 256        # partials the finish workgroup reads per pass
LOSS_TERMS = ("classification", "correction", "confidence", "feature_preservation", "shoal_safety", "total")
LOSS_COUNTS = ("n_masked", "false_positives", "shoal_false_positives", "deep_false_positives", "n_ignored", "n_invalid",
               "feature_as_noise")
LOSS_N_SUMS = 4



class AdamWSlot(C.Structure):
    """bgnn_adamw_slot: one updated tensor of the blob and the number of steps it has taken, this one included."""
    _fields_ = [("offset", C.c_uint64), ("count", C.c_uint64), ("step", C.c_int64)]


class AdamWParams(C.Structure):
    """bgnn_adamw_params: the per-call scalars of bgnn_adamw_step (max_norm <= 0 or inf: no clipping)."""
    _fields_ = [("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double),
                ("weight_decay", C.c_double), ("max_norm", C.c_double)]


# symbol -> (restype, argtypes); every symbol include/bgnn_optim.h declares (fused clip + AdamW, in-place model refresh)
_OPTIM_SIGNATURES = {
    "bgnn_adamw_step": (C.c_int, [C.c_void_p] + [C.c_void_p] * 4 + [C.c_size_t, C.POINTER(AdamWSlot), C.c_int32,
                                  C.POINTER(AdamWParams), C.c_void_p]),
    "bgnn_model_refresh_prepare": (C.c_int, [C.c_void_p, C.c_void_p]),
    "bgnn_model_refresh": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32]),
}
ADAMW_CHUNK = 2048                 # BGNN_ADAMW_CHUNK
REFRESH_ALL, REFRESH_STATS = 0, 1  # BGNN_REFRESH_*


# symbol -> (restype, argtypes); every symbol include/bgnn_trainer.h declares (per-node training targets, epoch bookkeeping)
_TRAINER_SIGNATURES = {
    "bgnn_training_targets": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 7),
    "bgnn_epoch_accumulate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "bgnn_epoch_reset": (C.c_int, [C.c_void_p, C.c_void_p]),
}
TARGETS_SYNTHETIC, TARGETS_GROUND_TRUTH = 0, 1     # BGNN_TARGETS_*
EPOCH_MAX_CLASSES = 16                             # BGNN_EPOCH_MAX_CLASSES
EPOCH_ACC_BYTES = 72 + 8 * EPOCH_MAX_CLASSES * EPOCH_MAX_CLASSES   # BGNN_EPOCH_ACC_BYTES: double [6] | int64 nodes, correct, steps | int64 [16 * 16]


# symbol -> (restype, argtypes); every symbol include/bgnn_eval.h declares (ground truth from a survey pair, model evaluation)
_EVAL_SIGNATURES = {
    "bgnn_ground_truth_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "bgnn_ground_truth_build": (C.c_int, [C.c_void_p] + [C.c_void_p] * 3 + [C.c_int64, C.c_double, C.c_double, C.c_void_p, C.c_size_t] +
                                [C.c_void_p] * 4),
    "bgnn_eval_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "bgnn_eval_reset": (C.c_int, [C.c_void_p, C.c_void_p]),
    "bgnn_eval_accumulate": (C.c_int, [C.c_void_p] + [C.c_void_p] * 3 + [C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p]),
}
# BGNN_GT_STATS_*: int64 valid, noise, seafloor | float64 noise_abs_sum, seafloor_sum | float32 offset, noise_abs_max
GT_STATS_BYTES = 48
GT_STATS_DTYPE = [("valid", "<i8"), ("noise", "<i8"), ("seafloor", "<i8"), ("noise_abs_sum", "<f8"), ("seafloor_sum", "<f8"),
                  ("offset", "<f4"), ("noise_abs_max", "<f4")]
# BGNN_EVAL_ACC_*: the accumulator block of an evaluation
EVAL_THRESHOLDS = (0.5, 0.6, 0.7, 0.8, 0.9)
EVAL_ACC_BYTES = 264
EVAL_ACC_DTYPE = [("total", "<i8"), ("correct", "<i8"), ("confusion", "<i8", (4, 4)), ("covered", "<i8", (5,)),
                  ("covered_correct", "<i8", (5,)), ("conf_sum", "<f8"), ("conf_sq", "<f8"), ("conf_correct_sum", "<f8"),
                  ("conf_incorrect_sum", "<f8"), ("conf_cells", "<i8")]


# symbol -> (restype, argtypes); every symbol include/bgnn_analysis.h declares (noise pattern analysis of a ground truth)
_ANALYSIS_SIGNATURES = {
    "bgnn_noise_analysis_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "bgnn_noise_analysis": (C.c_int, [C.c_void_p] + [C.c_void_p] * 4 + [C.c_int64, C.c_int64, C.c_void_p, C.c_size_t] + [C.c_void_p] * 3),
}
# BGNN_NA_*: the result block of a noise pattern analysis
NA_MAX_CELLS = 2 ** 31 - 1
NA_DEPTH_EDGES = (0, 10, 20, 50, 100, 200, 500, 1000, 10000)
NA_SIZE_EDGES = (1, 2, 5, 10, 50, 100, 1000, 10000)
NA_BYTES = 528
NA_DTYPE = [("valid", "<i8"), ("noise", "<i8"), ("seafloor", "<i8"), ("positive", "<i8"), ("negative", "<i8"), ("nonfinite", "<i8"),
            ("bin_noise", "<i8", (8,)), ("bin_valid", "<i8", (8,)), ("abs_sum", "<f8"), ("sq_sum", "<f8"), ("dev_sq_sum", "<f8"),
            ("pos_sum", "<f8"), ("neg_sum", "<f8"), ("bin_abs_sum", "<f8", (8,)), ("abs_max", "<f4"), ("pad", "<f4"),
            ("mag_rank", "<i8", (6,)), ("mag_value", "<f4", (6,)), ("num_clusters", "<i8"), ("cluster_cells", "<i8"),
            ("max_cluster", "<i8"), ("isolated", "<i8"), ("size_bins", "<i8", (7,)), ("size_mid", "<i8", (2,)),
            ("rough_count", "<i8", (2,)), ("rough_sum", "<f8", (2,)), ("rough_mid", "<f8", (4,))]


# symbol -> (restype, argtypes); every symbol include/bgnn_review.h declares (low-confidence regions for review)
_REVIEW_SIGNATURES = {
    "bgnn_review_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "bgnn_review_regions": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_float, C.c_float, C.c_int64, C.c_void_p, C.c_size_t,
                                      C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
}
# BGNN_RV_*: the limit, the counts and the record of a kept region (bgnn_review_record)
RV_MAX_CELLS = 2 ** 31 - 1
RV_COUNTS = 4
RV_COUNT_NAMES = ("uncertain_cells", "regions", "kept_regions", "kept_cells")
RV_FIXED_BYTES = 81920
RV_RECORD_DTYPE = np.dtype([("first", "<i8"), ("size", "<i8"), ("min_row", "<i4"), ("max_row", "<i4"), ("min_col", "<i4"),
                            ("max_col", "<i4"), ("conf_sum", "<u8")])
RV_RECORD_BYTES = RV_RECORD_DTYPE.itemsize


# symbol -> (restype, argtypes); every symbol include/bgnn_features.h declares (feature labels from charted objects)
_FEATURES_SIGNATURES = {
    "bgnn_feature_labels_plan_bytes": (C.c_size_t, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64]),
    "bgnn_feature_labels_plan": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_size_t]),
    "bgnn_feature_labels_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_size_t]),
    "bgnn_feature_labels": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_double, C.c_void_p, C.c_int64,
                                      C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
}
# BGNN_FL_*: the bins of the host plan, the limits, the statistics block of a feature-label call
FL_BIN = 64
FL_MAX_CELLS = 2 ** 31 - 1
FL_MAX_FEATURES = 2 ** 31 - 2
FL_STATS_BYTES = 24
FL_STATS_DTYPE = [("valid", "<i8"), ("feature", "<i8"), ("painted", "<i8")]


# symbol -> (restype, argtypes); every symbol include/bgnn_slope.h declares (slope-based feature labels)
_SLOPE_SIGNATURES = {
    "bgnn_slope_features_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "bgnn_slope_features": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_double, C.c_float, C.c_int64,
                                      C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
}
# BGNN_SL_*: the limit and the statistics block of a slope-feature call
SL_MAX_CELLS = 2 ** 31 - 1
SL_STATS = 6
SL_STATS_BYTES = 48
SL_STATS_NAMES = ("valid_cells", "steep_cells", "clusters", "kept_clusters", "kept_cells", "slope_feature_cells")


# symbol -> (restype, argtypes); every symbol include/bgnn_tilestore.h declares (training tiles cut from planes in HBM)
_TILESTORE_SIGNATURES = {
    "bgnn_tile_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "bgnn_tile_scan": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_double, C.c_void_p, C.c_int64,
                                 C.c_void_p, C.c_size_t, C.c_void_p]),
    "bgnn_tile_cut": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_int32,
                                C.c_double, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_size_t]),
}
TILE_VALID_LABEL, TILE_VALID_DEPTH = 0, 1          # BGNN_TILE_VALID_*
TILE_MAX_PLANES = 4                                # BGNN_TILE_MAX_PLANES
TILE_BAND_ROWS = 32                                # BGNN_TILE_BAND_ROWS
TILE_COUNTS = 4                                    # BGNN_TILE_COUNTS: valid, class 0, class 1, class 2
# bgnn_tile_box (BGNN_TILE_BOX_BYTES = 32)
TILE_BOX_DTYPE = np.dtype([("row0", "<i8"), ("col0", "<i8"), ("h", "<i4"), ("w", "<i4"), ("dst", "<i8")])
TILE_BOX_BYTES = TILE_BOX_DTYPE.itemsize


# symbol -> (restype, argtypes); every symbol include/bgnn_augment.h declares (tiles gathered under the symmetries of the square)
_AUGMENT_SIGNATURES = {
    "bgnn_tile_gather_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "bgnn_tile_gather": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                   C.c_void_p, C.c_int64, C.c_void_p, C.c_size_t]),
}
AUG_OPS = 8                                        # BGNN_AUG_OPS: op = k + 4 * f
AUG_MAX_PLANES = 4                                 # BGNN_AUG_MAX_PLANES
AUG_BLOCK = 64                                     # BGNN_AUG_BLOCK
# bgnn_tile_entry (BGNN_AUG_ENTRY_BYTES = 32); h, w: the SOURCE tile
TILE_ENTRY_DTYPE = np.dtype([("src", "<i8"), ("dst", "<i8"), ("h", "<i4"), ("w", "<i4"), ("op", "<i4"), ("pad", "<i4")])
AUG_ENTRY_BYTES = TILE_ENTRY_DTYPE.itemsize


# symbol -> (restype, argtypes); every symbol include/bgnn_vrtruth.h declares (native-resolution ground truth from a VR BAG pair)
_VRTRUTH_SIGNATURES = {
    "bgnn_vr_ground_truth_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "bgnn_vr_ground_truth": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64,
                                       C.c_double, C.c_double, C.c_void_p, C.c_size_t] + [C.c_void_p] * 7),
}
VT_TILE_CELLS = 1024                               # BGNN_VT_TILE_CELLS
VT_COUNTS = 4                                      # BGNN_VT_COUNTS: valid, class 0, class 1, class 2
# bgnn_vr_pair (BGNN_VT_PAIR_BYTES = 32)
VT_PAIR_DTYPE = np.dtype([("out_offset", "<i8"), ("cells", "<i8"), ("noisy_start", "<i8"), ("clean_start", "<i8")])
VT_PAIR_BYTES = VT_PAIR_DTYPE.itemsize
# BGNN_VT_STATS_*: int64 valid, noise, seafloor | float64 noise_abs_sum, noise_abs_median | float32 noise_abs_max, pad
VT_STATS_BYTES = 48
VT_STATS_DTYPE = [("valid", "<i8"), ("noise", "<i8"), ("seafloor", "<i8"), ("noise_abs_sum", "<f8"), ("noise_abs_median", "<f8"),
                  ("noise_abs_max", "<f4"), ("pad", "<i4")]


# symbol -> (restype, argtypes); every symbol include/bgnn_curve.h declares (operating curves: threshold sweep, correction residuals)
_CURVE_SIGNATURES = {
    "bgnn_curve_block_bytes": (C.c_size_t, [C.c_int]),
    "bgnn_curve_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "bgnn_curve_accumulate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_int64, C.c_void_p]),
}
CURVE_MAX_THRESHOLDS = 128                         # BGNN_CURVE_MAX_THRESHOLDS
CURVE_WG_CELLS = 1024                              # BGNN_CURVE_WG_CELLS: one workgroup's share of the cells
CURVE_MAX_GRID = 1024                              # BGNN_CURVE_MAX_GRID
CURVE_RES_CAP = 32768                              # BGNN_CURVE_RES_CAP
CURVE_RES_SCALE = 65536                            # BGNN_CURVE_RES_SCALE


def curve_block_dtype(n_thresholds: int):
    """The record of the block of a table of ``n_thresholds`` entries (BGNN_CURVE_*(T)): int64 throughout, B = 2T + 2 codes."""
    b = 2 * int(n_thresholds) + 2
    return [("counts", "<i8", (b, 4, 4)), ("res_cells", "<i8", (b, 4)), ("abs_before", "<i8", (b, 4)), ("abs_after", "<i8", (b, 4)),
            ("base_cells", "<i8", (4,)), ("base_abs", "<i8", (4,)), ("res_skipped", "<i8")]


# symbol -> (restype, argtypes); every symbol include/bgnn_soundings.h declares (gridding a point cloud of soundings)
_SOUNDINGS_SIGNATURES = {
    "bgnn_soundings_state_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "bgnn_soundings_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64]),
    "bgnn_soundings_add": (C.c_int, [C.c_void_p] * 4 + [C.c_int64] + [C.c_double] * 3 + [C.c_int64] * 3 + [C.c_void_p]),
    "bgnn_soundings_finalize": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_float] + [C.c_void_p] * 6),
    "bgnn_soundings_extent": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
}
SOUNDINGS_HEADER_BYTES = 32                        # BGNN_SOUNDINGS_HEADER_BYTES
SOUNDINGS_CELL_BYTES = 40                          # BGNN_SOUNDINGS_CELL_BYTES
SOUNDINGS_MAX_TOTAL = 2 ** 31 - 1                  # BGNN_SOUNDINGS_MAX_TOTAL
SOUNDINGS_Z_CAP = 32768                            # BGNN_SOUNDINGS_Z_CAP
SOUNDINGS_SCALE = 65536                            # BGNN_SOUNDINGS_SCALE
SOUNDINGS_EXTENT_BUFFER_BYTES = 48 * 1025          # BGNN_SOUNDINGS_EXTENT_BUFFER_BYTES
SOUNDINGS_COUNTERS = ("accepted", "nonfinite", "outside", "out_of_range")
# BGNN_SOUNDINGS_EXTENT_BYTES: the record in front of the extent buffer
SOUNDINGS_EXTENT_DTYPE = np.dtype([("min_x", "<f8"), ("max_x", "<f8"), ("min_y", "<f8"), ("max_y", "<f8"), ("finite_x", "<i8"),
                                   ("finite_y", "<i8")])

# symbol -> (restype, argtypes); every symbol include/bgnn_soundings_robust.h declares (robust gridding: per-cell median, MAD, flags)
_ROBUST_SIGNATURES = {
    "bgnn_soundings_robust_stage_bytes": (C.c_size_t, [C.c_int64]),
    "bgnn_soundings_robust_workspace_bytes": (C.c_size_t, [C.c_int64] * 3),
    "bgnn_soundings_robust_reset": (C.c_int, [C.c_void_p, C.c_void_p]),
    "bgnn_soundings_robust_add": (C.c_int, [C.c_void_p] * 4 + [C.c_int64] + [C.c_double] * 3 + [C.c_int64] * 4 + [C.c_void_p]),
    "bgnn_soundings_robust_finalize": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int64] * 4 + [C.c_double] * 2 + [C.c_int32, C.c_float,
                                                 C.c_void_p, C.c_size_t] + [C.c_void_p] * 13),
    "bgnn_soundings_robust_flag": (C.c_int, [C.c_void_p] * 4 + [C.c_int64] + [C.c_double] * 3 + [C.c_int64] * 2 + [C.c_void_p] * 3),
}
ROBUST_STAGE_HEADER_BYTES = 32                     # BGNN_ROBUST_STAGE_HEADER_BYTES
ROBUST_SLOT_BYTES = 8                              # BGNN_ROBUST_SLOT_BYTES
ROBUST_MAX_CAPACITY = 2 ** 31 - 1                  # BGNN_ROBUST_MAX_CAPACITY
ROBUST_MAX_CELLS = 2 ** 31 - 1                     # BGNN_ROBUST_MAX_CELLS
ROBUST_WAVE_MAX = 64                               # BGNN_ROBUST_WAVE_MAX: the longest segment ranked inside a wave
ROBUST_LDS_MAX = 4096                              # BGNN_ROBUST_LDS_MAX: the longest segment one workgroup sorts in LDS
ROBUST_FLAGS = ("kept", "rejected", "not_accepted")  # BGNN_ROBUST_FLAG_*: 0, 1, 2

# symbol -> (restype, argtypes); every symbol include/bgnn_soundings_vr.h declares (gridding soundings at variable resolution)
_VR_CLOUD = [C.c_void_p] * 4 + [C.c_int64] + [C.c_double] * 3 + [C.c_int64] * 2       # ctx, x, y, z, n, x0, y0, base_res, BH, BW
_VR_SOUNDINGS_SIGNATURES = {
    "bgnn_vr_soundings_plan_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "bgnn_vr_soundings_density": (C.c_int, _VR_CLOUD + [C.c_void_p]),
    "bgnn_vr_soundings_plan": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_int64, C.c_int64,
                                         C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "bgnn_vr_soundings_add": (C.c_int, _VR_CLOUD + [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    "bgnn_vr_soundings_stage": (C.c_int, _VR_CLOUD + [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    "bgnn_vr_soundings_flag": (C.c_int, _VR_CLOUD + [C.c_void_p, C.c_int64] + [C.c_void_p] * 3),
}
VR_ENTRY_BYTES = 16                                # BGNN_VR_ENTRY_BYTES
VR_ENTRY_DTYPE = np.dtype([("index", "<i8"), ("dx", "<i4"), ("dy", "<i4")])
VR_MAX_DIM = 32768                                 # BGNN_VR_MAX_DIM
VR_MAX_RUNGS = 16                                  # BGNN_VR_MAX_RUNGS
VR_MAX_BASE_CELLS = 2 ** 31 - 1                    # BGNN_VR_MAX_BASE_CELLS
VR_MAX_RECORDS = 2 ** 31 - 1                       # BGNN_VR_MAX_RECORDS
VR_MAX_TARGET = 2 ** 31 - 1                        # BGNN_VR_MAX_TARGET
VR_PLAN_TILE = 256                                 # BGNN_VR_PLAN_TILE
VR_SOUNDINGS_COUNTERS = SOUNDINGS_COUNTERS + ("unrefined",)

# symbol -> (restype, argtypes); every symbol include/bgnn_hypotheses.h declares (depth hypotheses per cell: runs of the sorted lists)
_HYPOTHESES_SIGNATURES = {
    "bgnn_hypotheses_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "bgnn_hypotheses_build": (C.c_int, [C.c_void_p] * 3 + [C.c_int64] * 3 + [C.c_int32, C.c_void_p, C.c_int32, C.c_float, C.c_void_p,
                                        C.c_size_t] + [C.c_void_p] * 14),
}
HYP_RULES = ("count", "guide")                     # BGNN_HYP_RULE_COUNT, BGNN_HYP_RULE_GUIDE: 0, 1
HYP_MAX_CELLS = 2 ** 31 - 1                        # BGNN_HYP_MAX_CELLS
HYP_MAX_CAPACITY = 2 ** 31 - 1                     # BGNN_HYP_MAX_CAPACITY
HYP_MAX_GAP_Q = 2 ** 32                            # BGNN_HYP_MAX_GAP_Q

# symbol -> (restype, argtypes); every symbol include/bgnn_locale.h declares (the locale rule: a guide from single-hypothesis neighbours)
_LOCALE_SIGNATURES = {
    "bgnn_locale_guide": (C.c_int, [C.c_void_p] * 4 + [C.c_int64] * 2 + [C.c_int32] * 2 + [C.c_void_p] * 2),
}
LOCALE_MAX_RADIUS = 8                              # BGNN_LOCALE_MAX_RADIUS
LOCALE_MAX_CELLS = 2 ** 31 - 1                     # height * width of bgnn_locale_guide

# symbol -> (restype, argtypes); every symbol include/bgnn_aux.h declares (auxiliary node-feature planes: sounding density)
_AUX_SIGNATURES = {
    "bgnn_graph_build_aux": (C.c_int, [C.c_void_p, C.POINTER(Tiles), C.POINTER(GraphOpts), C.c_int32, C.POINTER(C.c_void_p),
                                       C.POINTER(C.c_void_p)]),
    "bgnn_infer_tiles_aux": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Tiles), C.POINTER(GraphOpts), C.c_int32,
                                       C.POINTER(C.c_void_p), C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p]),
}
AUX_MAX_PLANES = 8                                 # BGNN_AUX_MAX_PLANES
AUX_ROW_FLOATS = 16                                # BGNN_AUX_ROW_FLOATS
# the planes a model may take beside the computed node features, in column order (checkpoints: "node_planes")
NODE_PLANES = ("uncertainty", "sounding_density")

# symbol -> (restype, argtypes); every symbol include/bgnn_quantile.h declares (exact percentiles of errors that stay on the device)
_QUANTILE_SIGNATURES = {
    "bgnn_quantile_reset": (C.c_int, [C.c_void_p, C.c_void_p]),
    "bgnn_quantile_add": (C.c_int, [C.c_void_p, C.c_int64] + [C.c_void_p] * 4 + [C.c_int64, C.c_void_p]),
    "bgnn_quantile_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "bgnn_quantile_select": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(C.c_double), C.c_int32, C.c_void_p,
                                       C.c_size_t, C.c_void_p]),
}
QUANTILE_MAX_FRACTIONS = 3                         # BGNN_QUANTILE_MAX_FRACTIONS
QUANTILE_TOP_BITS = 11                             # BGNN_QUANTILE_TOP_BITS
QUANTILE_MAX_GRID = 2048                           # BGNN_QUANTILE_MAX_GRID
QUANTILE_WG_ROWS = 4096                            # BGNN_QUANTILE_WG_ROWS: one workgroup's share of the rows, one slot reservation
QUANTILE_MAX_CAPACITY = 2 ** 32 - 1
# BGNN_QUANTILE_ST_*: the state block, BGNN_QUANTILE_STATE_BYTES
QUANTILE_STATE_DTYPE = np.dtype([("rows", "<i8"), ("filed", "<i8"), ("nonfinite", "<i8"), ("dropped", "<i8"), ("cursor", "<i8"),
                                 ("reserved", "<i8", (3,)), ("hist", "<u4", (1 << QUANTILE_TOP_BITS,))])
QUANTILE_STATE_BYTES = QUANTILE_STATE_DTYPE.itemsize
# BGNN_QUANTILE_OUT_*: the result block of a selection, BGNN_QUANTILE_OUT_BYTES
QUANTILE_OUT_DTYPE = np.dtype([("count", "<i8"), ("nonfinite", "<i8"), ("dropped", "<i8"), ("rows", "<i8"),
                               ("ranks", [("lo", "<i8"), ("hi", "<i8"), ("v_lo", "<f4"), ("v_hi", "<f4")], (QUANTILE_MAX_FRACTIONS,))])
QUANTILE_OUT_BYTES = QUANTILE_OUT_DTYPE.itemsize


_lib = None
_lib_lock = threading.Lock()


class BgnnError(RuntimeError):
    pass


def load_library(path: Optional[str] = None):
    """dlopen the HIP library and bind every symbol of include/bgnn.h, include/bgnn_train.h, include/bgnn_sidecar.h,
    include/bgnn_noise.h, include/bgnn_loss.h, include/bgnn_optim.h, include/bgnn_trainer.h, include/bgnn_eval.h, include/bgnn_analysis.h,
    include/bgnn_features.h, include/bgnn_tilestore.h, include/bgnn_review.h, include/bgnn_slope.h, include/bgnn_vrtruth.h,
    include/bgnn_augment.h, include/bgnn_curve.h, include/bgnn_soundings.h, include/bgnn_soundings_robust.h,
    include/bgnn_soundings_vr.h, include/bgnn_hypotheses.h, include/bgnn_locale.h, include/bgnn_aux.h and include/bgnn_quantile.h.
    Needs no GPU."""
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        p = path or os.environ.get("BGNN_LIB", LIB_PATH)
        if not os.path.exists(p):
            raise ImportError(
                f"{p} not found: the HIP library is not built. Run `python __graft_entry__.py` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        lib = C.CDLL(p)
        for name, (res, args) in list(_SIGNATURES.items()) + list(_TRAIN_SIGNATURES.items()) + list(_SIDECAR_SIGNATURES.items()) + \
                list(_NOISE_SIGNATURES.items()) + list(_LOSS_SIGNATURES.items()) + list(_OPTIM_SIGNATURES.items()) + list(_TRAINER_SIGNATURES.items()) + \
                list(_EVAL_SIGNATURES.items()) + list(_ANALYSIS_SIGNATURES.items()) + list(_FEATURES_SIGNATURES.items()) + \
                list(_TILESTORE_SIGNATURES.items()) + list(_REVIEW_SIGNATURES.items()) + list(_SLOPE_SIGNATURES.items()) + \
                list(_VRTRUTH_SIGNATURES.items()) + list(_AUGMENT_SIGNATURES.items()) + list(_CURVE_SIGNATURES.items()) + \
                list(_SOUNDINGS_SIGNATURES.items()) + list(_ROBUST_SIGNATURES.items()) + list(_VR_SOUNDINGS_SIGNATURES.items()) + \
                list(_HYPOTHESES_SIGNATURES.items()) + list(_LOCALE_SIGNATURES.items()) + list(_AUX_SIGNATURES.items()) + \
                list(_QUANTILE_SIGNATURES.items()):
            fn = getattr(lib, name)          # AttributeError if the .so lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        if lib.bgnn_abi_version() != ABI_VERSION:
            raise ImportError(f"{p}: ABI version {lib.bgnn_abi_version()} != {ABI_VERSION}")
        _lib = lib
        return lib


def build_id() -> str:
    """The kernel-source hash the loaded library was built from (``bgnn_build_id``)."""
    return load_library().bgnn_build_id().decode()


def check(rc: int):
    if rc == 0:
        return
    msg = load_library().bgnn_last_error().decode(errors="replace")
    if rc == ERR_INVALID:
        raise ValueError(msg)
    if rc == ERR_UNSUPPORTED:
        raise NotImplementedError(msg)
    if rc == ERR_NOMEM:
        raise MemoryError(msg)
    raise BgnnError(msg)


def ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


class Context:
    """One library context per (process, GPU): owns a HIP stream (created through torch so that
    torch events / stream waits can order against it) and the library's device arenas."""

    def __init__(self, device: torch.device):
        self.lib = load_library()
        if not torch.cuda.is_available():
            raise BgnnError("no GPU visible: bathymetric_gnn_amd computes only on an MI355X "
                            "(there is no CPU fallback)")
        self.device = torch.device("cuda", device.index if device.index is not None else torch.cuda.current_device())
        with torch.cuda.device(self.device):
            self.stream = torch.cuda.Stream(self.device)
        h = C.c_void_p()
        check(self.lib.bgnn_ctx_create(self.device.index, C.c_void_p(self.stream.cuda_stream), C.byref(h)))
        self.handle = h
        self._closers = []                 # run by close() before the context goes: packed models that live on it

    def on_close(self, fn):
        """``fn()`` is called when this context is closed (objects that hold library handles created on it)."""
        self._closers.append(fn)

    def close(self):
        """Release the context (stream-synchronised): first whatever registered through ``on_close`` (packed models), then the
        library context with its arenas.  Graph objects built on it must not be used afterwards.  Idempotent."""
        if getattr(self, "handle", None) is None:
            return
        for fn in reversed(getattr(self, "_closers", [])):
            try:
                fn()
            except Exception:
                pass
        self._closers = []
        h, self.handle = self.handle, None
        self.lib.bgnn_ctx_destroy(h)

    # -- ordering against the caller's current torch stream ------------------------------------
    def begin(self):
        self.stream.wait_stream(torch.cuda.current_stream(self.device))

    def end(self):
        torch.cuda.current_stream(self.device).wait_stream(self.stream)

    def synchronize(self):
        check(self.lib.bgnn_ctx_synchronize(self.handle))

    # -- run-time switches (include/bgnn.h: bgnn_ctx_set_option).  The environment is read once, when the
    #    context is created; afterwards only these calls change a switch.
    def set_option(self, name: str, value):
        if name == "matrix_path" and isinstance(value, str):
            value = MATRIX_PATHS[value]
        check(self.lib.bgnn_ctx_set_option(self.handle, name.encode(), int(value)))

    def get_option(self, name: str) -> int:
        v = C.c_int()
        check(self.lib.bgnn_ctx_get_option(self.handle, name.encode(), C.byref(v)))
        return v.value

    def copy_options_from(self, other: "Context"):
        """Give this context every run-time switch of ``other`` (OPTION_NAMES)."""
        for k in OPTION_NAMES:
            v = other.get_option(k)
            if self.get_option(k) != v:
                self.set_option(k, v)

    def options(self, **kw):
        """``with ctx.options(matrix_path="bf16x3"): ...`` -- set, run, restore."""
        ctx = self

        class _Scope:
            def __enter__(self_):
                self_.old = {k: ctx.get_option(k) for k in kw}
                for k, v in kw.items():
                    ctx.set_option(k, v)
                return ctx

            def __exit__(self_, *exc):
                for k, v in self_.old.items():
                    ctx.set_option(k, v)
                return False
        return _Scope()

    def profile(self, kernels):
        mask = 0
        for k in kernels:
            mask |= 1 << (K_INDEX[k] if isinstance(k, str) else int(k))
        check(self.lib.bgnn_ctx_profile(self.handle, mask))

    def profile_read(self) -> Dict[str, Dict[str, float]]:
        ms = (C.c_double * len(K_NAMES))()
        n = (C.c_int64 * len(K_NAMES))()
        check(self.lib.bgnn_ctx_profile_read(self.handle, ms, n))
        return {K_NAMES[i]: {"ms": ms[i], "launches": int(n[i])} for i in range(len(K_NAMES))}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_contexts: Dict[int, Context] = {}
_ctx_lock = threading.Lock()


def resolve_device(device=None) -> torch.device:
    if device is None:
        if not torch.cuda.is_available():
            raise BgnnError("no GPU visible: bathymetric_gnn_amd computes only on an MI355X "
                            "(there is no CPU fallback)")
        return torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise BgnnError(f"device {device} unsupported: the hot path runs on the GPU only (no CPU fallback)")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


def get_context(device=None) -> Context:
    device = resolve_device(device)
    with _ctx_lock:
        ctx = _contexts.get(device.index)
        if ctx is None:
            ctx = Context(device)
            _contexts[device.index] = ctx
        return ctx


def new_context(device=None) -> Context:
    """An ADDITIONAL library context on ``device`` (own HIP stream, own arenas): batches submitted to different contexts
    overlap on the GPU -- the tail of one small batch's kernels runs beside the head of the next one's.  The caller keeps
    it alive (models only hold weak references to the contexts they are packed on) and may ``close()`` it; ``get_context`` keeps
    returning the device's default context."""
    return Context(resolve_device(device))


def make_graph_opts(connectivity: str, include_self_loops: bool, node_features, edge_features) -> GraphOpts:
    conn = {"4-connected": 4, "8-connected": 8, "16-dilated": 16}.get(connectivity)
    if conn is None:
        raise ValueError(f"Unknown connectivity: {connectivity}")
    o = GraphOpts()
    o.connectivity = conn
    o.include_self_loops = 1 if include_self_loops else 0
    ids = [NODE_FEATURE_IDS[n] for n in node_features if n in NODE_FEATURE_IDS]   # unknown names are skipped
    if len(ids) > 8:
        raise ValueError("at most 8 node features")
    o.n_node_features = len(ids)
    for i, v in enumerate(ids):
        o.node_features[i] = v
    eids = [EDGE_FEATURE_IDS.get(n, EF_ZERO) for n in edge_features]             # unknown names give 0.0
    if not 1 <= len(eids) <= 4:
        raise ValueError("between 1 and 4 edge features are supported")
    o.n_edge_features = len(eids)
    for i, v in enumerate(eids):
        o.edge_features[i] = v
    return o


def make_tiles(hw: np.ndarray, res: np.ndarray, depth: torch.Tensor, mask: torch.Tensor,
               unc: Optional[torch.Tensor]):
    """hw int32 [T,2], res float64 [T,2] (host); depth/mask/unc flat device tensors.
    Returns (Tiles, keepalive)."""
    hw = np.ascontiguousarray(hw, dtype=np.int32)
    res = np.ascontiguousarray(res, dtype=np.float64)
    t = Tiles()
    t.n_tiles = hw.shape[0]
    t.hw = hw.ctypes.data_as(C.POINTER(C.c_int32))
    t.resolution = res.ctypes.data_as(C.POINTER(C.c_double))
    t.depth = depth.data_ptr()
    t.mask = mask.data_ptr()
    t.uncertainty = unc.data_ptr() if unc is not None else None
    return t, (hw, res, depth, mask, unc)


def make_aux_planes(planes, cells: Optional[int] = None):
    """The HOST pointer array of ``bgnn_graph_build_aux`` / ``bgnn_infer_tiles_aux`` from a sequence of flat float32 device planes.
    Returns (n_aux, array or None, keepalive)."""
    planes = [] if planes is None else list(planes)
    if len(planes) > AUX_MAX_PLANES:
        raise ValueError(f"at most {AUX_MAX_PLANES} auxiliary node planes, got {len(planes)}")
    keep = []
    for i, t in enumerate(planes):
        if t is None:
            raise ValueError(f"auxiliary node plane {i} is None")
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"auxiliary node plane {i} must be a contiguous float32 tensor")
        if cells is not None and t.numel() != cells:
            raise ValueError(f"auxiliary node plane {i} has {t.numel()} cells, the tile table has {cells}")
        keep.append(t)
    if not keep:
        return 0, None, keep
    arr = (C.c_void_p * len(keep))(*[t.data_ptr() for t in keep])
    return len(keep), arr, (keep, arr)
