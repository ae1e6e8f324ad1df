"""ctypes host binding of libr3dm.so -- the C ABI in include/r3dm.h.

This is the Python face of the drop-in boundary used by tests/, bench.py and the multi-GPU
driver.  It contains NO arithmetic: every call goes through the C ABI into the HIP kernels.
If the shared library (or a gfx950 GPU) is missing the calls raise -- there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libr3dm.so")

F32, U8, BIN = 0, 1, 2
KNN_MAX = 8                      # R3DM_KNN_MAX (include/r3dm.h)
LAYOUT_ROWS, LAYOUT_BF16, LAYOUT_SPLIT, LAYOUT_COUNTS, LAYOUT_BIN8 = 1, 2, 4, 8, 16
NONE = 0xFFFFFFFF

EXPORTS = [
    "r3dm_create", "r3dm_destroy", "r3dm_last_error", "r3dm_device_info", "r3dm_set_image", "r3dm_set_images", "r3dm_images_wait", "r3dm_view_info", "r3dm_memory_info", "r3dm_clear_images", "r3dm_trim",
    "r3dm_match_pairs", "r3dm_filter_F", "r3dm_filter_H", "r3dm_knn2", "r3dm_graph_num_pairs", "r3dm_graph_num_matches",
    "r3dm_graph_pairs", "r3dm_graph_offsets", "r3dm_graph_matches", "r3dm_graph_free", "r3dm_graph_from_csr",
    "r3dm_graph_merge", "r3dm_save_matches", "r3dm_load_matches", "r3dm_get_stats", "r3dm_filter_report",
    "r3dm_compute_matches_dir", "r3dm_compute_matches_stage", "r3dm_stage_create", "r3dm_stage_run", "r3dm_stage_destroy", "r3dm_liop_describe_patches", "r3dm_extract_liop",
    "r3dm_set_intrinsics", "r3dm_filter_E", "r3dm_ann_params_for_algorithm", "r3dm_detect_akaze", "r3dm_detect_akaze_mldb", "r3dm_gray_from_bgr8", "r3dm_extract_features_to_files", "r3dm_multi_extract_features",
    "r3dm_detect_akaze_batch", "r3dm_detect_akaze_classic", "r3dm_detect_akaze_classic_batch", "r3dm_extract_features_batch", "r3dm_multi_extract_features_ex", "r3dm_get_features_totals", "r3dm_kgraph_preset", "r3dm_match_pairs_kgraph", "r3dm_exhaustive_is_faster", "r3dm_kgraph_knn2", "r3dm_kgraph_index", "r3dm_drop_indices",
    "r3dm_filter_FEH", "r3dm_host_threads", "r3dm_set_features_sink", "r3dm_multi_set_features_sink", "r3dm_set_deferred_feature_files", "r3dm_set_background_nice", "r3dm_multi_set_background_nice", "r3dm_features_files_wait", "r3dm_multi_set_deferred_feature_files", "r3dm_multi_features_files_wait", "r3dm_hnsw_preset", "r3dm_match_pairs_hnsw", "r3dm_hnsw_knn2", "r3dm_hnsw_knn2_on_index", "r3dm_hnsw_index",
    "r3dm_mrpt_preset", "r3dm_match_pairs_mrpt", "r3dm_mrpt_knn2", "r3dm_mrpt_index", "r3dm_multi_match_pairs_mrpt",
    "r3dm_kgraph_knn", "r3dm_hnsw_knn", "r3dm_hnsw_knn_on_index", "r3dm_mrpt_knn", "r3dm_index_kgraph_knn", "r3dm_index_hnsw_knn", "r3dm_index_mrpt_knn",
    "r3dm_set_integer_mfma", "r3dm_set_split_mfma", "r3dm_set_hamming_mfma", "r3dm_index_create", "r3dm_index_knn2", "r3dm_index_destroy",
    "r3dm_knn", "r3dm_index_knn", "r3dm_set_knn_narrow_tiles", "r3dm_set_knn_hamming_tiles",
    "r3dm_multi_create", "r3dm_multi_destroy", "r3dm_multi_num_devices", "r3dm_multi_ctx", "r3dm_multi_last_error",
    "r3dm_multi_set_image", "r3dm_multi_transfer_counts", "r3dm_multi_set_intrinsics", "r3dm_multi_clear_images", "r3dm_multi_set_integer_mfma",
    "r3dm_multi_match_pairs", "r3dm_multi_match_pairs_kgraph", "r3dm_multi_match_pairs_hnsw", "r3dm_multi_filter_F", "r3dm_multi_filter_H", "r3dm_multi_filter_E", "r3dm_shard_pairs",
    "r3dm_comm_unique_id", "r3dm_comm_create", "r3dm_comm_destroy", "r3dm_comm_rank", "r3dm_comm_world", "r3dm_comm_last_error",
    "r3dm_allgather_graphs", "r3dm_graphs_pack", "r3dm_words_free", "r3dm_graphs_unpack_merge",
    "r3dm_set_device_graphs", "r3dm_graph_on_device", "r3dm_comm_last_device_graphs",
    "r3dm_guided_match", "r3dm_set_guided_matching", "r3dm_guided_report", "r3dm_multi_set_guided_matching",
    "r3dm_set_keypoint_detector", "r3dm_multi_set_keypoint_detector", "r3dm_akaze_classic_components",
    "r3dm_set_mutual_matching", "r3dm_multi_set_mutual_matching", "r3dm_compute_matches_dir_flags",
    "r3dm_set_symmetric_ratio", "r3dm_multi_set_symmetric_ratio", "r3dm_symmetric_ratio_report",
    "r3dm_set_kgraph_hamming", "r3dm_multi_set_kgraph_hamming", "r3dm_kgraph_hamming_report", "r3dm_kgraph_knn2_bits", "r3dm_kgraph_knn_bits",
    "r3dm_set_view_priority", "r3dm_preselect_pairs", "r3dm_set_preemptive_matching", "r3dm_preselect_report",
    "r3dm_multi_set_view_priority", "r3dm_multi_set_preemptive_matching",
    "r3dm_set_match_budget", "r3dm_budget_rows", "r3dm_budget_report", "r3dm_multi_set_match_budget",
    "r3dm_build_tracks", "r3dm_tracks_count", "r3dm_tracks_offsets", "r3dm_tracks_observations", "r3dm_tracks_report", "r3dm_tracks_phase_ms", "r3dm_tracks_in_pair",
    "r3dm_tracks_free",
    "r3dm_detect_akaze_mldb_batch", "r3dm_set_descriptor_arm", "r3dm_multi_set_descriptor_arm",
    "r3dm_set_prefix_pruning", "r3dm_get_prefix_pruning_counts", "r3dm_multi_set_prefix_pruning", "r3dm_multi_get_prefix_pruning_counts",
    "r3dm_get_pair_filter_counts", "r3dm_multi_get_pair_filter_counts",
    "r3dm_set_half_filter", "r3dm_get_half_filter_counts", "r3dm_multi_set_half_filter", "r3dm_multi_get_half_filter_counts",
    "r3dm_get_level2_skip_counts", "r3dm_multi_get_level2_skip_counts",
    "r3dm_set_min_tile_test", "r3dm_get_min_tile_test_counts", "r3dm_multi_set_min_tile_test", "r3dm_multi_get_min_tile_test_counts",
    "r3dm_set_half_prefix", "r3dm_get_half_prefix_counts", "r3dm_multi_set_half_prefix", "r3dm_multi_get_half_prefix_counts",
    "r3dm_detect_akaze_msurf", "r3dm_detect_akaze_msurf_batch",
    "r3dm_vocab_sample", "r3dm_vocab_from_rows", "r3dm_vocab_info", "r3dm_vocab_words", "r3dm_vocab_free", "r3dm_view_signatures", "r3dm_propose_pairs",
    "r3dm_vocab_report", "r3dm_vocab_train", "r3dm_vocab_train_report", "r3dm_vocab_set_weighting", "r3dm_vocab_weights",
]
GUIDED_KIND = {"F": 0, "E": 1, "H": 2}
STAGE_GUIDED_MATCHING = 32
STAGE_DETECTOR_AKAZE = 64
STAGE_MUTUAL_MATCHING = 128
STAGE_PREEMPTIVE_MATCHING = 256
STAGE_DESCRIPTOR_MLDB = 512
STAGE_DESCRIPTOR_MSURF = 1024
STAGE_SYMMETRIC_RATIO = 4096                      # R3DM_STAGE_SYMMETRIC_RATIO: r3dm_set_symmetric_ratio on every context of the stage
STAGE_PAIR_PROPOSAL = 2048                        # R3DM_STAGE_PAIR_PROPOSAL: 16,384 words (half the collection's rows when that is less), top_k 20
VOCAB_MAX_WORDS, VOCAB_HIST_LDS_WORDS, VOCAB_WORD_CHUNK = 65536, 8192, 32      # R3DM_VOCAB_* (include/r3dm.h)
LAYOUT_HEAD = 32                                  # R3DM_LAYOUT_HEAD
LAYOUT_BUDGET = 64                                # R3DM_LAYOUT_BUDGET
BUDGET_SELECT_CHUNK = 256                         # R3DM_BUDGET_SELECT_CHUNK
STAGE_PROPOSAL_TRAINED = 16384                    # R3DM_STAGE_PROPOSAL_TRAINED: with STAGE_PAIR_PROPOSAL, 10 Lloyd updates of the sampled vocabulary + idf weights
STAGE_MATCH_BUDGET = 8192                         # R3DM_STAGE_MATCH_BUDGET: r3dm_set_match_budget with max_rows 8,192 on every context of the stage
DETECTORS = {"Fast-AKAZE": 0, "AKAZE": 1}       # R3DM_DETECTOR_FAST_AKAZE / R3DM_DETECTOR_AKAZE
# the descriptor arms, the rows of csrc/descriptor_arms.hpp (tests/test_descriptor_arms.py holds the two to each other): name, id
# (R3DM_DESCRIPTOR_*; 2 is unassigned), stage flag, numpy dtype and length of a row
_ARMS = [("LIOP", 0, 0, np.float32, 144), ("MLDB", 1, STAGE_DESCRIPTOR_MLDB, np.uint8, 61), ("MSURF", 3, STAGE_DESCRIPTOR_MSURF, np.float32, 64)]
DESCRIPTOR_ARMS = {name: arm_id for name, arm_id, _, _, _ in _ARMS}      # every arm r3dm_set_descriptor_arm takes
DESCRIPTORS = {name: arm_id for name, arm_id in DESCRIPTOR_ARMS.items() if arm_id < 2}      # (the arms before M-SURF: a name the suite pins)
_DESCRIPTOR_STAGE_FLAGS = {name: flag for name, _, flag, _, _ in _ARMS}
_ARM_ROWS = {name: (dtype, dim) for name, _, _, dtype, dim in _ARMS}


def _detector_flag(detector: str) -> int:
    if detector not in DETECTORS:
        raise ValueError(f"detector must be one of {sorted(DETECTORS)}, not {detector!r}")
    return STAGE_DETECTOR_AKAZE if detector == "AKAZE" else 0


def _descriptor_flag(descriptor: str) -> int:
    if descriptor not in DESCRIPTOR_ARMS:
        raise ValueError(f"descriptor must be one of {sorted(DESCRIPTOR_ARMS)}, not {descriptor!r}")
    return _DESCRIPTOR_STAGE_FLAGS[descriptor]


class R3dmError(RuntimeError):
    pass


class ViewDesc(C.Structure):
    """r3dm_view_desc (include/r3dm.h): one view of an r3dm_set_images batch"""
    _fields_ = [("view_id", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("n", C.c_uint32), ("dim", C.c_uint32),
                ("dtype", C.c_int32), ("desc", C.c_void_p), ("xy", C.c_void_p)]


class Stats(C.Structure):
    _fields_ = [("ms_match_kernels", C.c_double), ("n_match_launches", C.c_uint64),
                ("ms_filter_kernels", C.c_double), ("n_pairs", C.c_uint64), ("n_queries", C.c_uint64),
                ("n_exact_fallback", C.c_uint64), ("algorithmic_flops", C.c_double),
                ("algorithmic_bytes", C.c_double), ("ms_wall_match", C.c_double),
                ("ms_wall_match_post", C.c_double), ("ms_wall_filter", C.c_double), ("ms_liop_kernel", C.c_double),
                ("ms_ann_build", C.c_double), ("ms_ann_search", C.c_double), ("n_ann_built", C.c_uint64),
                ("n_ann_dist", C.c_uint64), ("ms_detect", C.c_double), ("n_integer_mfma", C.c_uint64),
                ("n_split_mfma", C.c_uint64), ("n_views_staged", C.c_uint64),
                ("n_hamming_mfma", C.c_uint64), ("n_detect_images", C.c_uint64), ("n_ann_rows16", C.c_uint64), ("n_ann_rows8", C.c_uint64), ("n_ann_dot8", C.c_uint64),
                ("ms_detect_kernels", C.c_double), ("detect_algorithmic_bytes", C.c_double),
                ("ms_liop_wall", C.c_double), ("ms_feature_files", C.c_double),
                ("n_hnsw_launches", C.c_uint64), ("n_hnsw_retries", C.c_uint64), ("n_counts_mfma", C.c_uint64),
                ("detect_compulsory_bytes", C.c_double), ("n_filter_workgroups", C.c_uint64), ("n_filter_coop_pairs", C.c_uint64),
                ("n_knn_integer_tiles", C.c_uint64), ("n_knn_split_tiles", C.c_uint64),
                ("n_mutual_checked", C.c_uint64), ("n_mutual_dropped", C.c_uint64), ("n_knn_hamming_tiles", C.c_uint64)]


class KGraphHammingStats(C.Structure):
    """r3dm_kgraph_hamming_stats: what the packed-row kernels of the graph matcher did since the context was created"""
    _fields_ = [("n_index_builds", C.c_uint64), ("n_search_launches", C.c_uint64)]


class PreselectStats(C.Structure):
    """r3dm_preselect_stats: the gate of the last match call (preemptive matching on) or preselect_pairs call"""
    _fields_ = [("ms_kernels", C.c_double), ("ms_wall", C.c_double), ("n_pairs", C.c_uint64), ("n_kept", C.c_uint64),
                ("n_heads_built", C.c_uint64), ("n_views_without_priority", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class BudgetStats(C.Structure):
    """r3dm_budget_stats: the match budget's share of the last collection call (the switch on) or budget_rows call"""
    _fields_ = [("ms_select", C.c_double), ("ms_gather", C.c_double), ("ms_remap", C.c_double), ("ms_wall", C.c_double),
                ("n_views_budgeted", C.c_uint64), ("n_views_whole", C.c_uint64), ("n_subviews_built", C.c_uint64),
                ("n_rows_selected", C.c_uint64), ("n_matches_remapped", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class VocabStats(C.Structure):
    """r3dm_vocab_stats: the last propose_pairs / view_signatures call on a vocabulary"""
    _fields_ = [("ms_quantise", C.c_double), ("ms_histogram", C.c_double), ("ms_score", C.c_double), ("ms_select", C.c_double),
                ("n_rows_quantised", C.c_uint64), ("n_signatures_built", C.c_uint64), ("n_signatures_cached", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class VocabTrainStats(C.Structure):
    """r3dm_vocab_train_stats: the r3dm_vocab_train call that made a vocabulary"""
    _fields_ = [("n_updates", C.c_uint32), ("converged", C.c_uint32), ("n_moved", C.c_uint64), ("n_empty", C.c_uint64), ("max_members", C.c_uint64),
                ("n_rows_assigned", C.c_uint64), ("ms_assign", C.c_double), ("ms_sort", C.c_double), ("ms_update", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


VOCAB_WEIGHT_COUNTS, VOCAB_WEIGHT_IDF = 0, 1


class Vocab:
    """r3dm_vocab (include/r3dm.h, "Pair proposal"): n_words rows of one type and length, and the signatures of the views counted
    against them.  Made by Context.vocab_sample / vocab_from_rows; close() releases it."""

    def __init__(self, L, handle):
        self._L, self._h = L, handle
        nw, dim, dt = C.c_uint32(0), C.c_uint32(0), C.c_int32(0)
        L.r3dm_vocab_info(handle, C.byref(nw), C.byref(dim), C.byref(dt))
        self.n_words, self.dim, self.dtype = int(nw.value), int(dim.value), int(dt.value)

    def words(self) -> np.ndarray:
        """r3dm_vocab_words: the codebook, [n_words, dim] float32 (F32) or uint8 (U8 / BIN)"""
        out = np.zeros((self.n_words, self.dim), np.float32 if self.dtype == F32 else np.uint8)
        rc = self._L.r3dm_vocab_words(self._h, out.ctypes.data)
        if rc != 0:
            raise R3dmError(f"r3dm_vocab_words -> {rc}")
        return out

    def set_weighting(self, mode: int):
        """r3dm_vocab_set_weighting: VOCAB_WEIGHT_COUNTS (default) or VOCAB_WEIGHT_IDF for the propose_pairs calls on this vocabulary"""
        rc = self._L.r3dm_vocab_set_weighting(self._h, int(mode))
        if rc != 0:
            raise R3dmError(f"r3dm_vocab_set_weighting -> {rc}")

    def weights(self) -> np.ndarray:
        """r3dm_vocab_weights: q[w] of the last propose_pairs call, [n_words] uint32 (all 1 under COUNTS)"""
        out = np.zeros(self.n_words, np.uint32)
        rc = self._L.r3dm_vocab_weights(self._h, out.ctypes.data)
        if rc != 0:
            raise R3dmError(f"r3dm_vocab_weights -> {rc}")
        return out

    def close(self):
        if getattr(self, "_h", None):
            self._L.r3dm_vocab_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GuidedStats(C.Structure):
    """r3dm_guided_stats: the last guided-matching step of a context"""
    _fields_ = [("ms_kernels", C.c_double), ("ms_wall", C.c_double), ("n_pairs", C.c_uint64), ("n_queries", C.c_uint64),
                ("n_candidates", C.c_uint64), ("n_matches", C.c_uint64), ("n_desc_chunks", C.c_uint64)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["candidates_per_query"] = self.n_candidates / self.n_queries if self.n_queries else 0.0
        return d


class TracksStats(C.Structure):
    """r3dm_tracks_stats"""
    _fields_ = [(n, C.c_uint64) for n in ("n_matches", "n_nodes", "n_components", "n_conflicting", "n_short", "n_tracks", "n_observations",
                                          "n_matches_kept")] + \
               [("longest", C.c_uint32), ("largest_component", C.c_uint32), ("ms_kernels", C.c_double), ("ms_wall", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class FeaturesTotals(C.Structure):
    """r3dm_features_totals: the features work of one context since its creation"""
    _fields_ = [("n_images", C.c_uint64), ("n_passes", C.c_uint64), ("n_keypoints", C.c_uint64), ("n_regrows", C.c_uint64),
                ("ms_detect_kernels", C.c_double), ("detect_algorithmic_bytes", C.c_double), ("ms_liop_kernels", C.c_double),
                ("ms_wall", C.c_double), ("ms_files", C.c_double)]


class ViewImage(C.Structure):
    """r3dm_view_image (include/r3d_compute_matches.hpp)"""
    _fields_ = [("id", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("basename", C.c_char_p),
                ("bgr8", C.c_void_p), ("gray", C.c_void_p), ("focal_px", C.c_double), ("ppx", C.c_double), ("ppy", C.c_double)]


class StageReport(C.Structure):
    """r3dm_stage_report: wall time of the phases of R3DComputeMatches::computeMatches (ms), kernel times, counts"""
    _fields_ = [(k, C.c_double) for k in ("ms_features", "ms_load", "ms_match", "ms_filter_F", "ms_filter_E", "ms_filter_H", "ms_files", "ms_total",
                                          "ms_match_kernels", "ms_F_kernels", "ms_E_kernels", "ms_H_kernels", "ms_filters_wall", "ms_match_post")] + \
               [(k, C.c_uint64) for k in ("images_extracted", "n_keypoints", "n_putative_pairs", "n_putative_matches", "n_F_pairs", "n_F_matches",
                                          "n_E_pairs", "n_E_matches", "n_H_pairs", "n_H_matches", "match_was_exhaustive")] + [("features", FeaturesTotals)] + \
               [("descriptor_arm", C.c_uint64)]          # DESCRIPTOR_ARMS value: what the features stage of the call describes keypoints with

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k != "features"}
        d["features"] = {k: getattr(self.features, k) for k, _ in FeaturesTotals._fields_}
        return d


def _stage_views(views, keep):
    arr = (ViewImage * max(len(views), 1))()
    for k, v in enumerate(views):
        def ptr(a, dt):
            if a is None:
                return None
            if not hasattr(a, "data_ptr"):
                a = np.ascontiguousarray(a, dt)
            keep.append(a)
            return a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data
        arr[k] = ViewImage(int(v["id"]), int(v["width"]), int(v["height"]), v["basename"].encode(), ptr(v.get("bgr"), np.uint8),
                           ptr(v.get("gray"), np.float32), float(v.get("focal_px", -1.0)), float(v.get("ppx", 0.0)), float(v.get("ppy", 0.0)))
    return arr


_STAGE_ARGS = [C.c_char_p, C.c_void_p, C.c_uint32, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_int, C.c_int,
               C.c_uint32, C.c_void_p, C.c_char_p, C.c_size_t]


class Stage:
    """r3dm_stage_*: the R3DComputeMatches facade kept alive between calls (contexts, detector work buffers and page-locked memory
    are allocated once), as a long-lived host process would keep it."""

    def __init__(self, device_ids):
        L = load_library()
        L.r3dm_stage_create.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
        L.r3dm_stage_run.argtypes = [C.c_void_p] + _STAGE_ARGS
        L.r3dm_stage_destroy.argtypes = [C.c_void_p]
        L.r3dm_stage_destroy.restype = None
        ids = (C.c_int * len(device_ids))(*device_ids)
        h = C.c_void_p()
        rc = L.r3dm_stage_create(ids, len(device_ids), C.byref(h))
        if rc != 0:
            raise R3dmError(f"r3dm_stage_create({list(device_ids)}) -> {rc} (no gfx950 GPU visible? there is no CPU fallback)")
        self._h, self._L = h.value, L

    def run(self, matches_dir: str, views, threshold: float = 0.001, dist_ratio: float = 0.6, matching_algorithm: int = 9, compute_F: bool = True,
            compute_E: bool = True, compute_H: bool = True, seed: int = 5489, batches_in_flight: int = 3, images_per_batch: int = 8,
            arms_as_requested: bool = False, split_mfma: bool = False, integer_mfma: bool = False, f32_tiles: bool = False, background_nice: bool = False,
            guided: bool = False, detector: str = "Fast-AKAZE", mutual: bool = False, preemptive: bool = False, descriptor: str = "LIOP", proposal: bool = False,
            symmetric_ratio: bool = False, budget: bool = False) -> StageReport:
        """guided: bGuided_matching = true for the three filters (R3DM_STAGE_GUIDED_MATCHING); detector: "Fast-AKAZE" or "AKAZE"
        (R3DM_STAGE_DETECTOR_AKAZE, the GUI's keypointDetectorType 0); mutual: mutual nearest-neighbour matching (R3DM_STAGE_MUTUAL_MATCHING); preemptive: preemptive matching at 128 / 4
        (R3DM_STAGE_PREEMPTIVE_MATCHING); descriptor: "LIOP", "MLDB" (R3DM_STAGE_DESCRIPTOR_MLDB: binary regions, 61 bytes) or "MSURF"
        (R3DM_STAGE_DESCRIPTOR_MSURF: M-SURF-64, 64 floats); proposal: the matcher gets the pairs r3dm_propose_pairs proposes
        (R3DM_STAGE_PAIR_PROPOSAL); symmetric_ratio: the symmetric ratio test (R3DM_STAGE_SYMMETRIC_RATIO); budget: the match budget at 8,192
        rows per view (R3DM_STAGE_MATCH_BUDGET)"""
        dflag = _detector_flag(detector) | _descriptor_flag(descriptor)
        keep = []
        arr = _stage_views(views, keep)
        rep = StageReport(); err = C.create_string_buffer(1024)
        rc = self._L.r3dm_stage_run(self._h, matches_dir.encode(), arr, len(views), threshold, dist_ratio, matching_algorithm, int(compute_F),
                                    int(compute_E), int(compute_H), seed, batches_in_flight, images_per_batch,
                                    (1 if arms_as_requested else 0) | (2 if split_mfma else 0) | (4 if integer_mfma else 0) | (8 if f32_tiles else 0) | (16 if background_nice else 0)
                                    | (STAGE_GUIDED_MATCHING if guided else 0) | (STAGE_MUTUAL_MATCHING if mutual else 0) | (STAGE_PREEMPTIVE_MATCHING if preemptive else 0) | (STAGE_PAIR_PROPOSAL if proposal else 0) | (STAGE_SYMMETRIC_RATIO if symmetric_ratio else 0) | (STAGE_MATCH_BUDGET if budget else 0) | dflag, C.byref(rep), err, 1024)
        if rc != 0:
            raise R3dmError(f"r3dm_stage_run -> {rc}: {err.value.decode()}")
        return rep

    def close(self):
        if getattr(self, "_h", None):
            self._L.r3dm_stage_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def compute_matches_stage(device_ids, matches_dir: str, views, threshold: float = 0.001, dist_ratio: float = 0.6,
                          matching_algorithm: int = 9, compute_F: bool = True, compute_E: bool = True, compute_H: bool = True,
                          seed: int = 5489, batches_in_flight: int = 3, images_per_batch: int = 8, arms_as_requested: bool = False,
                          split_mfma: bool = False, integer_mfma: bool = False, f32_tiles: bool = False, background_nice: bool = False,
                          guided: bool = False, detector: str = "Fast-AKAZE", mutual: bool = False, preemptive: bool = False, descriptor: str = "LIOP", proposal: bool = False,
            symmetric_ratio: bool = False, budget: bool = False) -> StageReport:
    """R3DComputeMatches::computeMatches from pixels (r3dm_compute_matches_stage): features stage for the views whose .feat/.desc
    are missing, matching, F / E / H filters, match files.  views: dicts with id, width, height, basename and optionally
    gray ([h, w] float32) or bgr ([h, w, 3] uint8) -- numpy or torch (host or device) -- and focal_px / ppx / ppy.
    detector: "Fast-AKAZE" (default) or "AKAZE" (R3DM_STAGE_DETECTOR_AKAZE); mutual: R3DM_STAGE_MUTUAL_MATCHING; preemptive:
    R3DM_STAGE_PREEMPTIVE_MATCHING (head_rows 128, min_matches 4); descriptor: "LIOP" (default), "MLDB" (R3DM_STAGE_DESCRIPTOR_MLDB:
    the features stage writes MLDB-486 rows, the matcher runs its binary rules) or "MSURF" (R3DM_STAGE_DESCRIPTOR_MSURF: M-SURF-64
    rows of 64 floats, matched by the float rules as LIOP is); proposal: R3DM_STAGE_PAIR_PROPOSAL (the matcher gets the pairs
    r3dm_propose_pairs proposes from a vocabulary sampled from the stage's views: 16,384 words, half the collection's rows when that is
    less, top_k 20); symmetric_ratio: R3DM_STAGE_SYMMETRIC_RATIO (a match must also pass the 2-NN + ratio rule with the views swapped); budget:
    R3DM_STAGE_MATCH_BUDGET (only each view's 8,192 largest-scale features are matched)."""
    dflag = _detector_flag(detector) | _descriptor_flag(descriptor)
    L = load_library()
    keep = []
    arr = _stage_views(views, keep)
    ids = (C.c_int * len(device_ids))(*device_ids)
    rep = StageReport(); err = C.create_string_buffer(1024)
    L.r3dm_compute_matches_stage.argtypes = [C.c_void_p, C.c_int] + _STAGE_ARGS
    rc = L.r3dm_compute_matches_stage(ids, len(device_ids), matches_dir.encode(), arr, len(views), threshold, dist_ratio, matching_algorithm,
                                      int(compute_F), int(compute_E), int(compute_H), seed, batches_in_flight, images_per_batch,
                                      (1 if arms_as_requested else 0) | (2 if split_mfma else 0) | (4 if integer_mfma else 0) | (8 if f32_tiles else 0) | (16 if background_nice else 0)
                                      | (STAGE_GUIDED_MATCHING if guided else 0) | (STAGE_MUTUAL_MATCHING if mutual else 0) | (STAGE_PREEMPTIVE_MATCHING if preemptive else 0) | (STAGE_PAIR_PROPOSAL if proposal else 0) | (STAGE_SYMMETRIC_RATIO if symmetric_ratio else 0) | (STAGE_MATCH_BUDGET if budget else 0) | dflag, C.byref(rep), err, 1024)
    if rc != 0:
        raise R3dmError(f"r3dm_compute_matches_stage -> {rc}: {err.value.decode()}")
    return rep


class _DirView(C.Structure):
    """r3dm_view (include/r3d_compute_matches.hpp)"""
    _fields_ = [("id", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("basename", C.c_char_p)]


def compute_matches_dir(device_id: int, matches_dir: str, views, dtype: int = 0, dim: int = 144, dist_ratio: float = 0.6,
                        compute_F: bool = True, seed: int = 5489, f32_tiles: bool = False, mutual: bool = False, preemptive: bool = False,
                        proposal: bool = False, symmetric_ratio: bool = False, budget: bool = False, proposal_trained: bool = False):
    """R3DComputeMatches::computeMatches over a directory that holds every view's .feat / .desc (r3dm_compute_matches_dir_flags):
    exhaustive matching, the F filter when asked, matches.putative.txt / matches.f.txt.  views: dicts with id, width, height,
    basename; dtype: F32 / U8 / BIN; mutual: R3DM_STAGE_MUTUAL_MATCHING; preemptive: R3DM_STAGE_PREEMPTIVE_MATCHING (the .feat scale column is
    every view's priority); proposal: R3DM_STAGE_PAIR_PROPOSAL; proposal_trained: R3DM_STAGE_PROPOSAL_TRAINED (with proposal: the
    vocabulary is trained for at most 10 updates and the scores are idf-weighted); symmetric_ratio: R3DM_STAGE_SYMMETRIC_RATIO; budget: R3DM_STAGE_MATCH_BUDGET (8,192 rows
    per view, priority = the .feat scale column).  -> (putative pairs, geometric pairs)"""
    L = load_library()
    arr = (_DirView * len(views))(*[_DirView(int(v["id"]), int(v["width"]), int(v["height"]), str(v["basename"]).encode()) for v in views])
    npp, ngp = C.c_uint64(0), C.c_uint64(0)
    err = C.create_string_buffer(1024)
    L.r3dm_compute_matches_dir_flags.argtypes = [C.c_int, C.c_char_p, C.c_void_p, C.c_uint32, C.c_int, C.c_uint32, C.c_float, C.c_int, C.c_uint64,
                                                 C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_char_p, C.c_size_t]
    rc = L.r3dm_compute_matches_dir_flags(device_id, matches_dir.encode(), arr, len(views), dtype, dim, dist_ratio, int(compute_F), seed,
                                          (8 if f32_tiles else 0) | (STAGE_MUTUAL_MATCHING if mutual else 0) | (STAGE_PREEMPTIVE_MATCHING if preemptive else 0)
                                          | (STAGE_PAIR_PROPOSAL if proposal else 0) | (STAGE_SYMMETRIC_RATIO if symmetric_ratio else 0) | (STAGE_MATCH_BUDGET if budget else 0)
                                          | (STAGE_PROPOSAL_TRAINED if proposal_trained else 0), C.byref(npp), C.byref(ngp), err, 1024)
    if rc != 0:
        raise R3dmError(f"r3dm_compute_matches_dir_flags -> {rc}: {err.value.decode()}")
    return int(npp.value), int(ngp.value)


class KGraphParams(C.Structure):
    """r3dm_kgraph_params: index_K forward neighbours per row, search_P start rows, search_S neighbours per step."""
    _fields_ = [("index_K", C.c_uint32), ("search_P", C.c_uint32), ("search_S", C.c_uint32), ("reserved", C.c_uint32),
                ("seed", C.c_uint64)]

    @staticmethod
    def preset(which) -> "KGraphParams":
        """which: 0 / "fast", 1 / "medium", 2 / "precise", anything else the reference's default block"""
        code = {"fast": 0, "medium": 1, "precise": 2}.get(which, which if isinstance(which, int) else 3)
        kp = KGraphParams()
        if load_library().r3dm_kgraph_preset(int(code), C.byref(kp)) != 0:
            raise R3dmError("r3dm_kgraph_preset failed")
        return kp


class HnswParams(C.Structure):
    """r3dm_hnsw_params: M links per row (2M on layer 0), ef_construction (unused by the batch build), ef search beam, seed of the level draw"""
    _fields_ = [("M", C.c_uint32), ("ef_construction", C.c_uint32), ("ef", C.c_uint32), ("seed", C.c_uint32)]

    @staticmethod
    def preset(which) -> "HnswParams":
        """which: 0 / "fast", 1 / "medium", 2 / "precise" (matchingAlgorithm 6 / 7 / 8 of the reference)"""
        code = {"fast": 0, "medium": 1, "precise": 2}.get(which, which if isinstance(which, int) else 2)
        hp = HnswParams()
        if load_library().r3dm_hnsw_preset(int(code), C.byref(hp)) != 0:
            raise R3dmError("r3dm_hnsw_preset failed")
        return hp


class MrptParams(C.Structure):
    """r3dm_mrpt_params: n_trees, depth (clamped per view), votes, density (<= 0: 1 / sqrt(dim)), seed of the random vectors"""
    _fields_ = [("n_trees", C.c_uint32), ("depth", C.c_uint32), ("votes", C.c_uint32), ("density", C.c_float), ("seed", C.c_uint64)]

    @staticmethod
    def preset() -> "MrptParams":
        mp = MrptParams()
        if load_library().r3dm_mrpt_preset(C.byref(mp)) != 0:
            raise R3dmError("r3dm_mrpt_preset failed")
        return mp


class HnswArrays(C.Structure):
    """r3dm_hnsw_arrays: an HNSW index in hnswlib's own shape"""
    _fields_ = [("M", C.c_uint32), ("links0", C.c_void_p), ("up_off", C.c_void_p), ("up_links", C.c_void_p), ("up_rows", C.c_uint32),
                ("enterpoint", C.c_int32), ("maxlevel", C.c_int32)]


class PairReport(C.Structure):
    _fields_ = [("threshold_px", C.c_double), ("nfa", C.c_double), ("iterations", C.c_uint32),
                ("models", C.c_uint32), ("inliers", C.c_uint32), ("reserved", C.c_uint32)]


_lib = None
DEV_LIB_PATH = os.path.join(_HERE, "libr3dm_dev.so")


def use_developer_library():
    """tools/ and the fallback-path tests: load the developer build (build.sh dev: -DR3DM_DEVTOOLS, the A/B kernel variants,
    traces and test hooks that read R3DM_* environment variables) instead of the product library.  Must be called before the
    first load_library(); the product library itself never reads the environment."""
    global LIB_PATH
    if _lib is not None:
        raise R3dmError("the library is already loaded")
    LIB_PATH = DEV_LIB_PATH


def use_library(path: str):
    """load a specific build of the library (bisecting tools); before the first load_library()"""
    global LIB_PATH
    if _lib is not None:
        raise R3dmError("the library is already loaded")
    LIB_PATH = path


def load_library():
    """dlopen libr3dm.so and declare prototypes.  Raises if the extension was not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise R3dmError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                        "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    L = C.CDLL(LIB_PATH)
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    L.r3dm_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.r3dm_destroy.argtypes = [vp]; L.r3dm_destroy.restype = None
    L.r3dm_last_error.argtypes = [vp]; L.r3dm_last_error.restype = C.c_char_p
    L.r3dm_device_info.argtypes = [vp, C.c_char_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(u64)]
    L.r3dm_set_image.argtypes = [vp, u32, u32, u32, vp, u32, u32, C.c_int, vp]
    L.r3dm_set_images.argtypes = [vp, vp, u32]
    L.r3dm_images_wait.argtypes = [vp]
    L.r3dm_view_info.argtypes = [vp, u32, vp, vp, vp, vp]
    L.r3dm_memory_info.argtypes = [vp, vp, vp, vp]
    L.r3dm_clear_images.argtypes = [vp]
    L.r3dm_trim.argtypes = [vp]
    L.r3dm_set_integer_mfma.argtypes = [vp, C.c_int]
    L.r3dm_set_split_mfma.argtypes = [vp, C.c_int]
    L.r3dm_set_prefix_pruning.argtypes = [vp, C.c_int]
    L.r3dm_get_prefix_pruning_counts.argtypes = [vp, C.POINTER(u64)]
    L.r3dm_multi_set_prefix_pruning.argtypes = [vp, C.c_int]
    L.r3dm_multi_get_prefix_pruning_counts.argtypes = [vp, C.POINTER(u64)]
    L.r3dm_get_pair_filter_counts.argtypes = [vp, C.POINTER(u64)]
    L.r3dm_multi_get_pair_filter_counts.argtypes = [vp, C.POINTER(u64)]
    L.r3dm_set_half_filter.argtypes = [vp, C.c_int]
    L.r3dm_get_half_filter_counts.argtypes = [vp, C.POINTER(u64)]
    L.r3dm_multi_set_half_filter.argtypes = [vp, C.c_int]
    L.r3dm_multi_get_half_filter_counts.argtypes = [vp, C.POINTER(u64)]
    L.r3dm_get_level2_skip_counts.argtypes = [vp, C.POINTER(u64)]
    L.r3dm_multi_get_level2_skip_counts.argtypes = [vp, C.POINTER(u64)]
    L.r3dm_set_min_tile_test.argtypes = [vp, C.c_int]
    L.r3dm_get_min_tile_test_counts.argtypes = [vp, C.POINTER(u64)]
    L.r3dm_multi_set_min_tile_test.argtypes = [vp, C.c_int]
    L.r3dm_multi_get_min_tile_test_counts.argtypes = [vp, C.POINTER(u64)]
    L.r3dm_set_half_prefix.argtypes = [vp, C.c_int]
    L.r3dm_get_half_prefix_counts.argtypes = [vp, C.POINTER(u64)]
    L.r3dm_multi_set_half_prefix.argtypes = [vp, C.c_int]
    L.r3dm_multi_get_half_prefix_counts.argtypes = [vp, C.POINTER(u64)]
    L.r3dm_set_hamming_mfma.argtypes = [vp, C.c_int]
    L.r3dm_set_knn_narrow_tiles.argtypes = [vp, C.c_int]
    L.r3dm_set_knn_hamming_tiles.argtypes = [vp, C.c_int]
    L.r3dm_set_mutual_matching.argtypes = [vp, C.c_int]
    L.r3dm_multi_set_mutual_matching.argtypes = [vp, C.c_int]
    L.r3dm_set_symmetric_ratio.argtypes = [vp, C.c_int]
    L.r3dm_multi_set_symmetric_ratio.argtypes = [vp, C.c_int]
    L.r3dm_symmetric_ratio_report.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.r3dm_set_kgraph_hamming.argtypes = [vp, C.c_int]
    L.r3dm_multi_set_kgraph_hamming.argtypes = [vp, C.c_int]
    L.r3dm_kgraph_hamming_report.argtypes = [vp, vp]
    L.r3dm_kgraph_knn2_bits.argtypes = [vp, vp, u32, vp, u32, u32, vp, u32, u32, vp, vp]
    L.r3dm_kgraph_knn_bits.argtypes = [vp, vp, u32, vp, u32, u32, vp, u32, u32, u32, vp, vp]
    L.r3dm_set_view_priority.argtypes = [vp, u32, vp, u32]
    L.r3dm_multi_set_view_priority.argtypes = [vp, u32, vp, u32]
    L.r3dm_preselect_pairs.argtypes = [vp, vp, C.c_uint64, u32, C.c_float, C.c_int, vp]
    L.r3dm_set_preemptive_matching.argtypes = [vp, C.c_int, u32, u32]
    L.r3dm_multi_set_preemptive_matching.argtypes = [vp, C.c_int, u32, u32]
    L.r3dm_preselect_report.argtypes = [vp, vp]
    L.r3dm_set_match_budget.argtypes = [vp, C.c_int, u32]
    L.r3dm_multi_set_match_budget.argtypes = [vp, C.c_int, u32]
    L.r3dm_budget_rows.argtypes = [vp, u32, u32, vp, vp]
    L.r3dm_budget_report.argtypes = [vp, vp]
    L.r3dm_vocab_sample.argtypes = [vp, vp, u32, u32, C.POINTER(vp)]
    L.r3dm_vocab_from_rows.argtypes = [vp, vp, u32, u32, C.c_int, C.POINTER(vp)]
    L.r3dm_vocab_info.argtypes = [vp, vp, vp, vp]
    L.r3dm_vocab_words.argtypes = [vp, vp]
    L.r3dm_vocab_free.argtypes = [vp]; L.r3dm_vocab_free.restype = None
    L.r3dm_view_signatures.argtypes = [vp, vp, vp, u32, vp]
    L.r3dm_propose_pairs.argtypes = [vp, vp, vp, u32, u32, vp, C.c_uint64, C.POINTER(C.c_uint64), vp]
    L.r3dm_vocab_report.argtypes = [vp, vp]
    L.r3dm_vocab_train.argtypes = [vp, vp, vp, u32, u32, C.POINTER(vp)]
    L.r3dm_vocab_train_report.argtypes = [vp, vp]
    L.r3dm_vocab_set_weighting.argtypes = [vp, C.c_int]
    L.r3dm_vocab_weights.argtypes = [vp, vp]
    L.r3dm_index_create.argtypes = [vp, vp, u32, u32, C.c_int, C.POINTER(vp)]
    L.r3dm_index_knn2.argtypes = [vp, vp, vp, u32, vp, vp]
    L.r3dm_index_destroy.argtypes = [vp]; L.r3dm_index_destroy.restype = None
    L.r3dm_match_pairs.argtypes = [vp, vp, u64, C.c_float, C.c_int, C.POINTER(vp)]
    L.r3dm_filter_F.argtypes = [vp, vp, C.c_double, u32, u64, C.c_int, C.POINTER(vp), vp]
    L.r3dm_filter_H.argtypes = [vp, vp, C.c_double, u32, u64, C.POINTER(vp), vp]
    L.r3dm_filter_E.argtypes = [vp, vp, C.c_double, u32, u64, u32, C.c_float, C.POINTER(vp), vp]
    L.r3dm_filter_FEH.argtypes = [vp, vp, C.c_double, u32, u64, C.c_int, u32, C.c_float, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), vp, vp]
    L.r3dm_set_intrinsics.argtypes = [vp, u32, vp]
    L.r3dm_guided_match.argtypes = [vp, vp, C.c_int, vp, vp, C.c_double, C.POINTER(vp)]
    L.r3dm_set_guided_matching.argtypes = [vp, C.c_int, C.c_double, C.c_double, C.c_double]
    L.r3dm_guided_report.argtypes = [vp, vp]
    L.r3dm_multi_set_guided_matching.argtypes = [vp, C.c_int, C.c_double, C.c_double, C.c_double]
    L.r3dm_set_keypoint_detector.argtypes = [vp, C.c_int]
    L.r3dm_multi_set_keypoint_detector.argtypes = [vp, C.c_int]
    L.r3dm_set_descriptor_arm.argtypes = [vp, C.c_int]
    L.r3dm_multi_set_descriptor_arm.argtypes = [vp, C.c_int]
    L.r3dm_akaze_classic_components.argtypes = [vp, vp]
    L.r3dm_liop_describe_patches.argtypes = [vp, vp, u32, u32, vp, C.POINTER(u32)]
    L.r3dm_extract_liop.argtypes = [vp, vp, u32, u32, vp, u32, C.c_float, vp, vp]
    L.r3dm_knn2.argtypes = [vp, vp, u32, vp, u32, u32, C.c_int, vp, vp]
    L.r3dm_knn.argtypes = [vp, vp, u32, vp, u32, u32, C.c_int, u32, vp, vp]
    L.r3dm_index_knn.argtypes = [vp, vp, vp, u32, u32, vp, vp]
    L.r3dm_detect_akaze.argtypes = [vp, vp, u32, u32, C.c_float, vp, vp, u32, C.POINTER(u32)]
    L.r3dm_detect_akaze_mldb.argtypes = [vp, vp, u32, u32, C.c_float, vp, vp, u32, C.POINTER(u32)]
    L.r3dm_gray_from_bgr8.argtypes = [vp, vp, u32, u32, vp]
    L.r3dm_extract_features_to_files.argtypes = [vp, vp, u32, u32, C.c_float, C.c_char_p, C.c_char_p, C.POINTER(u32)]
    L.r3dm_multi_extract_features.argtypes = [vp, u32, vp, vp, vp, C.c_float, vp, vp, vp, vp, C.c_char_p, C.c_size_t]
    L.r3dm_multi_extract_features_ex.argtypes = [vp, u32, vp, vp, vp, vp, C.c_float, vp, vp, vp, vp, u32, C.c_char_p, C.c_size_t]
    L.r3dm_get_features_totals.argtypes = [vp, vp]
    L.r3dm_detect_akaze_batch.argtypes = [vp, u32, vp, u32, u32, C.c_float, vp, vp, u32, vp]
    L.r3dm_detect_akaze_mldb_batch.argtypes = [vp, u32, vp, u32, u32, C.c_float, vp, vp, u32, vp]
    L.r3dm_detect_akaze_msurf.argtypes = [vp, vp, u32, u32, C.c_float, vp, vp, u32, C.POINTER(u32)]
    L.r3dm_detect_akaze_msurf_batch.argtypes = [vp, u32, vp, u32, u32, C.c_float, vp, vp, u32, vp]
    L.r3dm_detect_akaze_classic.argtypes = [vp, vp, u32, u32, C.c_float, vp, vp, u32, C.POINTER(u32)]
    L.r3dm_detect_akaze_classic_batch.argtypes = [vp, u32, vp, u32, u32, C.c_float, vp, vp, u32, vp]
    L.r3dm_extract_features_batch.argtypes = [vp, u32, vp, vp, u32, u32, C.c_float, vp, vp, vp]
    L.r3dm_kgraph_preset.argtypes = [C.c_int, vp]
    L.r3dm_ann_params_for_algorithm.argtypes = [C.c_int, vp]
    L.r3dm_match_pairs_kgraph.argtypes = [vp, vp, u64, C.c_float, vp, C.POINTER(vp)]
    L.r3dm_kgraph_knn2.argtypes = [vp, vp, u32, vp, u32, u32, vp, u32, u32, vp, vp]
    L.r3dm_kgraph_index.argtypes = [vp, u32, u32, vp, vp]
    L.r3dm_hnsw_preset.argtypes = [C.c_int, vp]
    L.r3dm_mrpt_preset.argtypes = [vp]
    L.r3dm_match_pairs_mrpt.argtypes = [vp, vp, u64, C.c_float, vp, C.POINTER(vp)]
    L.r3dm_mrpt_knn2.argtypes = [vp, vp, C.c_uint32, vp, C.c_uint32, C.c_uint32, vp, vp, vp]
    L.r3dm_mrpt_index.argtypes = [vp, C.c_uint32, vp, vp, vp, vp, vp, vp]
    L.r3dm_multi_match_pairs_mrpt.argtypes = [vp, vp, u64, C.c_float, vp, C.POINTER(vp)]
    L.r3dm_match_pairs_hnsw.argtypes = [vp, vp, u64, C.c_float, vp, C.POINTER(vp)]
    L.r3dm_hnsw_knn2.argtypes = [vp, vp, u32, vp, u32, u32, vp, vp, vp]
    L.r3dm_hnsw_knn2_on_index.argtypes = [vp, vp, u32, u32, vp, vp, u32, u32, vp, vp]
    L.r3dm_hnsw_index.argtypes = [vp, u32, vp, vp, vp, vp, u32, vp, vp, vp]
    L.r3dm_drop_indices.argtypes = [vp]
    L.r3dm_kgraph_knn.argtypes = [vp, vp, u32, vp, u32, u32, vp, u32, u32, u32, vp, vp]
    L.r3dm_hnsw_knn.argtypes = [vp, vp, u32, vp, u32, u32, vp, u32, vp, vp]
    L.r3dm_hnsw_knn_on_index.argtypes = [vp, vp, u32, u32, vp, vp, u32, u32, u32, vp, vp]
    L.r3dm_mrpt_knn.argtypes = [vp, vp, u32, vp, u32, u32, vp, u32, vp, vp]
    L.r3dm_index_kgraph_knn.argtypes = [vp, vp, vp, vp, u32, u32, u32, u32, vp, vp]
    L.r3dm_index_hnsw_knn.argtypes = [vp, vp, vp, vp, u32, u32, vp, vp]
    L.r3dm_index_mrpt_knn.argtypes = [vp, vp, vp, vp, u32, u32, vp, vp]
    L.r3dm_graph_num_pairs.argtypes = [vp]; L.r3dm_graph_num_pairs.restype = u64
    L.r3dm_graph_num_matches.argtypes = [vp]; L.r3dm_graph_num_matches.restype = u64
    L.r3dm_graph_pairs.argtypes = [vp]; L.r3dm_graph_pairs.restype = vp
    L.r3dm_graph_offsets.argtypes = [vp]; L.r3dm_graph_offsets.restype = vp
    L.r3dm_graph_matches.argtypes = [vp]; L.r3dm_graph_matches.restype = vp
    L.r3dm_graph_free.argtypes = [vp]; L.r3dm_graph_free.restype = None
    L.r3dm_graph_from_csr.argtypes = [vp, u64, vp, vp, C.POINTER(vp)]
    L.r3dm_graph_merge.argtypes = [vp, u32, C.POINTER(vp)]
    L.r3dm_comm_unique_id.argtypes = [vp]
    L.r3dm_comm_create.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    L.r3dm_comm_destroy.argtypes = [vp]; L.r3dm_comm_destroy.restype = None
    L.r3dm_comm_rank.argtypes = [vp]; L.r3dm_comm_world.argtypes = [vp]
    L.r3dm_comm_last_error.argtypes = [vp]; L.r3dm_comm_last_error.restype = C.c_char_p
    L.r3dm_allgather_graphs.argtypes = [vp, vp, u32, vp]
    L.r3dm_set_device_graphs.argtypes = [vp, C.c_int]
    L.r3dm_graph_on_device.argtypes = [vp]
    L.r3dm_set_deferred_feature_files.argtypes = [vp, C.c_int]
    L.r3dm_features_files_wait.argtypes = [vp]
    L.r3dm_multi_set_deferred_feature_files.argtypes = [vp, C.c_int]
    L.r3dm_multi_features_files_wait.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.r3dm_comm_last_device_graphs.argtypes = [vp]
    L.r3dm_graphs_pack.argtypes = [vp, u32, C.POINTER(vp), C.POINTER(u64)]
    L.r3dm_words_free.argtypes = [vp]; L.r3dm_words_free.restype = None
    L.r3dm_graphs_unpack_merge.argtypes = [vp, vp, u32, u32, vp]
    L.r3dm_save_matches.argtypes = [vp, C.c_char_p]
    L.r3dm_load_matches.argtypes = [C.c_char_p, C.POINTER(vp)]
    L.r3dm_get_stats.argtypes = [vp, C.POINTER(Stats)]
    L.r3dm_filter_report.argtypes = [vp, vp, u64]
    L.r3dm_multi_create.argtypes = [vp, C.c_int, C.POINTER(vp)]
    L.r3dm_multi_destroy.argtypes = [vp]; L.r3dm_multi_destroy.restype = None
    L.r3dm_multi_num_devices.argtypes = [vp]
    L.r3dm_multi_ctx.argtypes = [vp, C.c_int]; L.r3dm_multi_ctx.restype = vp
    L.r3dm_multi_last_error.argtypes = [vp]; L.r3dm_multi_last_error.restype = C.c_char_p
    L.r3dm_multi_set_image.argtypes = [vp, u32, u32, u32, vp, u32, u32, C.c_int, vp]
    L.r3dm_multi_set_intrinsics.argtypes = [vp, u32, vp]
    L.r3dm_multi_clear_images.argtypes = [vp]
    L.r3dm_multi_set_integer_mfma.argtypes = [vp, C.c_int]
    L.r3dm_multi_match_pairs.argtypes = [vp, vp, u64, C.c_float, C.c_int, C.POINTER(vp)]
    L.r3dm_multi_match_pairs_kgraph.argtypes = [vp, vp, u64, C.c_float, vp, C.POINTER(vp)]
    L.r3dm_multi_match_pairs_hnsw.argtypes = [vp, vp, u64, C.c_float, vp, C.POINTER(vp)]
    L.r3dm_multi_filter_F.argtypes = [vp, vp, C.c_double, u32, u64, C.POINTER(vp), vp]
    L.r3dm_multi_filter_H.argtypes = [vp, vp, C.c_double, u32, u64, C.POINTER(vp), vp]
    L.r3dm_multi_filter_E.argtypes = [vp, vp, C.c_double, u32, u64, u32, C.c_float, C.POINTER(vp), vp]
    L.r3dm_shard_pairs.argtypes = [vp, u64, u32, vp]
    L.r3dm_build_tracks.argtypes = [vp, vp, u32, C.POINTER(vp), vp]
    L.r3dm_tracks_count.argtypes = [vp]; L.r3dm_tracks_count.restype = u64
    L.r3dm_tracks_offsets.argtypes = [vp]; L.r3dm_tracks_offsets.restype = vp
    L.r3dm_tracks_observations.argtypes = [vp]; L.r3dm_tracks_observations.restype = vp
    L.r3dm_tracks_report.argtypes = [vp, C.POINTER(TracksStats)]
    L.r3dm_tracks_phase_ms.argtypes = [vp, vp]
    L.r3dm_tracks_in_pair.argtypes = [vp, u32, u32, vp, u64, C.POINTER(u64)]
    L.r3dm_tracks_free.argtypes = [vp]; L.r3dm_tracks_free.restype = None
    _lib = L
    return L


class DevAcLevel(C.Structure):
    """r3dm_dev_ac_level (developer build, api_akaze_classic.cpp): one level of a classic A-KAZE level table"""
    _fields_ = [("w", C.c_int32), ("h", C.c_int32), ("octave", C.c_int32), ("esigma", C.c_float), ("ratio", C.c_float)]


def bind_dev_akaze_classic_walk(L):
    """the developer build's walk entries (libr3dm_dev.so only, declared in no header), bound when first asked for"""
    if getattr(L, "_r3dm_dev_walk_bound", False):
        return L
    if not hasattr(L, "r3dm_dev_akaze_classic_walk"):
        raise R3dmError("r3dm_dev_akaze_classic_walk exists in the developer build only: use_developer_library() before the first load")
    vp, u32 = C.c_void_p, C.c_uint32
    L.r3dm_dev_akaze_classic_walk_check.argtypes = [vp, u32, u32, u32, u32, vp, vp, C.c_int, u32]
    L.r3dm_dev_akaze_classic_walk.argtypes = [vp, vp, u32, u32, u32, u32, vp, vp, C.c_int, u32, vp, vp, vp]
    L._r3dm_dev_walk_bound = True
    return L


def dev_walk_args(levels, lists):
    """(level array, n_cand [B] uint32, candidates [sum, 4] uint32 words) of the walk entries.  levels: dicts with w, h, octave,
    esigma, ratio; lists: per image (level, row, col, value) tuples -- stored as the library's (x = col, y = row, level, value)"""
    lv = (DevAcLevel * max(len(levels), 1))(*[DevAcLevel(int(e["w"]), int(e["h"]), int(e["octave"]), float(e["esigma"]), float(e["ratio"]))
                                              for e in levels])
    n_cand = np.array([len(l) for l in lists], np.uint32)
    words = np.zeros((int(n_cand.sum()), 4), np.uint32)
    flat = [c for l in lists for c in l]
    if flat:
        words[:, 0] = [c[2] for c in flat]; words[:, 1] = [c[1] for c in flat]; words[:, 2] = [c[0] for c in flat]
        words[:, 3] = np.array([c[3] for c in flat], np.float32).view(np.uint32)
    return lv, n_cand, words


def bind_dev_akaze_classic_head(L):
    """the developer build's classic head entries (libr3dm_dev.so only, declared in no header), bound when first asked for"""
    if getattr(L, "_r3dm_dev_classic_head_bound", False):
        return L
    if not hasattr(L, "r3dm_dev_akaze_classic_head"):
        raise R3dmError("r3dm_dev_akaze_classic_head exists in the developer build only: use_developer_library() before the first load")
    vp, u32 = C.c_void_p, C.c_uint32
    L.r3dm_dev_akaze_classic_levels.argtypes = [u32, u32, vp, vp]
    L.r3dm_dev_akaze_classic_head_check.argtypes = [u32, vp, u32, u32]
    L.r3dm_dev_akaze_classic_head.argtypes = [vp, u32, vp, u32, u32, C.c_float, vp, vp, vp, u32, vp, vp]
    L.r3dm_dev_akaze_classic_extrema_check.argtypes = [u32, u32, u32, u32, vp, vp]
    L.r3dm_dev_akaze_classic_extrema.argtypes = [vp, u32, u32, u32, u32, vp, vp, C.c_float, vp, u32, vp, vp]
    L._r3dm_dev_classic_head_bound = True
    return L


def dev_akaze_classic_levels(L, width: int, height: int):
    """r3dm_dev_akaze_classic_levels (needs no device): the classic arm's level table of an image size, a list of dicts"""
    bind_dev_akaze_classic_head(L)
    lv = (DevAcLevel * 16)()
    n = C.c_uint32(0)
    rc = L.r3dm_dev_akaze_classic_levels(width, height, C.addressof(lv), C.addressof(n))
    if rc != 0:
        raise R3dmError(f"r3dm_dev_akaze_classic_levels -> {rc}")
    return [dict(w=lv[i].w, h=lv[i].h, octave=lv[i].octave, esigma=lv[i].esigma, ratio=lv[i].ratio) for i in range(n.value)]


def dev_classic_bound(levels) -> int:
    """the candidates an image of this level table can hold at most: strict 3 x 3 maxima lie at least two apart on both axes, inside
    rows 1 .. h - 2 and columns 1 .. w - 2"""
    return sum(((e["w"] - 1) // 2) * ((e["h"] - 1) // 2) for e in levels)


def _dev_classic_candidates(counts, n, cand, B):
    """per image (counts [n_levels] uint32, candidates [n, 4]: x, y, level as uint32 words and the value's bits) -> dicts"""
    out = []
    for b in range(B):
        words = cand[b, :int(n[b])].copy()
        out.append(dict(counts=counts[b].copy(), x=words[:, 0], y=words[:, 1], level=words[:, 2], value=words[:, 3].copy().view(np.float32)))
    return out


class DevAkLevel(C.Structure):
    """r3dm_dev_ak_level (developer build, api_akaze.cpp): one level of the Fast arm's level table"""
    _fields_ = [("w", C.c_int32), ("h", C.c_int32), ("border", C.c_int32), ("sigma_size", C.c_int32), ("ratio", C.c_float),
                ("esigma", C.c_float), ("psize", C.c_float)]


def bind_dev_akaze_tail(L):
    """the developer build's Fast-arm tail entries (libr3dm_dev.so only, declared in no header), bound when first asked for"""
    if getattr(L, "_r3dm_dev_tail_bound", False):
        return L
    if not hasattr(L, "r3dm_dev_akaze_tail"):
        raise R3dmError("r3dm_dev_akaze_tail exists in the developer build only: use_developer_library() before the first load")
    vp, u32 = C.c_void_p, C.c_uint32
    L.r3dm_dev_akaze_tail_levels.argtypes = [u32, u32, vp, vp]
    L.r3dm_dev_akaze_tail_check.argtypes = [u32, u32, u32, u32, vp, vp, vp, vp]
    L.r3dm_dev_akaze_tail.argtypes = [vp, u32, u32, u32, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L._r3dm_dev_tail_bound = True
    return L


def dev_akaze_tail_levels(L, width: int, height: int):
    """r3dm_dev_akaze_tail_levels: the Fast arm's level table of a width x height image, as dicts (w, h, border, sigma_size, ratio,
    esigma, psize)"""
    bind_dev_akaze_tail(L)
    lv = (DevAkLevel * 16)(); n = C.c_uint32(0)
    rc = L.r3dm_dev_akaze_tail_levels(width, height, C.addressof(lv), C.addressof(n))
    if rc != 0:
        raise R3dmError(f"r3dm_dev_akaze_tail_levels -> {rc}")
    return [{k: getattr(lv[i], k) for k, _ in DevAkLevel._fields_} for i in range(n.value)]


MSURF_ITEM = np.dtype([("level", np.uint32), ("xf", np.float32), ("yf", np.float32), ("co", np.float32), ("si", np.float32),
                       ("scale", np.int32)])          # AkMsurfItem (r3dm_internal.hpp): a keypoint in level coordinates, cos / sin of its angle


def bind_dev_akaze_msurf(L):
    """the developer build's M-SURF-64 kernel entries (libr3dm_dev.so only, declared in no header), bound when first asked for"""
    if getattr(L, "_r3dm_dev_msurf_bound", False):
        return L
    if not hasattr(L, "r3dm_dev_akaze_msurf"):
        raise R3dmError("r3dm_dev_akaze_msurf exists in the developer build only: use_developer_library() before the first load")
    vp, u32 = C.c_void_p, C.c_uint32
    L.r3dm_dev_akaze_msurf_levels.argtypes = [u32, u32, vp, vp]
    L.r3dm_dev_akaze_msurf_check.argtypes = [u32, u32, u32, vp, vp, u32, vp]
    L.r3dm_dev_akaze_msurf.argtypes = [vp, u32, u32, u32, vp, vp, u32, vp, vp]
    L._r3dm_dev_msurf_bound = True
    return L


def dev_akaze_msurf_levels(L, width: int, height: int):
    """r3dm_dev_akaze_msurf_levels: the level table the M-SURF arm forms for a width x height image (border from 12 sqrt(2)), as
    dev_akaze_tail_levels gives the MLDB one"""
    bind_dev_akaze_msurf(L)
    lv = (DevAkLevel * 16)(); n = C.c_uint32(0)
    rc = L.r3dm_dev_akaze_msurf_levels(width, height, C.addressof(lv), C.addressof(n))
    if rc != 0:
        raise R3dmError(f"r3dm_dev_akaze_msurf_levels -> {rc}")
    return [{k: getattr(lv[i], k) for k, _ in DevAkLevel._fields_} for i in range(n.value)]


def dev_msurf_args(planes, items):
    """the arrays of the M-SURF entries.  planes: [n_levels] of (Lx, Ly) float32 [h, w]; items: MSURF_ITEM records
    -> (n_levels, plane_dims, plane pointers, n, items, keep-alive)"""
    keep = [[np.ascontiguousarray(q, np.float32) for q in lev] for lev in planes]
    nl = len(keep)
    dims = np.array([[lev[0].shape[1], lev[0].shape[0]] for lev in keep], np.uint32).reshape(nl, 2)
    ptrs = (C.c_void_p * max(2 * nl, 1))(*[q.ctypes.data for lev in keep for q in lev])
    its = np.ascontiguousarray(items, MSURF_ITEM)
    return nl, dims, ptrs, len(its), its, keep


def dev_akaze_msurf_check(L, width: int, height: int, planes, items) -> int:
    """r3dm_dev_akaze_msurf_check: 0 when the kernel reads these planes and items inside the planes, R3DM_ERR_INVALID else; needs no device"""
    bind_dev_akaze_msurf(L)
    nl, dims, ptrs, n, its, keep = dev_msurf_args(planes, items)
    return L.r3dm_dev_akaze_msurf_check(width, height, nl, _ptr(dims), C.addressof(ptrs), n, its.ctypes.data)


def dev_tail_args(images):
    """the arrays of the tail entries.  images: per image a dict with planes [n_levels] of (Ldet, Lx, Ly, Lt) float32 [h, w] and lists
    [n_levels] of [n, 3] float32 (x, y, response).  -> (n_levels, plane_dims [n_levels, 2] uint32, plane pointers, n_list [B, n_levels]
    uint32, lists [sum, 3] float32, keep-alive)"""
    nl = len(images[0]["planes"])
    keep = [[[np.ascontiguousarray(q, np.float32) for q in lev] for lev in im["planes"]] for im in images]
    dims = np.array([[lev[0].shape[1], lev[0].shape[0]] for lev in keep[0]], np.uint32).reshape(nl, 2)
    ptrs = (C.c_void_p * (len(images) * nl * 4))(*[q.ctypes.data for im in keep for lev in im for q in lev])
    ls = [np.ascontiguousarray(l, np.float32).reshape(-1, 3) for im in images for l in im["lists"]]
    n_list = np.array([len(l) for l in ls], np.uint32)
    lists = np.ascontiguousarray(np.concatenate(ls + [np.zeros((1, 3), np.float32)]))
    return nl, dims, ptrs, n_list, lists, keep


class DevAkPlan(C.Structure):
    """r3dm_dev_ak_plan (developer build, api_akaze.cpp): what the scale space launched for one level"""
    _fields_ = [("head_form", C.c_int32), ("head_rows", C.c_int32), ("n_launch", C.c_int32), ("n_steps", C.c_int32),
                ("form", C.c_int32 * 32), ("steps", C.c_int32 * 32), ("rows", C.c_int32 * 32)]


def bind_dev_akaze_head(L):
    """the developer build's Fast-arm head entries (libr3dm_dev.so only, declared in no header), bound when first asked for"""
    if getattr(L, "_r3dm_dev_head_bound", False):
        return L
    if not hasattr(L, "r3dm_dev_akaze_head"):
        raise R3dmError("r3dm_dev_akaze_head exists in the developer build only: use_developer_library() before the first load")
    bind_dev_akaze_tail(L)
    vp, u32 = C.c_void_p, C.c_uint32
    L.r3dm_dev_akaze_head_bound.argtypes = [u32, u32, vp]
    L.r3dm_dev_akaze_head_plan.argtypes = [u32, u32, u32, vp]
    L.r3dm_dev_akaze_head_check.argtypes = [u32, vp, u32, u32]
    L.r3dm_dev_akaze_head.argtypes = [vp, u32, vp, u32, u32, C.c_float, vp, vp, vp, vp, vp]
    L.r3dm_dev_akaze_extrema_check.argtypes = [u32, u32, u32, u32, vp, vp]
    L.r3dm_dev_akaze_extrema.argtypes = [vp, u32, u32, u32, u32, vp, vp, C.c_float, vp, vp]
    L._r3dm_dev_head_bound = True
    return L


def dev_head_bound(L, width: int, height: int) -> int:
    """r3dm_dev_akaze_head_bound: the candidates an image of this size can hold at most -- the triples per image of the head entries' lists"""
    bound = C.c_uint64(0)
    rc = bind_dev_akaze_head(L).r3dm_dev_akaze_head_bound(width, height, C.addressof(bound))
    if rc != 0:
        raise R3dmError(f"r3dm_dev_akaze_head_bound -> {rc}")
    return int(bound.value)


def _dev_plan_dicts(plan, nl):
    return [dict(head_form=plan[i].head_form, head_rows=plan[i].head_rows, n_steps=plan[i].n_steps,
                 launches=[(plan[i].form[m], plan[i].steps[m], plan[i].rows[m]) for m in range(plan[i].n_launch)]) for i in range(nl)]


def dev_head_plan(L, width: int, height: int, B: int = 1):
    """r3dm_dev_akaze_head_plan (needs no device): the launches the scale space issues per level for B width x height images, under this
    process's developer knobs -> per level a dict: head_form (the one-pass level head runs), head_rows, n_steps (FED steps), launches
    [(form: 0 one step, 1 steps through LDS, 2 marching strips; steps; rows per band)]"""
    bind_dev_akaze_head(L)
    nl = len(dev_akaze_tail_levels(L, width, height))
    plan = (DevAkPlan * max(nl, 1))()
    rc = L.r3dm_dev_akaze_head_plan(width, height, B, C.addressof(plan))
    if rc != 0:
        raise R3dmError(f"r3dm_dev_akaze_head_plan -> {rc}")
    return _dev_plan_dicts(plan, nl)


def dev_head_images(images):
    """the image array of r3dm_dev_akaze_head(_check): (pointers, keep-alive)"""
    keep = [np.ascontiguousarray(im, np.float32) for im in images]
    return (C.c_void_p * len(keep))(*[k.ctypes.data for k in keep]), keep


def dev_extrema_args(planes):
    """the arrays of r3dm_dev_akaze_extrema(_check).  planes: per image [n_levels] Ldet float32 [h, w] -> (n_levels, plane_dims
    [n_levels, 2] uint32, plane pointers, keep-alive)"""
    nl = len(planes[0])
    keep = [[np.ascontiguousarray(q, np.float32) for q in im] for im in planes]
    dims = np.array([[q.shape[1], q.shape[0]] for q in keep[0]], np.uint32).reshape(nl, 2)
    ptrs = (C.c_void_p * (len(planes) * nl))(*[q.ctypes.data for im in keep for q in im])
    return nl, dims, ptrs, keep


def _dev_head_lists(counts, lists, B, nl, bound):
    """(n_cand [nl], lists [nl] of [n, 3]) per image from the head entries' counts_out and lists_out"""
    out = []
    for b in range(B):
        at, ls = b * bound, []
        for i in range(nl):
            n = int(counts[b, i, 1])
            ls.append(lists[at:at + n].copy()); at += n
        out.append((counts[b, :, 0].copy(), ls))
    return out


def _ptr(a) -> Optional[int]:
    """address of a numpy array or torch tensor (host or device) -- the ABI takes plain pointers"""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data
    return int(a.data_ptr())           # torch tensor


def _rows_arg(a):
    """a contiguous [n, dim] numpy array or torch tensor for the ABI.  The library reads a device tensor on its own stream: work torch
    has queued on the tensor's current stream must have finished before the call, so that stream is synchronised first."""
    if isinstance(a, np.ndarray):
        return np.ascontiguousarray(a)
    a = a.contiguous()
    if a.is_cuda:
        import torch
        torch.cuda.current_stream(a.device).synchronize()
    return a


def _is_f32(a) -> bool:
    if isinstance(a, np.ndarray):
        return a.dtype == np.float32
    import torch
    return a.dtype == torch.float32


class Graph:
    """PairWiseMatches: pairs [P,2] u32 ordered by (I,J); offsets [P+1] u64; matches [M,2] u32 (i_, j_)."""

    def __init__(self, handle: int):
        self._h = handle

    @property
    def on_device(self) -> int:
        """device id of the graph's device mirror, -1 without one"""
        return load_library().r3dm_graph_on_device(self._h)

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                load_library().r3dm_graph_free(self._h)
                self._h = None
        except Exception:          # interpreter shutdown
            pass

    @property
    def num_pairs(self) -> int:
        return int(load_library().r3dm_graph_num_pairs(self._h))

    @property
    def num_matches(self) -> int:
        return int(load_library().r3dm_graph_num_matches(self._h))

    def _view(self, fn, n, dtype):
        if n == 0:
            return np.zeros(0, dtype)
        addr = fn(self._h)
        buf = (C.c_char * (n * np.dtype(dtype).itemsize)).from_address(addr)
        return np.frombuffer(buf, dtype=dtype).copy()

    @property
    def pairs(self) -> np.ndarray:
        return self._view(load_library().r3dm_graph_pairs, 2 * self.num_pairs, np.uint32).reshape(-1, 2)

    @property
    def offsets(self) -> np.ndarray:
        if self.num_pairs == 0:
            return np.zeros(1, np.uint64)
        return self._view(load_library().r3dm_graph_offsets, self.num_pairs + 1, np.uint64)

    @property
    def matches(self) -> np.ndarray:
        return self._view(load_library().r3dm_graph_matches, 2 * self.num_matches, np.uint32).reshape(-1, 2)

    def as_dict(self):
        """{(I, J): ndarray [m, 2]} -- the std::map view used by the parity tests"""
        p, o, m = self.pairs, self.offsets, self.matches
        return {(int(p[k, 0]), int(p[k, 1])): m[int(o[k]):int(o[k + 1])] for k in range(p.shape[0])}

    def save(self, path: str) -> None:
        rc = load_library().r3dm_save_matches(self._h, path.encode())
        if rc != 0:
            raise R3dmError(f"r3dm_save_matches({path}) -> {rc}")

    @staticmethod
    def load(path: str) -> "Graph":
        h = C.c_void_p()
        rc = load_library().r3dm_load_matches(path.encode(), C.byref(h))
        if rc != 0:
            raise R3dmError(f"r3dm_load_matches({path}) -> {rc}")
        return Graph(h.value)

    @staticmethod
    def from_csr(pairs: np.ndarray, offsets: np.ndarray, matches: np.ndarray) -> "Graph":
        pairs = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2)
        offsets = np.ascontiguousarray(offsets, np.uint64)
        matches = np.ascontiguousarray(matches, np.uint32).reshape(-1, 2)
        h = C.c_void_p()
        rc = load_library().r3dm_graph_from_csr(_ptr(pairs) if pairs.size else None, pairs.shape[0], _ptr(offsets),
                                                 _ptr(matches) if matches.size else None, C.byref(h))
        if rc != 0:
            raise R3dmError(f"r3dm_graph_from_csr -> {rc}")
        return Graph(h.value)

    @staticmethod
    def merge(parts: Sequence["Graph"]) -> "Graph":
        arr = (C.c_void_p * len(parts))(*[p._h for p in parts])
        h = C.c_void_p()
        rc = load_library().r3dm_graph_merge(arr, len(parts), C.byref(h))
        if rc != 0:
            raise R3dmError(f"r3dm_graph_merge -> {rc}")
        return Graph(h.value)


class Tracks:
    """Feature tracks of a match graph (r3dm_build_tracks): track t is observations[offsets[t]:offsets[t + 1]], rows (view id, feature)
    sorted by view id; tracks are sorted by their first observation."""

    def __init__(self, handle: int):
        self._h = handle

    def close(self):
        if getattr(self, "_h", None):
            load_library().r3dm_tracks_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:          # interpreter shutdown
            pass

    def _handle(self) -> int:
        if not getattr(self, "_h", None):
            raise R3dmError("the Tracks object is closed")
        return self._h

    def __len__(self) -> int:
        return int(load_library().r3dm_tracks_count(self._handle()))

    @property
    def offsets(self) -> np.ndarray:
        n = len(self) + 1
        buf = (C.c_char * (8 * n)).from_address(load_library().r3dm_tracks_offsets(self._h))
        return np.frombuffer(buf, dtype=np.uint64).copy()

    @property
    def observations(self) -> np.ndarray:
        n = int(self.offsets[-1])
        if n == 0:
            return np.zeros((0, 2), np.uint32)
        buf = (C.c_char * (8 * n)).from_address(load_library().r3dm_tracks_observations(self._h))
        return np.frombuffer(buf, dtype=np.uint32).copy().reshape(-1, 2)

    @property
    def stats(self) -> TracksStats:
        s = TracksStats()
        rc = load_library().r3dm_tracks_report(self._handle(), C.byref(s))
        if rc != 0:
            raise R3dmError(f"r3dm_tracks_report -> {rc}")
        return s

    @property
    def phase_ms(self) -> np.ndarray:
        """r3dm_tracks_phase_ms: stats.ms_kernels split into [extents, components, sort + filter, outputs]"""
        out = np.zeros(4, np.float64)
        rc = load_library().r3dm_tracks_phase_ms(self._handle(), _ptr(out))
        if rc != 0:
            raise R3dmError(f"r3dm_tracks_phase_ms -> {rc}")
        return out

    def in_pair(self, view_a: int, view_b: int) -> np.ndarray:
        """GetTracksInImages({a, b}): [n, 2] (feature in a, feature in b) of every track that observes both views, in track order"""
        L = load_library()
        n = C.c_uint64()
        rc = L.r3dm_tracks_in_pair(self._handle(), view_a, view_b, None, 0, C.byref(n))
        if rc != 0:
            raise R3dmError(f"r3dm_tracks_in_pair({view_a}, {view_b}) -> {rc}")
        out = np.zeros((n.value, 2), np.uint32)
        if n.value:
            rc = L.r3dm_tracks_in_pair(self._h, view_a, view_b, _ptr(out), n.value, C.byref(n))
            if rc != 0:
                raise R3dmError(f"r3dm_tracks_in_pair({view_a}, {view_b}) -> {rc}")
        return out


def graphs_pack(graphs: Sequence["Graph"]) -> np.ndarray:
    """r3dm_graphs_pack: the wire format of a rank's graphs (uint32 words), for a transport of the caller's own"""
    L = load_library()
    arr = (C.c_void_p * len(graphs))(*[g._h for g in graphs])
    words = C.c_void_p(); n = C.c_uint64()
    rc = L.r3dm_graphs_pack(arr, len(graphs), C.byref(words), C.byref(n))
    if rc != 0:
        raise R3dmError(f"r3dm_graphs_pack -> {rc}")
    try:
        return np.ctypeslib.as_array(C.cast(words, C.POINTER(C.c_uint32)), shape=(n.value,)).copy()
    finally:
        L.r3dm_words_free(words)


def graphs_unpack_merge(rank_words: Sequence[np.ndarray], n_graphs: int) -> List["Graph"]:
    """r3dm_graphs_unpack_merge: the packed graphs of every rank -> the graphs of the whole collection, ordered by (I, J)"""
    L = load_library()
    bufs = [np.ascontiguousarray(w, np.uint32) for w in rank_words]
    ptrs = (C.c_void_p * len(bufs))(*[b.ctypes.data for b in bufs])
    lens = (C.c_uint64 * len(bufs))(*[b.size for b in bufs])
    out = (C.c_void_p * max(n_graphs, 1))()
    rc = L.r3dm_graphs_unpack_merge(ptrs, lens, len(bufs), n_graphs, out)
    if rc != 0:
        raise R3dmError(f"r3dm_graphs_unpack_merge -> {rc}")
    return [Graph(out[k]) for k in range(n_graphs)]


class Comm:
    """r3dm_comm: the RCCL communicator of the one-process-per-GPU route (r3dm_allgather_graphs).  Rank 0 draws the id
    (Comm.unique_id()) and hands its 128 bytes to the other ranks; every rank then creates its end."""

    def __init__(self, unique_id: bytes, rank: int, world: int, device: int = 0):
        L = load_library()
        h = C.c_void_p()
        buf = (C.c_ubyte * 128).from_buffer_copy(unique_id)
        rc = L.r3dm_comm_create(buf, rank, world, device, C.byref(h))
        if rc != 0:
            raise R3dmError(f"r3dm_comm_create -> {rc}")
        self._h = h.value

    @staticmethod
    def unique_id() -> bytes:
        buf = (C.c_ubyte * 128)()
        rc = load_library().r3dm_comm_unique_id(buf)
        if rc != 0:
            raise R3dmError(f"r3dm_comm_unique_id -> {rc}" + (" (librccl.so not found)" if rc == -5 else ""))
        return bytes(buf)

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                load_library().r3dm_comm_destroy(self._h)
                self._h = None
        except Exception:
            pass

    @property
    def rank(self) -> int:
        return load_library().r3dm_comm_rank(self._h)

    @property
    def world(self) -> int:
        return load_library().r3dm_comm_world(self._h)

    @property
    def last_device_graphs(self) -> int:
        """local graphs of the last exchange that went on the wire from their device mirror (Context.set_device_graphs)"""
        return load_library().r3dm_comm_last_device_graphs(self._h)

    def allgather_graphs(self, local: Sequence["Graph"]) -> List["Graph"]:
        L = load_library()
        arr = (C.c_void_p * len(local))(*[g._h for g in local])
        out = (C.c_void_p * max(len(local), 1))()
        rc = L.r3dm_allgather_graphs(self._h, arr, len(local), out)
        if rc != 0:
            raise R3dmError(f"r3dm_allgather_graphs -> {rc}: {L.r3dm_comm_last_error(self._h).decode()}")
        return [Graph(out[k]) for k in range(len(local))]


def _knn_out(nq: int, k: int):
    return np.full((max(nq, 1), max(k, 1)), -1, np.int32), np.zeros((max(nq, 1), max(k, 1)), np.float32)


class Index:
    """r3dm_index: a dataset staged once for many searches.  The approximate matchers' structures (graph, HNSW, forest) are built on it
    by the first kgraph_knn / hnsw_knn / mrpt_knn call, from that call's build parameters; a later call that names other build
    parameters raises.  ctx: any Context of the index's device."""

    def __init__(self, handle: int, binary: bool = False):
        self._h = handle
        self.binary = bool(binary)

    def kgraph_knn(self, ctx: "Context", query, params: "KGraphParams" = None, pair=(0, 1), k: int = 2):
        """ArrayMatcher_kgraph::SearchNeighbours(NN = k) (r3dm_index_kgraph_knn): (idx [nq, k] int32, -1 where the pool ran short;
        dist [nq, k] float32, +inf there).  A binary index (ctx.set_kgraph_hamming on) takes packed uint8 rows and reports Hamming counts."""
        query = np.ascontiguousarray(query, np.uint8) if self.binary else np.ascontiguousarray(query, np.float32)
        kp = params if params is not None else KGraphParams.preset(3)
        nq, k = int(query.shape[0]), int(k)
        idx, dist = _knn_out(nq, k)
        ctx._check(ctx._L.r3dm_index_kgraph_knn(ctx._h, self._h, C.addressof(kp), _ptr(query), nq, pair[0], pair[1], k, _ptr(idx), _ptr(dist)),
                   "r3dm_index_kgraph_knn")
        return idx[:nq], dist[:nq]

    def hnsw_knn(self, ctx: "Context", query, params: "HnswParams" = None, k: int = 2):
        """ArrayMatcher_hnsw::SearchNeighbours(NN = k) (r3dm_index_hnsw_knn)"""
        query = np.ascontiguousarray(query, np.float32)
        hp = params if params is not None else HnswParams.preset(2)
        nq, k = int(query.shape[0]), int(k)
        idx, dist = _knn_out(nq, k)
        ctx._check(ctx._L.r3dm_index_hnsw_knn(ctx._h, self._h, C.addressof(hp), _ptr(query), nq, k, _ptr(idx), _ptr(dist)), "r3dm_index_hnsw_knn")
        return idx[:nq], dist[:nq]

    def mrpt_knn(self, ctx: "Context", query, params: "MrptParams" = None, k: int = 2):
        """ArrayMatcher_mrpt::SearchNeighbours(NN = k) (r3dm_index_mrpt_knn): a dropped query holds -1 / -1 in all k entries; dist = SQUARE ROOTS"""
        query = np.ascontiguousarray(query, np.float32)
        mp = params if params is not None else MrptParams.preset()
        nq, k = int(query.shape[0]), int(k)
        idx, dist = _knn_out(nq, k)
        ctx._check(ctx._L.r3dm_index_mrpt_knn(ctx._h, self._h, C.addressof(mp), _ptr(query), nq, k, _ptr(idx), _ptr(dist)), "r3dm_index_mrpt_knn")
        return idx[:nq], dist[:nq]

    def close(self):
        if getattr(self, "_h", None):
            load_library().r3dm_index_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    """One GPU, one context (one process per GPU)."""

    def __init__(self, device: int = 0):
        L = load_library()
        h = C.c_void_p()
        rc = L.r3dm_create(device, C.byref(h))
        if rc != 0:
            raise R3dmError(f"r3dm_create(device={device}) -> {rc} (no gfx950 GPU visible? there is no CPU fallback)")
        self._h = h.value
        self._L = L

    def close(self):
        if getattr(self, "_h", None):
            self._L.r3dm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:          # interpreter shutdown: ctypes globals may already be gone
            pass

    def _check(self, rc: int, what: str):
        if rc != 0:
            raise R3dmError(f"{what} -> {rc}: {self._L.r3dm_last_error(self._h).decode()}")

    def device_info(self) -> Tuple[str, int, int]:
        arch = C.create_string_buffer(64); cu = C.c_int(); hbm = C.c_uint64()
        self._check(self._L.r3dm_device_info(self._h, arch, 64, C.byref(cu), C.byref(hbm)), "r3dm_device_info")
        return arch.value.decode(), cu.value, hbm.value

    def set_image(self, view_id: int, desc, xy=None, width: int = 0, height: int = 0, binary: bool = False):
        """desc: [n, dim] float32 / uint8 numpy array or torch tensor (host or device memory)."""
        if isinstance(desc, np.ndarray):
            desc = np.ascontiguousarray(desc)
            is_f32 = desc.dtype == np.float32
            if not is_f32 and desc.dtype != np.uint8:
                raise TypeError(desc.dtype)
        else:
            import torch
            desc = desc.contiguous()
            is_f32 = desc.dtype == torch.float32
            if not is_f32 and desc.dtype != torch.uint8:
                raise TypeError(desc.dtype)
        n, dim = int(desc.shape[0]), int(desc.shape[1])
        dt = F32 if is_f32 else (BIN if binary else U8)
        if xy is not None:
            xy = np.ascontiguousarray(xy, np.float32) if isinstance(xy, np.ndarray) else xy.contiguous().float()
        self._check(self._L.r3dm_set_image(self._h, view_id, width, height, _ptr(desc), n, dim, dt, _ptr(xy)),
                    "r3dm_set_image")

    def set_images(self, view_ids, descs, xys=None, width: int = 0, height: int = 0, binary: bool = False, wait: bool = False):
        """a whole collection in one call (r3dm_set_images): descs / xys are sequences of [n, dim] / [n, 2] arrays (numpy: host memory,
        copied through the library's page-locked ring by helper threads; torch: device or page-locked tensors, copied by the copy engine straight
        into the ring's device slot).  wait: return when every view is
        resident and laid out (r3dm_images_wait) instead of when the caller's buffers are consumed."""
        keep = []
        arr = (ViewDesc * len(view_ids))()
        for k, vid in enumerate(view_ids):
            d = descs[k]
            if isinstance(d, np.ndarray):
                d = np.ascontiguousarray(d)
                is_f32 = d.dtype == np.float32
                if not is_f32 and d.dtype != np.uint8:
                    raise TypeError(d.dtype)
            else:
                import torch
                d = d.contiguous()
                is_f32 = d.dtype == torch.float32
                if not is_f32 and d.dtype != torch.uint8:
                    raise TypeError(d.dtype)
            x = None if xys is None else xys[k]
            if x is not None:
                x = np.ascontiguousarray(x, np.float32) if isinstance(x, np.ndarray) else x.contiguous().float()
            keep.append((d, x))
            arr[k] = ViewDesc(int(vid), width, height, int(d.shape[0]), int(d.shape[1]), F32 if is_f32 else (BIN if binary else U8), _ptr(d), _ptr(x))
        self._check(self._L.r3dm_set_images(self._h, C.cast(arr, C.c_void_p), len(view_ids)), "r3dm_set_images")
        if wait:
            self.images_wait()

    def images_wait(self):
        self._check(self._L.r3dm_images_wait(self._h), "r3dm_images_wait")

    def memory_info(self):
        """-> (device bytes of the slabs the registered views' layouts are cut from, device bytes of the upload ring, its page-locked host bytes)"""
        a = C.c_uint64(); b = C.c_uint64(); h = C.c_uint64()
        self._check(self._L.r3dm_memory_info(self._h, C.byref(a), C.byref(b), C.byref(h)), "r3dm_memory_info")
        return a.value, b.value, h.value

    def view_info(self, view_id: int):
        """-> (layout bits LAYOUT_*, bytes of HBM the view's layouts and indices occupy, views whose rows went through the page-locked ring, views copied straight from the caller's device / page-locked buffers)"""
        lay = C.c_uint32(); b = C.c_uint64(); ru = C.c_uint64(); du = C.c_uint64()
        self._check(self._L.r3dm_view_info(self._h, view_id, C.byref(lay), C.byref(b), C.byref(ru), C.byref(du)), "r3dm_view_info")
        return lay.value, b.value, ru.value, du.value

    def clear_images(self):
        self._check(self._L.r3dm_clear_images(self._h), "r3dm_clear_images")

    def trim(self):
        """give the staging buffers kept by clear_images() back to the device"""
        self._check(self._L.r3dm_trim(self._h), "r3dm_trim")

    def match_pairs(self, pairs, dist_ratio: float = 0.6, squared_metric: bool = True) -> Graph:
        pairs = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2)
        h = C.c_void_p()
        self._check(self._L.r3dm_match_pairs(self._h, _ptr(pairs) if pairs.size else None, pairs.shape[0],
                                             dist_ratio, int(squared_metric), C.byref(h)), "r3dm_match_pairs")
        return Graph(h.value)

    def match_pairs_kgraph(self, pairs, dist_ratio: float = 0.6, params: "KGraphParams" = None) -> Graph:
        """kgraph_match: approximate 2-NN through a per-view graph index (config C5)"""
        pairs = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2)
        kp = params if params is not None else KGraphParams.preset(3)
        h = C.c_void_p()
        self._check(self._L.r3dm_match_pairs_kgraph(self._h, _ptr(pairs) if pairs.size else None, pairs.shape[0], dist_ratio,
                                                    C.addressof(kp), C.byref(h)), "r3dm_match_pairs_kgraph")
        return Graph(h.value)

    def kgraph_knn2(self, dataset, query, params: "KGraphParams" = None, pair=(0, 1), binary: bool = False):
        """binary: packed uint8 rows under the Hamming metric (r3dm_kgraph_knn2_bits), distances are the counts as float32"""
        rows_t, entry, name = (np.uint8, self._L.r3dm_kgraph_knn2_bits, "r3dm_kgraph_knn2_bits") if binary else \
                              (np.float32, self._L.r3dm_kgraph_knn2, "r3dm_kgraph_knn2")
        dataset = np.ascontiguousarray(dataset, rows_t); query = np.ascontiguousarray(query, rows_t)
        kp = params if params is not None else KGraphParams.preset(3)
        nq = query.shape[0]
        idx = np.full((max(nq, 1), 2), -1, np.int32); dist = np.zeros((max(nq, 1), 2), np.float32)
        self._check(entry(self._h, _ptr(dataset), dataset.shape[0], _ptr(query), nq, dataset.shape[1],
                          C.addressof(kp), pair[0], pair[1], _ptr(idx), _ptr(dist)), name)
        return idx[:nq], dist[:nq]

    def kgraph_knn(self, dataset, query, params: "KGraphParams" = None, pair=(0, 1), k: int = 2, binary: bool = False):
        """ArrayMatcher_kgraph::SearchNeighbours(NN = k), k = 1 .. KNN_MAX (r3dm_kgraph_knn): the pool holds k + search_P entries;
        (idx [nq, k] int32, -1 where the pool ran short; dist [nq, k] float32, +inf there).  binary: packed uint8 rows under the
        Hamming metric (r3dm_kgraph_knn_bits)"""
        rows_t, entry, name = (np.uint8, self._L.r3dm_kgraph_knn_bits, "r3dm_kgraph_knn_bits") if binary else \
                              (np.float32, self._L.r3dm_kgraph_knn, "r3dm_kgraph_knn")
        dataset = np.ascontiguousarray(dataset, rows_t); query = np.ascontiguousarray(query, rows_t)
        kp = params if params is not None else KGraphParams.preset(3)
        nq, k = int(query.shape[0]), int(k)
        idx, dist = _knn_out(nq, k)
        self._check(entry(self._h, _ptr(dataset), dataset.shape[0], _ptr(query), nq, dataset.shape[1],
                          C.addressof(kp), pair[0], pair[1], k, _ptr(idx), _ptr(dist)), name)
        return idx[:nq], dist[:nq]

    def set_kgraph_hamming(self, enable: bool = True):
        """opt-in (include/r3dm.h: r3dm_set_kgraph_hamming): match_pairs_kgraph, kgraph_index and Index.kgraph_knn serve binary views --
        Hamming index and search on the packed rows, the ratio unsquared.  Off: they refuse binary views."""
        self._check(self._L.r3dm_set_kgraph_hamming(self._h, int(bool(enable))), "r3dm_set_kgraph_hamming")

    def kgraph_hamming_report(self) -> dict:
        """r3dm_kgraph_hamming_report: indices built and searches launched by the packed-row kernels since the context was created"""
        s = KGraphHammingStats()
        self._check(self._L.r3dm_kgraph_hamming_report(self._h, C.byref(s)), "r3dm_kgraph_hamming_report")
        return {"n_index_builds": int(s.n_index_builds), "n_search_launches": int(s.n_search_launches)}

    def drop_indices(self):
        """r3dm_drop_indices: the next match_pairs_kgraph rebuilds the graph index of every view it uses"""
        self._check(self._L.r3dm_drop_indices(self._h), "r3dm_drop_indices")

    def kgraph_index(self, view_id: int, n_rows: int, index_K: int = 24):
        """-> (adj [n, 64] uint32 padded with 0xFFFFFFFF, deg [n] uint32) of a registered view"""
        adj = np.zeros((n_rows, 64), np.uint32); deg = np.zeros(n_rows, np.uint32)
        self._check(self._L.r3dm_kgraph_index(self._h, view_id, index_K, _ptr(adj), _ptr(deg)), "r3dm_kgraph_index")
        return adj, deg

    def match_pairs_hnsw(self, pairs, dist_ratio: float = 0.6, params: "HnswParams" = None) -> Graph:
        """hnsw_match: hnswlib's searchKnn on a batch-built HNSW index per first view (matchingAlgorithm 6 / 7 / 8)"""
        pairs = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2)
        hp = params if params is not None else HnswParams.preset(2)
        h = C.c_void_p()
        self._check(self._L.r3dm_match_pairs_hnsw(self._h, _ptr(pairs) if pairs.size else None, pairs.shape[0], dist_ratio,
                                                  C.addressof(hp), C.byref(h)), "r3dm_match_pairs_hnsw")
        return Graph(h.value)

    def match_pairs_mrpt(self, pairs, dist_ratio: float = 0.6, params: "MrptParams" = None) -> Graph:
        """mrpt_match (matchingAlgorithm 5): random projection trees per first view, vote, exact re-rank (r3dm_match_pairs_mrpt)"""
        pairs = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2)
        mp = params if params is not None else MrptParams.preset()
        h = C.c_void_p()
        self._check(self._L.r3dm_match_pairs_mrpt(self._h, _ptr(pairs) if pairs.size else None, pairs.shape[0], dist_ratio,
                                                  C.addressof(mp), C.byref(h)), "r3dm_match_pairs_mrpt")
        return Graph(h.value)

    def mrpt_knn2(self, dataset, query, params: "MrptParams" = None):
        """ArrayMatcher_mrpt-shaped: (idx [nq, 2] int32 (-1: dropped), dist [nq, 2] float32 = SQUARE ROOTS of the squared L2 distances)"""
        dataset = np.ascontiguousarray(dataset, np.float32); query = np.ascontiguousarray(query, np.float32)
        mp = params if params is not None else MrptParams.preset()
        nq = query.shape[0]
        idx = np.full((max(nq, 1), 2), -1, np.int32); dist = np.zeros((max(nq, 1), 2), np.float32)
        self._check(self._L.r3dm_mrpt_knn2(self._h, _ptr(dataset), dataset.shape[0], _ptr(query), nq, dataset.shape[1],
                                           C.addressof(mp), _ptr(idx), _ptr(dist)), "r3dm_mrpt_knn2")
        return idx[:nq], dist[:nq]

    def mrpt_knn(self, dataset, query, params: "MrptParams" = None, k: int = 2):
        """ArrayMatcher_mrpt::SearchNeighbours(NN = k) (r3dm_mrpt_knn): (idx [nq, k] int32, dist [nq, k] float32 = SQUARE ROOTS); a query
        with fewer than k elected rows after the retry is dropped: -1 / -1 in all k entries"""
        dataset = np.ascontiguousarray(dataset, np.float32); query = np.ascontiguousarray(query, np.float32)
        mp = params if params is not None else MrptParams.preset()
        nq, k = int(query.shape[0]), int(k)
        idx, dist = _knn_out(nq, k)
        self._check(self._L.r3dm_mrpt_knn(self._h, _ptr(dataset), dataset.shape[0], _ptr(query), nq, dataset.shape[1],
                                          C.addressof(mp), k, _ptr(idx), _ptr(dist)), "r3dm_mrpt_knn")
        return idx[:nq], dist[:nq]

    def mrpt_index(self, view_id: int, n_rows: int, dim: int, params: "MrptParams" = None) -> dict:
        """the MRPT index of a registered view as arrays (r3dm_mrpt_index), cut to the view's clamped depth"""
        mp = params if params is not None else MrptParams.preset()
        nl = 1 << mp.depth
        R = np.zeros((mp.n_trees * mp.depth, dim), np.float32); sp = np.zeros((mp.n_trees, nl - 1), np.float32)
        lv = np.zeros((mp.n_trees, n_rows), np.int32); lf = np.zeros(nl + 1, np.int32); d = C.c_uint32(0)
        self._check(self._L.r3dm_mrpt_index(self._h, view_id, C.addressof(mp), _ptr(R), _ptr(sp), _ptr(lv), _ptr(lf), C.byref(d)), "r3dm_mrpt_index")
        d = d.value; nl = 1 << d
        return dict(R=R.reshape(-1)[:mp.n_trees * d * dim].reshape(mp.n_trees * d, dim).copy(), splits=sp.reshape(-1)[:mp.n_trees * (nl - 1)].reshape(mp.n_trees, nl - 1).copy(),
                    leaves=lv, leaf_first=lf[:nl + 1].copy(), depth=d)

    def hnsw_knn2(self, dataset, query, params: "HnswParams" = None):
        dataset = np.ascontiguousarray(dataset, np.float32); query = np.ascontiguousarray(query, np.float32)
        hp = params if params is not None else HnswParams.preset(2)
        nq = query.shape[0]
        idx = np.full((max(nq, 1), 2), -1, np.int32); dist = np.zeros((max(nq, 1), 2), np.float32)
        self._check(self._L.r3dm_hnsw_knn2(self._h, _ptr(dataset), dataset.shape[0], _ptr(query), nq, dataset.shape[1],
                                           C.addressof(hp), _ptr(idx), _ptr(dist)), "r3dm_hnsw_knn2")
        return idx[:nq], dist[:nq]

    def hnsw_knn(self, dataset, query, params: "HnswParams" = None, k: int = 2):
        """ArrayMatcher_hnsw::SearchNeighbours(NN = k) (r3dm_hnsw_knn): searchKnn(row, k) with the beam max(ef, k); (idx [nq, k], dist [nq, k])"""
        dataset = np.ascontiguousarray(dataset, np.float32); query = np.ascontiguousarray(query, np.float32)
        hp = params if params is not None else HnswParams.preset(2)
        nq, k = int(query.shape[0]), int(k)
        idx, dist = _knn_out(nq, k)
        self._check(self._L.r3dm_hnsw_knn(self._h, _ptr(dataset), dataset.shape[0], _ptr(query), nq, dataset.shape[1],
                                          C.addressof(hp), k, _ptr(idx), _ptr(dist)), "r3dm_hnsw_knn")
        return idx[:nq], dist[:nq]

    def hnsw_knn_on_index(self, dataset, index: dict, M: int, query, ef: int, k: int):
        """searchKnn(row, k) with setEf(ef) on an index given as arrays (r3dm_hnsw_knn_on_index; keys as hnsw_knn2_on_index)"""
        dataset = np.ascontiguousarray(dataset, np.float32); query = np.ascontiguousarray(query, np.float32)
        l0 = np.ascontiguousarray(index["links0"], np.int32); uo = np.ascontiguousarray(index["up_off"], np.int32)
        ul = np.ascontiguousarray(index["up_links"], np.int32).reshape(-1, 1 + M)
        a = HnswArrays(M, l0.ctypes.data, uo.ctypes.data, ul.ctypes.data if ul.size else None, ul.shape[0], int(index["enterpoint"]), int(index["maxlevel"]))
        nq, k = int(query.shape[0]), int(k)
        idx, dist = _knn_out(nq, k)
        self._check(self._L.r3dm_hnsw_knn_on_index(self._h, _ptr(dataset), dataset.shape[0], dataset.shape[1], C.addressof(a),
                                                   _ptr(query), nq, ef, k, _ptr(idx), _ptr(dist)), "r3dm_hnsw_knn_on_index")
        return idx[:nq], dist[:nq]

    def hnsw_knn2_on_index(self, dataset, index: dict, M: int, query, ef: int):
        """searchKnn(row, 2) with setEf(ef) on an index given as arrays (keys links0, up_off, up_links, enterpoint, maxlevel)"""
        dataset = np.ascontiguousarray(dataset, np.float32); query = np.ascontiguousarray(query, np.float32)
        l0 = np.ascontiguousarray(index["links0"], np.int32); uo = np.ascontiguousarray(index["up_off"], np.int32)
        ul = np.ascontiguousarray(index["up_links"], np.int32).reshape(-1, 1 + M)
        a = HnswArrays(M, l0.ctypes.data, uo.ctypes.data, ul.ctypes.data if ul.size else None, ul.shape[0], int(index["enterpoint"]), int(index["maxlevel"]))
        nq = query.shape[0]
        idx = np.full((max(nq, 1), 2), -1, np.int32); dist = np.zeros((max(nq, 1), 2), np.float32)
        self._check(self._L.r3dm_hnsw_knn2_on_index(self._h, _ptr(dataset), dataset.shape[0], dataset.shape[1], C.addressof(a),
                                                    _ptr(query), nq, ef, _ptr(idx), _ptr(dist)), "r3dm_hnsw_knn2_on_index")
        return idx[:nq], dist[:nq]

    def hnsw_index(self, view_id: int, n_rows: int, params: "HnswParams" = None) -> dict:
        """the HNSW index of a registered view as arrays in hnswlib's shape (r3dm_hnsw_arrays)"""
        hp = params if params is not None else HnswParams.preset(2)
        M = hp.M
        l0 = np.zeros((n_rows, 1 + 2 * M), np.int32); uo = np.zeros(n_rows + 1, np.int32)
        cap = n_rows + 64
        ul = np.zeros((cap, 1 + M), np.int32)
        rows = C.c_uint32(0); ep = C.c_int32(0); ml = C.c_int32(0)
        self._check(self._L.r3dm_hnsw_index(self._h, view_id, C.addressof(hp), _ptr(l0), _ptr(uo), _ptr(ul), cap, C.byref(rows), C.byref(ep), C.byref(ml)),
                    "r3dm_hnsw_index")
        return dict(links0=l0, up_off=uo, up_links=ul[:rows.value].copy(), enterpoint=ep.value, maxlevel=ml.value,
                    levels=np.diff(uo).astype(np.int32))

    def filter_F(self, putative: Graph, max_residual_px: float = 4.0, max_iter: int = 2048, seed: int = 5489,
                 want_F: bool = False):
        h = C.c_void_p()
        Fbuf = np.zeros((max(putative.num_pairs, 1), 9), np.float64) if want_F else None
        self._check(self._L.r3dm_filter_F(self._h, putative._h, max_residual_px, max_iter, seed, 0, C.byref(h),
                                          _ptr(Fbuf)), "r3dm_filter_F")
        g = Graph(h.value)
        return (g, Fbuf[:g.num_pairs].copy()) if want_F else g

    def filter_H(self, putative: Graph, max_residual_px: float = 4.0, max_iter: int = 2048, seed: int = 5489,
                 want_H: bool = False):
        h = C.c_void_p()
        Hbuf = np.zeros((max(putative.num_pairs, 1), 9), np.float64) if want_H else None
        self._check(self._L.r3dm_filter_H(self._h, putative._h, max_residual_px, max_iter, seed, C.byref(h), _ptr(Hbuf)),
                    "r3dm_filter_H")
        g = Graph(h.value)
        return (g, Hbuf[:g.num_pairs].copy()) if want_H else g

    def set_device_graphs(self, enable: bool = True):
        """r3dm_set_device_graphs: graphs produced from now on keep a device mirror (sent by Comm.allgather_graphs without a host round trip)"""
        self._check(self._L.r3dm_set_device_graphs(self._h, int(bool(enable))), "r3dm_set_device_graphs")

    def build_tracks(self, graph: Graph, min_length: int = 2, want_graph: bool = False):
        """r3dm_build_tracks: the tracks of `graph` (TracksBuilder Build + Filter); with want_graph also the graph restricted to the
        matches whose component is a track"""
        h = C.c_void_p(); k = C.c_void_p()
        self._check(self._L.r3dm_build_tracks(self._h, graph._h, min_length, C.byref(h), C.byref(k) if want_graph else None), "r3dm_build_tracks")
        return (Tracks(h.value), Graph(k.value)) if want_graph else Tracks(h.value)

    def set_integer_mfma(self, enable: bool = True):
        """opt-in bf16-exact MFMA path for integer-valued descriptors (include/r3dm.h: r3dm_set_integer_mfma)"""
        self._check(self._L.r3dm_set_integer_mfma(self._h, int(bool(enable))), "r3dm_set_integer_mfma")

    def set_hamming_mfma(self, enable: bool = True):
        """opt-in exact MFMA formulation of the Hamming matcher (include/r3dm.h: r3dm_set_hamming_mfma)"""
        self._check(self._L.r3dm_set_hamming_mfma(self._h, int(bool(enable))), "r3dm_set_hamming_mfma")

    def set_knn_narrow_tiles(self, enable: bool = True):
        """opt-in K-list nominators on the bf16 tiles / split-f16 planes for knn / index_knn with k >= 3 (include/r3dm.h:
        r3dm_set_knn_narrow_tiles); same results, Stats.n_knn_integer_tiles / n_knn_split_tiles tell which tiles a call ran on"""
        self._check(self._L.r3dm_set_knn_narrow_tiles(self._h, int(bool(enable))), "r3dm_set_knn_narrow_tiles")

    def set_knn_hamming_tiles(self, enable: bool = True):
        """opt-in K-list nominator on the i8 MFMA tiles for knn / index_knn with k >= 3 on binary rows (include/r3dm.h:
        r3dm_set_knn_hamming_tiles); same results, Stats.n_knn_hamming_tiles counts the launch"""
        self._check(self._L.r3dm_set_knn_hamming_tiles(self._h, int(bool(enable))), "r3dm_set_knn_hamming_tiles")

    def set_prefix_pruning(self, enable: bool = True):
        """prefix pruning of the f32 matcher in match mode, default on (include/r3dm.h: r3dm_set_prefix_pruning); graphs are the same
        either way"""
        self._check(self._L.r3dm_set_prefix_pruning(self._h, int(bool(enable))), "r3dm_set_prefix_pruning")

    def prefix_pruning_counts(self):
        """(tiles tested, tiles pruned) of the last match_pairs call; (0, 0) when the pruning kernel did not run"""
        out = (C.c_uint64 * 2)()
        self._check(self._L.r3dm_get_prefix_pruning_counts(self._h, out), "r3dm_get_prefix_pruning_counts")
        return int(out[0]), int(out[1])

    def pair_filter_counts(self):
        """tiles of the last match_pairs call that the pair-norm filter pruned (part of prefix_pruning_counts()[1])"""
        out = C.c_uint64(0)
        self._check(self._L.r3dm_get_pair_filter_counts(self._h, C.byref(out)), "r3dm_get_pair_filter_counts")
        return int(out.value)

    def set_half_filter(self, enable: bool = True):
        """the f16 level in front of the pair-norm filter, default on (include/r3dm.h: r3dm_set_half_filter); it prunes only tiles the
        filter would prune, so graphs and the other counters are the same either way"""
        self._check(self._L.r3dm_set_half_filter(self._h, int(bool(enable))), "r3dm_set_half_filter")

    def half_filter_counts(self):
        """tiles of the last match_pairs call that the f16 level pruned (part of pair_filter_counts())"""
        out = C.c_uint64(0)
        self._check(self._L.r3dm_get_half_filter_counts(self._h, C.byref(out)), "r3dm_get_half_filter_counts")
        return int(out.value)

    def level2_skip_counts(self):
        """tiles of the last match_pairs call that went from the f16 level straight to the restart, the filter provably unable to
        prune them (0 with the f16 level off)"""
        out = C.c_uint64(0)
        self._check(self._L.r3dm_get_level2_skip_counts(self._h, C.byref(out)), "r3dm_get_level2_skip_counts")
        return int(out.value)

    def set_min_tile_test(self, enable: bool = True):
        """the min form of the three levels' tile tests, default on (include/r3dm.h: r3dm_set_min_tile_test); it decides every tile as
        the general form does, so graphs and the other counters are the same either way"""
        self._check(self._L.r3dm_set_min_tile_test(self._h, int(bool(enable))), "r3dm_set_min_tile_test")

    def min_tile_test_counts(self):
        """(pairs matched in the min form, pairs matched in the general form) by the three-level kernel in the last match_pairs call"""
        out = (C.c_uint64 * 2)()
        self._check(self._L.r3dm_get_min_tile_test_counts(self._h, out), "r3dm_get_min_tile_test_counts")
        return int(out[0]), int(out[1])

    def set_half_prefix(self, enable: bool = True):
        """the restart's prefix test on f16 rows in front of the restart, default on (include/r3dm.h: r3dm_set_half_prefix); it prunes
        only tiles the restart's own prefix test would, so graphs and the other counters are the same either way"""
        self._check(self._L.r3dm_set_half_prefix(self._h, int(bool(enable))), "r3dm_set_half_prefix")

    def half_prefix_counts(self):
        """(tiles that reached the f16 prefix test, tiles it pruned) in the last match_pairs call"""
        out = (C.c_uint64 * 2)()
        self._check(self._L.r3dm_get_half_prefix_counts(self._h, out), "r3dm_get_half_prefix_counts")
        return int(out[0]), int(out[1])

    def set_mutual_matching(self, enable: bool = True):
        """opt-in mutual nearest-neighbour matching (include/r3dm.h: r3dm_set_mutual_matching): a match (i, j) of match_pairs and the
        approximate matchers is kept iff j is the nearest row of J to row i under (distance, row index); Stats.n_mutual_checked /
        n_mutual_dropped report the last call.  knn2 / knn / the index entries return raw lists and ignore it"""
        self._check(self._L.r3dm_set_mutual_matching(self._h, int(bool(enable))), "r3dm_set_mutual_matching")

    def set_symmetric_ratio(self, enable: bool = True):
        """opt-in symmetric ratio test (include/r3dm.h: r3dm_set_symmetric_ratio): a match (i, j) of match_pairs and the approximate
        matchers is kept iff the 2-NN + ratio rule with the views swapped accepts it too -- j is the nearest row of J to row i AND
        f(d1) < R f(d2) with the forward test's R and f, d2 the smallest distance from row i to another row of J; no match survives
        a view J of fewer than two rows.  Contains the mutual rule; independent of set_mutual_matching.  Raw-list entries ignore it"""
        self._check(self._L.r3dm_set_symmetric_ratio(self._h, int(bool(enable))), "r3dm_set_symmetric_ratio")

    def symmetric_ratio_report(self):
        """r3dm_symmetric_ratio_report of the last collecting call -> (checked, dropped_not_nearest, dropped_ratio); zeros after a call
        with the switch off"""
        a, b, c = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._check(self._L.r3dm_symmetric_ratio_report(self._h, C.byref(a), C.byref(b), C.byref(c)), "r3dm_symmetric_ratio_report")
        return int(a.value), int(b.value), int(c.value)

    def set_view_priority(self, view_id: int, priority):
        """r3dm_set_view_priority: one float per row of the view (its feature scale: finite, >= 0), or None to remove it"""
        p = None if priority is None else np.ascontiguousarray(priority, np.float32).reshape(-1)
        self._check(self._L.r3dm_set_view_priority(self._h, view_id, None if p is None else p.ctypes.data, 0 if p is None else p.size), "r3dm_set_view_priority")

    def preselect_pairs(self, pairs, head_rows: int = 128, dist_ratio: float = 0.6, squared_metric: bool = True) -> np.ndarray:
        """r3dm_preselect_pairs: the count of every pair (its accepted queries when the head_rows largest-priority rows of J are
        2-NN-matched against those of I), in the caller's order; works whatever set_preemptive_matching says"""
        pairs = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2)
        counts = np.zeros(pairs.shape[0], np.uint32)
        self._check(self._L.r3dm_preselect_pairs(self._h, _ptr(pairs) if pairs.size else None, pairs.shape[0], head_rows, dist_ratio,
                                                 int(squared_metric), _ptr(counts) if counts.size else None), "r3dm_preselect_pairs")
        return counts

    def set_preemptive_matching(self, enable: bool = True, head_rows: int = 128, min_matches: int = 4):
        """opt-in preemptive matching (include/r3dm.h: r3dm_set_preemptive_matching): match_pairs and the approximate matchers match a
        pair only if its preselect count reaches min_matches -- dropped pairs lose real matches; knn2 / knn / the index entries ignore it"""
        self._check(self._L.r3dm_set_preemptive_matching(self._h, int(bool(enable)), head_rows, min_matches), "r3dm_set_preemptive_matching")

    def set_match_budget(self, enable: bool = True, max_rows: int = 8192):
        """opt-in match budget (include/r3dm.h: r3dm_set_match_budget): match_pairs and the approximate matchers match only each view's
        max_rows highest-priority rows (a view of at most max_rows rows is matched whole) and return the view's own row numbers -- rows
        outside the budget lose their matches; knn2 / knn / the index entries, guided matching and the filters ignore it"""
        self._check(self._L.r3dm_set_match_budget(self._h, int(bool(enable)), max_rows), "r3dm_set_match_budget")

    def budget_rows(self, view_id: int, max_rows: int) -> np.ndarray:
        """r3dm_budget_rows: the rows of the view the budget max_rows selects (device selection), ascending; works whatever
        set_match_budget says"""
        rows = np.zeros(max(min(int(max_rows), 1 << 22), 1), np.uint32)      # (a view holds fewer than 2^22 rows)
        cnt = C.c_uint32(0)
        self._check(self._L.r3dm_budget_rows(self._h, view_id, max_rows, _ptr(rows), C.byref(cnt)), "r3dm_budget_rows")
        return rows[:cnt.value].copy()

    def budget_report(self) -> dict:
        """r3dm_budget_report: the budget's share of the last collection call (kernel times, wall time, views budgeted / whole, sub-views
        built, rows selected, matches remapped)"""
        s = BudgetStats()
        self._check(self._L.r3dm_budget_report(self._h, C.byref(s)), "r3dm_budget_report")
        return s.as_dict()

    def preselect_report(self) -> dict:
        """r3dm_preselect_report: the gate of the last call (times, pairs, pairs kept, heads built, views without priority)"""
        s = PreselectStats()
        self._check(self._L.r3dm_preselect_report(self._h, C.byref(s)), "r3dm_preselect_report")
        return s.as_dict()

    def vocab_sample(self, view_ids, n_words: int) -> Vocab:
        """r3dm_vocab_sample: a vocabulary of n_words rows, the deterministic even sample of the listed registered views (one type,
        one length, each listed once): word t is row floor((2 t + 1) T / (2 n_words)) of their T rows in list order"""
        ids = np.ascontiguousarray(view_ids, np.uint32).reshape(-1)
        h = C.c_void_p()
        self._check(self._L.r3dm_vocab_sample(self._h, _ptr(ids) if ids.size else None, ids.size, n_words, C.byref(h)), "r3dm_vocab_sample")
        return Vocab(self._L, h.value)

    def vocab_from_rows(self, rows, binary: bool = False) -> Vocab:
        """r3dm_vocab_from_rows: the caller's own words, [n_words, dim] float32 (F32), uint8 (U8) or uint8 with binary=True (BIN)"""
        rows = np.asarray(rows)
        dtype = BIN if binary else (U8 if rows.dtype == np.uint8 else F32)
        rows = np.ascontiguousarray(rows, np.uint8 if dtype != F32 else np.float32)
        h = C.c_void_p()
        self._check(self._L.r3dm_vocab_from_rows(self._h, _ptr(rows) if rows.size else None, rows.shape[0], rows.shape[1] if rows.ndim == 2 else 0, dtype,
                                                 C.byref(h)), "r3dm_vocab_from_rows")
        return Vocab(self._L, h.value)

    def view_signatures(self, vocab: Vocab, view_ids) -> np.ndarray:
        """r3dm_view_signatures: the word histograms of the listed views, [n_views, n_words] uint32 in list order"""
        ids = np.ascontiguousarray(view_ids, np.uint32).reshape(-1)
        out = np.zeros((ids.size, vocab.n_words), np.uint32)
        self._check(self._L.r3dm_view_signatures(self._h, vocab._h, _ptr(ids) if ids.size else None, ids.size, _ptr(out) if out.size else None), "r3dm_view_signatures")
        return out

    def propose_pairs(self, vocab: Vocab, view_ids, top_k: int, with_scores: bool = False, cap_pairs=None):
        """r3dm_propose_pairs: every listed view's top_k partners by histogram intersection, as unique pairs (min id, max id) sorted by
        (I, J): [n_pairs, 2] uint32 -- and, with_scores, the [n_views, n_views] uint32 score matrix in list order (diagonal 0).
        cap_pairs: the room handed to the library (default n_views * top_k, the least it accepts)"""
        ids = np.ascontiguousarray(view_ids, np.uint32).reshape(-1)
        cap = ids.size * max(int(top_k), 0) if cap_pairs is None else int(cap_pairs)
        pairs = np.zeros((max(cap, 1), 2), np.uint32)
        scores = np.zeros((ids.size, ids.size), np.uint32) if with_scores else None
        n = C.c_uint64(0)
        self._check(self._L.r3dm_propose_pairs(self._h, vocab._h, _ptr(ids) if ids.size else None, ids.size, top_k, _ptr(pairs), cap, C.byref(n),
                                               _ptr(scores) if with_scores and scores.size else None), "r3dm_propose_pairs")
        pairs = pairs[:int(n.value)].copy()
        return (pairs, scores) if with_scores else pairs

    def vocab_report(self, vocab: Vocab) -> dict:
        """r3dm_vocab_report: rows quantised, signatures built / cached and the HIP-event times of the phases of the last call"""
        s = VocabStats()
        rc = self._L.r3dm_vocab_report(vocab._h, C.byref(s))
        if rc != 0:
            raise R3dmError(f"r3dm_vocab_report -> {rc}")
        return s.as_dict()

    def vocab_train(self, init: Vocab, view_ids, max_iterations: int) -> Vocab:
        """r3dm_vocab_train: Lloyd's iterations on the device over every row of the listed views, starting from `init` (left as it is);
        the new vocabulary has init's type, length and word count and no signatures.  The rule is in include/r3dm.h"""
        ids = np.ascontiguousarray(view_ids, np.uint32).reshape(-1)
        h = C.c_void_p()
        self._check(self._L.r3dm_vocab_train(self._h, init._h, _ptr(ids) if ids.size else None, ids.size, max_iterations, C.byref(h)), "r3dm_vocab_train")
        return Vocab(self._L, h.value)

    def vocab_train_report(self, vocab: Vocab) -> dict:
        """r3dm_vocab_train_report: updates run, converged, moved / empty / largest member count of the last assignment, rows assigned
        and the HIP-event times of assignment, sort and update of the r3dm_vocab_train call that made `vocab`"""
        s = VocabTrainStats()
        rc = self._L.r3dm_vocab_train_report(vocab._h, C.byref(s))
        if rc != 0:
            raise R3dmError(f"r3dm_vocab_train_report -> {rc}")
        return s.as_dict()

    def set_split_mfma(self, enable: bool = True):
        """opt-in split-f16 nominator for real-valued descriptors (include/r3dm.h: r3dm_set_split_mfma)"""
        self._check(self._L.r3dm_set_split_mfma(self._h, int(bool(enable))), "r3dm_set_split_mfma")

    def set_intrinsics(self, view_id: int, K):
        K = None if K is None else np.ascontiguousarray(K, np.float64).reshape(9)
        self._check(self._L.r3dm_set_intrinsics(self._h, view_id, _ptr(K)), "r3dm_set_intrinsics")

    def filter_E(self, putative: Graph, max_residual_px: float = 4.0, max_iter: int = 2048, seed: int = 5489,
                 min_count: int = 50, min_ratio: float = 0.3, want_E: bool = False):
        h = C.c_void_p()
        Ebuf = np.zeros((max(putative.num_pairs, 1), 9), np.float64) if want_E else None
        self._check(self._L.r3dm_filter_E(self._h, putative._h, max_residual_px, max_iter, seed, min_count, min_ratio,
                                          C.byref(h), _ptr(Ebuf)), "r3dm_filter_E")
        g = Graph(h.value)
        return (g, Ebuf[:g.num_pairs].copy()) if want_E else g

    def filter_FEH(self, putative: Graph, which: str = "FEH", max_residual_px: float = 4.0, max_iter: int = 2048, seed: int = 5489,
                   min_count: int = 50, min_ratio: float = 0.3):
        """r3dm_filter_FEH: the requested filters side by side -> ({"F": Graph, ...}, ms_kernels [F, E, H], ms_wall [F, E, H])"""
        bits = sum({"F": 1, "E": 2, "H": 4}[k] for k in which)
        hs = {k: C.c_void_p() for k in "FEH"}
        msk = np.zeros(3); msw = np.zeros(3)
        self._check(self._L.r3dm_filter_FEH(self._h, putative._h, max_residual_px, max_iter, seed, bits, min_count, min_ratio,
                                            C.byref(hs["F"]), C.byref(hs["E"]), C.byref(hs["H"]), _ptr(msk), _ptr(msw)), "r3dm_filter_FEH")
        return {k: Graph(hs[k].value) for k in which}, msk, msw

    def set_guided_matching(self, enable: bool = True, ratio_F: float = 0.6, ratio_E: float = 0.6, ratio_H: float = -1.0):
        """r3dm_set_guided_matching: the filters return the guided lists of their accepted pairs (ratio < 0: geometry only)"""
        self._check(self._L.r3dm_set_guided_matching(self._h, int(bool(enable)), ratio_F, ratio_E, ratio_H), "r3dm_set_guided_matching")

    def set_keypoint_detector(self, detector: str = "Fast-AKAZE"):
        """r3dm_set_keypoint_detector: the arm of the features entries, "Fast-AKAZE" (default) or "AKAZE" (classic A-KAZE)"""
        _detector_flag(detector)
        self._check(self._L.r3dm_set_keypoint_detector(self._h, DETECTORS[detector]), "r3dm_set_keypoint_detector")

    def set_descriptor_arm(self, descriptor: str = "LIOP"):
        """r3dm_set_descriptor_arm: what the features entries describe the keypoints with, "LIOP" (default: .desc rows of 144 floats),
        "MLDB" (the Fast-AKAZE detector's MLDB-486: .desc rows of 61 bytes) or "MSURF" (its M-SURF-64: .desc rows of 64 floats; the
        detector then runs on the level table with the M-SURF border)"""
        _descriptor_flag(descriptor)
        self._check(self._L.r3dm_set_descriptor_arm(self._h, DESCRIPTOR_ARMS[descriptor]), "r3dm_set_descriptor_arm")

    def akaze_classic_components(self) -> np.ndarray:
        """r3dm_akaze_classic_components: [32] component-size histogram of the classic arm's kpts_aux walk since creation
        (bin k: components of 2^k .. 2^(k+1) - 1 candidates)"""
        h = np.zeros(32, np.uint64)
        self._check(self._L.r3dm_akaze_classic_components(self._h, _ptr(h)), "r3dm_akaze_classic_components")
        return h

    def dev_akaze_classic_walk(self, levels, width: int, height: int, lists, parallel: bool = True, bound: int = 64):
        """r3dm_dev_akaze_classic_walk (developer build): the classic arm's kpts_aux walk and upper-level filter on the caller's
        candidate lists, one per image (see dev_walk_args) -> per image a dict: x, y, size, resp [n_slots] float32 and cls [n_slots]
        uint32 in list order, kept [n_slots] bool (the upper-level filter), hist [32] (component sizes of the parallel form)"""
        L = bind_dev_akaze_classic_walk(self._L)
        lv, n_cand, words = dev_walk_args(levels, lists)
        B = len(lists)
        n_slots = np.zeros(max(B, 1), np.uint32); out = np.zeros((max(len(words), 1), 6), np.uint32); hist = np.zeros((max(B, 1), 32), np.uint32)
        self._check(L.r3dm_dev_akaze_classic_walk(self._h, C.addressof(lv), len(levels), width, height, B, _ptr(n_cand), _ptr(words),
                                                  int(bool(parallel)), bound, _ptr(n_slots), _ptr(out), _ptr(hist)), "r3dm_dev_akaze_classic_walk")
        res, at = [], 0
        for b in range(B):
            o = out[at:at + int(n_slots[b])]
            f = np.ascontiguousarray(o[:, :4]).view(np.float32)
            res.append(dict(x=f[:, 0].copy(), y=f[:, 1].copy(), size=f[:, 2].copy(), resp=f[:, 3].copy(), cls=o[:, 4].copy(),
                            kept=o[:, 5] != 0, hist=hist[b].copy()))
            at += int(n_cand[b])
        return res

    def dev_akaze_classic_head(self, images, threshold: float):
        """r3dm_dev_akaze_classic_head (developer build): the classic arm's head -- k-contrast, scale space, derivatives, determinant,
        extremum passes, the functions the detector calls -- on same-size images [h, w] in [0, 1] -> per image a dict: hmax_bits
        (uint32), hist [300] uint32, inv_k2 [8] float32, planes [n_levels] of dicts Lsmooth, Lflow (None at level 0), Lt, Lx, Ly, Ldet
        float32 [h_i, w_i], counts [n_levels] uint32, and the candidates in scan order: x, y, level uint32 and value float32"""
        L = bind_dev_akaze_classic_head(self._L)
        ptrs, keep = dev_head_images(images)
        B = len(keep)
        h, w = keep[0].shape
        lv = dev_akaze_classic_levels(L, w, h)
        nl, cap = len(lv), max(dev_classic_bound(lv), 1)
        names = ("Lsmooth", "Lflow", "Lt", "Lx", "Ly", "Ldet")
        planes = [[[np.zeros((e["h"], e["w"]), np.float32) for _ in names] for e in lv] for _ in range(B)]
        pp = (C.c_void_p * (B * nl * 6))(*[q.ctypes.data for im in planes for lev in im for q in lev])
        small = np.zeros((B, 309), np.uint32); counts = np.zeros((B, nl), np.uint32); n = np.zeros(B, np.uint32)
        cand = np.zeros((B, cap, 4), np.uint32)
        self._check(L.r3dm_dev_akaze_classic_head(self._h, B, C.addressof(ptrs), w, h, float(threshold), _ptr(small), C.addressof(pp),
                                                  _ptr(counts), cap, _ptr(n), _ptr(cand)), "r3dm_dev_akaze_classic_head")
        del keep
        res = _dev_classic_candidates(counts, n, cand, B)
        for b, r in enumerate(res):
            r.update(hmax_bits=small[b, 0].copy(), hist=small[b, 1:301].copy(), inv_k2=small[b, 301:309].copy().view(np.float32),
                     planes=[{k: (None if i == 0 and k == "Lflow" else q) for k, q in zip(names, lev)} for i, lev in enumerate(planes[b])])
        return res

    def dev_akaze_classic_extrema(self, width: int, height: int, planes, threshold: float):
        """r3dm_dev_akaze_classic_extrema (developer build): the classic arm's extremum passes, row scan and totals on the caller's
        determinant planes (per image [n_levels] float32 [h_i, w_i], the level table of width x height; any value) -> per image a
        dict: counts [n_levels] uint32 and the candidates in scan order (x, y, level, value)"""
        L = bind_dev_akaze_classic_head(self._L)
        nl, dims, ptrs, keep = dev_extrema_args(planes)
        B = len(planes)
        cap = max(dev_classic_bound(dev_akaze_classic_levels(L, width, height)), 1)
        counts = np.zeros((B, max(nl, 1)), np.uint32); n = np.zeros(B, np.uint32); cand = np.zeros((B, cap, 4), np.uint32)
        self._check(L.r3dm_dev_akaze_classic_extrema(self._h, width, height, B, nl, _ptr(dims), C.addressof(ptrs), float(threshold),
                                                     _ptr(counts), cap, _ptr(n), _ptr(cand)), "r3dm_dev_akaze_classic_extrema")
        del keep
        return _dev_classic_candidates(counts, n, cand, B)

    def dev_akaze_tail(self, width: int, height: int, images):
        """r3dm_dev_akaze_tail (developer build): the Fast arm's tail -- cross-level filters, refinement, orientation, compaction, the
        host's angles, MLDB -- on the caller's planes and lists (see dev_tail_args) -> per image a dict: n, the seven record fields
        (x, y, size, response, max_x, max_y float32; level uint32), theta, cos, sin [n] float32, desc [n, 61] uint8, dead [per level]
        [n_i, 2] uint8 (dead_lower, dead_upper of every list entry)"""
        L = bind_dev_akaze_tail(self._L)
        nl, dims, ptrs, n_list, lists, keep = dev_tail_args(images)
        B = len(images)
        total = max(int(n_list.sum()), 1)
        n_kp = np.zeros(B, np.uint32); recs = np.zeros((total, 8), np.uint32); ang = np.zeros((total, 3), np.float32)
        desc = np.zeros((total, 61), np.uint8); dead = np.zeros((total, 2), np.uint8)
        self._check(L.r3dm_dev_akaze_tail(self._h, width, height, B, nl, _ptr(dims), C.addressof(ptrs), _ptr(n_list), _ptr(lists),
                                          _ptr(n_kp), _ptr(recs), _ptr(ang), _ptr(desc), _ptr(dead)), "r3dm_dev_akaze_tail")
        del keep
        res, at = [], 0
        per = n_list.reshape(B, nl)
        for b in range(B):
            n = int(n_kp[b])
            r = recs[at:at + n]; f = np.ascontiguousarray(r[:, :6]).view(np.float32)
            out = dict(n=n, level=r[:, 6].copy(), theta=ang[at:at + n, 0].copy(), cos=ang[at:at + n, 1].copy(), sin=ang[at:at + n, 2].copy(),
                       desc=desc[at:at + n].copy(), dead=[])
            for j, k in enumerate(("x", "y", "size", "response", "max_x", "max_y")):
                out[k] = f[:, j].copy()
            e = at
            for i in range(nl):
                out["dead"].append(dead[e:e + int(per[b, i])].copy()); e += int(per[b, i])
            res.append(out)
            at += int(per[b].sum())
        return res

    def dev_akaze_msurf(self, width: int, height: int, planes, items) -> np.ndarray:
        """r3dm_dev_akaze_msurf (developer build): the product's M-SURF-64 kernel on the caller's Lx / Ly planes (see dev_msurf_args)
        and items, through r3dm_dev_akaze_msurf_check first -> rows [n, 64] float32"""
        L = bind_dev_akaze_msurf(self._L)
        nl, dims, ptrs, n, its, keep = dev_msurf_args(planes, items)
        rows = np.zeros((n, 64), np.float32)
        self._check(L.r3dm_dev_akaze_msurf(self._h, width, height, nl, _ptr(dims), C.addressof(ptrs), n, its.ctypes.data, rows.ctypes.data),
                    "r3dm_dev_akaze_msurf")
        del keep
        return rows

    def dev_akaze_head(self, images, threshold: float):
        """r3dm_dev_akaze_head (developer build): the Fast arm's head -- scale space, extremum pass, in-level pruning, the product's
        own launches -- on same-size images [h, w] in [0, 1] -> (per image a dict: planes [n_levels] of [Ldet, Lx, Ly, Lt] float32,
        n_cand [n_levels] uint32, lists [n_levels] of [n, 3] float32 in list order, hmax_bits (uint32), hist [300] uint32, inv_k2 [8]
        float32; plan: per level a dict head_form, head_rows, n_steps, launches [(form, steps, rows per band)])"""
        L = bind_dev_akaze_head(self._L)
        ptrs, keep = dev_head_images(images)
        B = len(keep)
        h, w = keep[0].shape
        lv = dev_akaze_tail_levels(L, w, h)
        nl = len(lv)
        bound = dev_head_bound(L, w, h)
        planes = [[[np.zeros((e["h"], e["w"]), np.float32) for _ in range(4)] for e in lv] for _ in range(B)]
        pp = (C.c_void_p * max(B * nl * 4, 1))(*[q.ctypes.data for im in planes for lev in im for q in lev])
        counts = np.zeros((B, max(nl, 1), 2), np.uint32); lists = np.zeros((B * max(bound, 1), 3), np.float32)
        small = np.zeros((B, 309), np.uint32); plan = (DevAkPlan * max(nl, 1))()
        self._check(L.r3dm_dev_akaze_head(self._h, B, C.addressof(ptrs), w, h, float(threshold), C.addressof(pp), _ptr(counts), _ptr(lists),
                                          _ptr(small), C.addressof(plan)), "r3dm_dev_akaze_head")
        del keep
        res = []
        for b, (n_cand, ls) in enumerate(_dev_head_lists(counts, lists, B, nl, bound)):
            res.append(dict(planes=planes[b], n_cand=n_cand, lists=ls, hmax_bits=small[b, 0].copy(), hist=small[b, 1:301].copy(),
                            inv_k2=small[b, 301:309].copy().view(np.float32)))
        return res, _dev_plan_dicts(plan, nl)

    def dev_akaze_extrema(self, width: int, height: int, planes, threshold: float):
        """r3dm_dev_akaze_extrema (developer build): the Fast arm's extremum pass and in-level pruning on the caller's determinant
        planes (per image [n_levels] float32 [h_i, w_i], the level table of width x height) -> per image (n_cand [n_levels] uint32,
        lists [n_levels] of [n, 3] float32 (x, y, response) in list order)"""
        L = bind_dev_akaze_head(self._L)
        nl, dims, ptrs, keep = dev_extrema_args(planes)
        B = len(planes)
        bound = dev_head_bound(L, width, height)
        counts = np.zeros((B, max(nl, 1), 2), np.uint32); lists = np.zeros((B * max(bound, 1), 3), np.float32)
        self._check(L.r3dm_dev_akaze_extrema(self._h, width, height, B, nl, _ptr(dims), C.addressof(ptrs), float(threshold), _ptr(counts),
                                             _ptr(lists)), "r3dm_dev_akaze_extrema")
        del keep
        return _dev_head_lists(counts, lists, B, nl, bound)

    def guided_match(self, pairs, kind: str, models, threshold_px, ratio: float) -> Graph:
        """r3dm_guided_match: guided matching of `pairs` (a Graph -- only its pair list is read -- or an (P, 2) array in (I, J) order)
        with the caller's models (P x 9: F, E or H) and thresholds (P, as filter_report reports them); ratio < 0: geometry only"""
        if isinstance(pairs, Graph):
            g = pairs
        else:
            pa = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2)
            key = pa[:, 0].astype(np.uint64) << np.uint64(32) | pa[:, 1].astype(np.uint64)
            if pa.shape[0] > 1 and not np.all(key[1:] > key[:-1]):
                raise ValueError("guided_match: pairs must be distinct and in (I, J) order")
            g = Graph.from_csr(pa, np.arange(pa.shape[0] + 1, dtype=np.uint64), np.zeros((pa.shape[0], 2), np.uint32))
        P = g.num_pairs
        M = np.ascontiguousarray(models, np.float64).reshape(P, 9)
        T = np.ascontiguousarray(threshold_px, np.float64).reshape(P)
        h = C.c_void_p()
        self._check(self._L.r3dm_guided_match(self._h, g._h, GUIDED_KIND[kind], _ptr(M) if P else None, _ptr(T) if P else None, float(ratio),
                                              C.byref(h)), "r3dm_guided_match")
        return Graph(h.value)

    def guided_report(self) -> dict:
        """r3dm_guided_report: the last guided step (times, pairs, queries, candidates, matches, candidates per query)"""
        s = GuidedStats()
        self._check(self._L.r3dm_guided_report(self._h, C.byref(s)), "r3dm_guided_report")
        return s.as_dict()

    def knn2(self, dataset: np.ndarray, query: np.ndarray, binary: bool = False):
        dataset = np.ascontiguousarray(dataset); query = np.ascontiguousarray(query)
        dt = F32 if dataset.dtype == np.float32 else (BIN if binary else U8)
        nq = query.shape[0]
        idx = np.full((max(nq, 1), 2), -1, np.int32); dist = np.zeros((max(nq, 1), 2), np.float32)
        self._check(self._L.r3dm_knn2(self._h, _ptr(dataset), dataset.shape[0], _ptr(query), nq, dataset.shape[1], dt,
                                      _ptr(idx), _ptr(dist)), "r3dm_knn2")
        return idx[:nq], dist[:nq]

    def knn(self, dataset, query, k: int, binary: bool = False):
        """ArrayMatcher::SearchNeighbours(NN = k), k = 1 .. KNN_MAX (r3dm_knn): (idx [nq, k] int32, dist [nq, k] float32), each row
        ascending under (distance, dataset row).  dataset / query: numpy arrays or torch tensors (host or device memory)."""
        dataset = _rows_arg(dataset); query = _rows_arg(query)
        dt = F32 if _is_f32(dataset) else (BIN if binary else U8)
        nq, k = int(query.shape[0]), int(k)
        idx = np.full((max(nq, 1), max(k, 1)), -1, np.int32); dist = np.zeros((max(nq, 1), max(k, 1)), np.float32)
        self._check(self._L.r3dm_knn(self._h, _ptr(dataset), int(dataset.shape[0]), _ptr(query), nq, int(dataset.shape[1]), dt, k,
                                     _ptr(idx), _ptr(dist)), "r3dm_knn")
        return idx[:nq], dist[:nq]

    def index_knn(self, index: "Index", query, k: int):
        """ArrayMatcher::SearchNeighbours(NN = k) against a staged dataset (r3dm_index_knn); any context of the index's device"""
        query = _rows_arg(query)
        nq, k = int(query.shape[0]), int(k)
        idx = np.full((max(nq, 1), max(k, 1)), -1, np.int32); dist = np.zeros((max(nq, 1), max(k, 1)), np.float32)
        self._check(self._L.r3dm_index_knn(self._h, index._h, _ptr(query), nq, k, _ptr(idx), _ptr(dist)), "r3dm_index_knn")
        return idx[:nq], dist[:nq]

    def index_create(self, dataset: np.ndarray, binary: bool = False) -> "Index":
        """ArrayMatcher::Build: stage the dataset once (r3dm_index_create)"""
        dataset = np.ascontiguousarray(dataset)
        dt = F32 if dataset.dtype == np.float32 else (BIN if binary else U8)
        h = C.c_void_p()
        self._check(self._L.r3dm_index_create(self._h, _ptr(dataset), dataset.shape[0], dataset.shape[1], dt, C.byref(h)), "r3dm_index_create")
        return Index(h.value, binary=dt == BIN)

    def index_knn2(self, index: "Index", query: np.ndarray):
        """ArrayMatcher::SearchNeighbours(NN = 2) against a staged dataset; any context of the index's device"""
        query = np.ascontiguousarray(query)
        nq = query.shape[0]
        idx = np.full((max(nq, 1), 2), -1, np.int32); dist = np.zeros((max(nq, 1), 2), np.float32)
        self._check(self._L.r3dm_index_knn2(self._h, index._h, _ptr(query), nq, _ptr(idx), _ptr(dist)), "r3dm_index_knn2")
        return idx[:nq], dist[:nq]

    def liop_describe_patches(self, patches):
        """patches: [n, 41, 41] float32 (numpy or torch, host or device) -> (desc [n, 144] float32, n_resorted)"""
        if isinstance(patches, np.ndarray):
            patches = np.ascontiguousarray(patches, np.float32)
        n, side = int(patches.shape[0]), int(patches.shape[1])
        out = np.zeros((max(n, 1), 144), np.float32)
        nt = C.c_uint32(0)
        self._check(self._L.r3dm_liop_describe_patches(self._h, _ptr(patches), n, side, _ptr(out), C.byref(nt)),
                    "r3dm_liop_describe_patches")
        return out[:n], int(nt.value)

    def extract_liop(self, image, keypoints, kp_size_factor: float = 8.0, want_patches: bool = False):
        """image: [h, w] float32 gray/255; keypoints: [n, 4] float32 (x, y, size, angle_deg) -> desc [n, 144]"""
        image = np.ascontiguousarray(image, np.float32) if isinstance(image, np.ndarray) else image.contiguous()
        keypoints = np.ascontiguousarray(keypoints, np.float32)
        n = keypoints.shape[0]
        desc = np.zeros((max(n, 1), 144), np.float32)
        patches = np.zeros((max(n, 1), 41, 41), np.float32) if want_patches else None
        self._check(self._L.r3dm_extract_liop(self._h, _ptr(image), int(image.shape[1]), int(image.shape[0]), _ptr(keypoints), n,
                                              kp_size_factor, _ptr(desc), _ptr(patches)), "r3dm_extract_liop")
        return (desc[:n], patches[:n]) if want_patches else desc[:n]

    def detect_akaze(self, image, threshold: float = 0.001, cap: int = 200000):
        """image: [h, w] float32 in [0, 1] (numpy or torch, host or device) -> (keypoints [n, 4] (x, y, size, angle_deg), responses [n])"""
        h, w = int(image.shape[0]), int(image.shape[1])
        if isinstance(image, np.ndarray):
            image = np.ascontiguousarray(image, np.float32)
        kps = np.zeros((cap, 4), np.float32); resp = np.zeros(cap, np.float32)
        n = C.c_uint32(0)
        self._check(self._L.r3dm_detect_akaze(self._h, _ptr(image), w, h, threshold, _ptr(kps), _ptr(resp), cap, C.byref(n)),
                    "r3dm_detect_akaze")
        k = min(n.value, cap)
        return kps[:k].copy(), resp[:k].copy()

    def detect_akaze_mldb(self, image, threshold: float = 0.001, cap: int = 200000):
        """AKAZE2::detectAndCompute(DESCRIPTOR_MLDB) -> (keypoints [n, 4], descriptors [n, 61] uint8)"""
        h, w = int(image.shape[0]), int(image.shape[1])
        if isinstance(image, np.ndarray):
            image = np.ascontiguousarray(image, np.float32)
        kps = np.zeros((cap, 4), np.float32); desc = np.zeros((cap, 61), np.uint8)
        n = C.c_uint32(0)
        self._check(self._L.r3dm_detect_akaze_mldb(self._h, _ptr(image), w, h, threshold, _ptr(kps), _ptr(desc), cap, C.byref(n)),
                    "r3dm_detect_akaze_mldb")
        k = min(n.value, cap)
        return kps[:k].copy(), desc[:k].copy()

    def detect_akaze_batch(self, images, threshold: float = 0.001, cap: int = 200000):
        """r3dm_detect_akaze_batch: B same-size images (numpy or torch, host or device) in one pass of the detector
        -> list of (keypoints [n, 4], responses [n])"""
        imgs = [im if hasattr(im, "data_ptr") else np.ascontiguousarray(im, np.float32) for im in images]
        B = len(imgs); h, w = int(imgs[0].shape[0]), int(imgs[0].shape[1])
        assert all(tuple(im.shape) == (h, w) for im in imgs), "a batch holds images of one size"
        ip = (C.c_void_p * B)(*[(im.data_ptr() if hasattr(im, "data_ptr") else im.ctypes.data) for im in imgs])
        kps = [np.zeros((cap, 4), np.float32) for _ in range(B)]; resp = [np.zeros(cap, np.float32) for _ in range(B)]
        kp_p = (C.c_void_p * B)(*[k.ctypes.data for k in kps]); rp_p = (C.c_void_p * B)(*[r.ctypes.data for r in resp])
        n = np.zeros(B, np.uint32)
        self._check(self._L.r3dm_detect_akaze_batch(self._h, B, ip, w, h, threshold, kp_p, rp_p, cap, _ptr(n)), "r3dm_detect_akaze_batch")
        return [(kps[b][:min(int(n[b]), cap)].copy(), resp[b][:min(int(n[b]), cap)].copy()) for b in range(B)]

    def _detect_describe_batch(self, arm: str, entry: str, images, threshold: float, cap: int, single: bool = False):
        """a describing detect entry of `arm` over B same-size images -> list of (keypoints [n, 4], descriptors [n, dim]); single: the
        one image of the list through the entry of one image, `entry` without its _batch"""
        dtype, dim = _ARM_ROWS[arm]
        imgs = [im if hasattr(im, "data_ptr") else np.ascontiguousarray(im, np.float32) for im in images]
        B = len(imgs); h, w = int(imgs[0].shape[0]), int(imgs[0].shape[1])
        assert all(tuple(im.shape) == (h, w) for im in imgs), "a batch holds images of one size"
        ip = (C.c_void_p * B)(*[(im.data_ptr() if hasattr(im, "data_ptr") else im.ctypes.data) for im in imgs])
        kps = [np.zeros((cap, 4), np.float32) for _ in range(B)]; desc = [np.zeros((cap, dim), dtype) for _ in range(B)]
        kp_p = (C.c_void_p * B)(*[k.ctypes.data for k in kps]); dp_p = (C.c_void_p * B)(*[d.ctypes.data for d in desc])
        n = np.zeros(B, np.uint32)
        if single:
            assert B == 1
            entry = entry[:-len("_batch")]
            self._check(getattr(self._L, entry)(self._h, ip[0], w, h, threshold, kp_p[0], dp_p[0], cap, n.ctypes.data_as(C.POINTER(C.c_uint32))), entry)
        else:
            self._check(getattr(self._L, entry)(self._h, B, ip, w, h, threshold, kp_p, dp_p, cap, _ptr(n)), entry)
        return [(kps[b][:min(int(n[b]), cap)].copy(), desc[b][:min(int(n[b]), cap)].copy()) for b in range(B)]

    def detect_akaze_mldb_batch(self, images, threshold: float = 0.001, cap: int = 200000):
        """r3dm_detect_akaze_mldb_batch: B same-size images in one pass of the detector and ONE MLDB launch
        -> list of (keypoints [n, 4], descriptors [n, 61] uint8)"""
        return self._detect_describe_batch("MLDB", "r3dm_detect_akaze_mldb_batch", images, threshold, cap)

    def detect_akaze_msurf_batch(self, images, threshold: float = 0.001, cap: int = 200000, single: bool = False):
        """r3dm_detect_akaze_msurf_batch: B same-size images in one pass of the detector (on the level table with the M-SURF border) and
        ONE M-SURF-64 launch -> list of (keypoints [n, 4], descriptors [n, 64] float32).  single: the one image of the list through
        r3dm_detect_akaze_msurf instead"""
        return self._detect_describe_batch("MSURF", "r3dm_detect_akaze_msurf_batch", images, threshold, cap, single)

    def detect_akaze_classic(self, image, threshold: float = 0.001, cap: int = 200000):
        """r3dm_detect_akaze_classic, Regard3D's "AKAZE" arm (libAKAZE): image [h, w] float32 in [0, 1] (numpy or torch, host or device)
        -> (keypoints [n, 4] (x, y, size, angle in degrees, no + 90), responses [n])"""
        h, w = int(image.shape[0]), int(image.shape[1])
        if isinstance(image, np.ndarray):
            image = np.ascontiguousarray(image, np.float32)
        kps = np.zeros((cap, 4), np.float32); resp = np.zeros(cap, np.float32)
        n = C.c_uint32(0)
        self._check(self._L.r3dm_detect_akaze_classic(self._h, _ptr(image), w, h, threshold, _ptr(kps), _ptr(resp), cap, C.byref(n)),
                    "r3dm_detect_akaze_classic")
        k = min(n.value, cap)
        return kps[:k].copy(), resp[:k].copy()

    def detect_akaze_classic_batch(self, images, threshold: float = 0.001, cap: int = 200000):
        """r3dm_detect_akaze_classic_batch: B same-size images in one pass -> list of (keypoints [n, 4], responses [n])"""
        imgs = [im if hasattr(im, "data_ptr") else np.ascontiguousarray(im, np.float32) for im in images]
        B = len(imgs); h, w = int(imgs[0].shape[0]), int(imgs[0].shape[1])
        assert all(tuple(im.shape) == (h, w) for im in imgs), "a batch holds images of one size"
        ip = (C.c_void_p * B)(*[(im.data_ptr() if hasattr(im, "data_ptr") else im.ctypes.data) for im in imgs])
        kps = [np.zeros((cap, 4), np.float32) for _ in range(B)]; resp = [np.zeros(cap, np.float32) for _ in range(B)]
        kp_p = (C.c_void_p * B)(*[k.ctypes.data for k in kps]); rp_p = (C.c_void_p * B)(*[r.ctypes.data for r in resp])
        n = np.zeros(B, np.uint32)
        self._check(self._L.r3dm_detect_akaze_classic_batch(self._h, B, ip, w, h, threshold, kp_p, rp_p, cap, _ptr(n)),
                    "r3dm_detect_akaze_classic_batch")
        return [(kps[b][:min(int(n[b]), cap)].copy(), resp[b][:min(int(n[b]), cap)].copy()) for b in range(B)]

    def extract_features_batch(self, images, feat_paths, desc_paths, threshold: float = 0.001, bgr: bool = False):
        """r3dm_extract_features_batch: detector + LIOP + .feat / .desc files of B same-size images in one pass.
        images: [h, w] float32 gray / 255, or with bgr=True [h, w, 3] uint8 as cv::imread decodes -> n_features [B]"""
        if bgr:
            imgs = [im if hasattr(im, "data_ptr") else np.ascontiguousarray(im, np.uint8) for im in images]
        else:
            imgs = [im if hasattr(im, "data_ptr") else np.ascontiguousarray(im, np.float32) for im in images]
        B = len(imgs); h, w = int(imgs[0].shape[0]), int(imgs[0].shape[1])
        ip = (C.c_void_p * B)(*[(im.data_ptr() if hasattr(im, "data_ptr") else im.ctypes.data) for im in imgs])
        fp = (C.c_char_p * B)(*[p.encode() for p in feat_paths]); dp = (C.c_char_p * B)(*[p.encode() for p in desc_paths])
        nf = np.zeros(B, np.uint32)
        self._check(self._L.r3dm_extract_features_batch(self._h, B, None if bgr else ip, ip if bgr else None, w, h, threshold, fp, dp, _ptr(nf)),
                    "r3dm_extract_features_batch")
        return nf

    def set_deferred_feature_files(self, on: bool = True):
        """r3dm_set_deferred_feature_files: features calls return when the images are computed; their files are written on the
        context's writer thread (features_files_wait joins it and reports its I/O error)"""
        self._check(self._L.r3dm_set_deferred_feature_files(self._h, 1 if on else 0), "r3dm_set_deferred_feature_files")

    def features_files_wait(self):
        self._check(self._L.r3dm_features_files_wait(self._h), "r3dm_features_files_wait")

    def gray_from_bgr8(self, bgr: np.ndarray) -> np.ndarray:
        bgr = np.ascontiguousarray(bgr, np.uint8)
        out = np.zeros(bgr.shape[:2], np.float32)
        self._check(self._L.r3dm_gray_from_bgr8(self._h, _ptr(bgr), bgr.shape[1], bgr.shape[0], _ptr(out)), "r3dm_gray_from_bgr8")
        return out

    def extract_features_to_files(self, gray, feat_path: str, desc_path: str, threshold: float = 0.001) -> int:
        gray = np.ascontiguousarray(gray, np.float32)
        n = C.c_uint32(0)
        self._check(self._L.r3dm_extract_features_to_files(self._h, _ptr(gray), gray.shape[1], gray.shape[0], threshold,
                                                           feat_path.encode(), desc_path.encode(), C.byref(n)), "r3dm_extract_features_to_files")
        return n.value

    def filter_report(self):
        """per putative pair of the last filter_F call: (threshold_px, nfa, iterations, models, inliers)"""
        n = self._L.r3dm_filter_report(self._h, None, 0)
        arr = (PairReport * max(n, 1))()
        self._L.r3dm_filter_report(self._h, arr, n)
        return [(r.threshold_px, r.nfa, r.iterations, r.models, r.inliers) for r in arr[:n]]

    def features_totals(self) -> FeaturesTotals:
        t = FeaturesTotals()
        self._check(self._L.r3dm_get_features_totals(self._h, C.byref(t)), "r3dm_get_features_totals")
        return t

    def stats(self) -> Stats:
        s = Stats()
        self._check(self._L.r3dm_get_stats(self._h, C.byref(s)), "r3dm_get_stats")
        return s


def shard_owner(pairs: np.ndarray, world: int) -> np.ndarray:
    """r3dm_shard_pairs: the device / rank that the snake deal of rows I gives every pair (host code, no GPU needed)"""
    pairs = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2)
    owner = np.zeros(pairs.shape[0], np.uint32)
    rc = load_library().r3dm_shard_pairs(_ptr(pairs) if pairs.size else None, pairs.shape[0], int(world), _ptr(owner) if pairs.size else None)
    if rc != 0:
        raise R3dmError(f"r3dm_shard_pairs -> {rc}")
    return owner


class MultiContext:
    """r3dm_multi_*: one process driving several GPUs (one context + one host thread per device); device ids may repeat."""

    def __init__(self, device_ids: Sequence[int]):
        L = load_library()
        ids = (C.c_int * len(device_ids))(*device_ids)
        h = C.c_void_p()
        rc = L.r3dm_multi_create(ids, len(device_ids), C.byref(h))
        if rc != 0:
            raise R3dmError(f"r3dm_multi_create({list(device_ids)}) -> {rc} (no gfx950 GPU visible? there is no CPU fallback)")
        self._h = h.value
        self._L = L

    def close(self):
        if getattr(self, "_h", None):
            self._L.r3dm_multi_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, what: str):
        if rc != 0:
            raise R3dmError(f"{what} -> {rc}: {self._L.r3dm_multi_last_error(self._h).decode()}")

    @property
    def num_devices(self) -> int:
        return int(self._L.r3dm_multi_num_devices(self._h))

    def device_stats(self, k: int) -> Stats:
        s = Stats()
        rc = self._L.r3dm_get_stats(self._L.r3dm_multi_ctx(self._h, k), C.byref(s))
        self._check(rc, "r3dm_get_stats")
        return s

    def set_image(self, view_id: int, desc, xy=None, width: int = 0, height: int = 0, binary: bool = False):
        desc = np.ascontiguousarray(desc)
        dt = F32 if desc.dtype == np.float32 else (BIN if binary else U8)
        if xy is not None:
            xy = np.ascontiguousarray(xy, np.float32)
        self._check(self._L.r3dm_multi_set_image(self._h, view_id, width, height, _ptr(desc), desc.shape[0], desc.shape[1], dt, _ptr(xy)),
                    "r3dm_multi_set_image")

    def transfer_counts(self):
        """(views uploaded from host memory, device-to-device copies) of the set_image calls so far"""
        a, b = C.c_uint64(0), C.c_uint64(0)
        self._L.r3dm_multi_transfer_counts.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        self._check(self._L.r3dm_multi_transfer_counts(self._h, C.byref(a), C.byref(b)), "r3dm_multi_transfer_counts")
        return int(a.value), int(b.value)

    def set_intrinsics(self, view_id: int, K):
        K = None if K is None else np.ascontiguousarray(K, np.float64).reshape(9)
        self._check(self._L.r3dm_multi_set_intrinsics(self._h, view_id, _ptr(K)), "r3dm_multi_set_intrinsics")

    def set_integer_mfma(self, enable: bool = True):
        self._check(self._L.r3dm_multi_set_integer_mfma(self._h, int(bool(enable))), "r3dm_multi_set_integer_mfma")

    def set_prefix_pruning(self, enable: bool = True):
        """r3dm_multi_set_prefix_pruning: Context.set_prefix_pruning on every context"""
        self._check(self._L.r3dm_multi_set_prefix_pruning(self._h, int(bool(enable))), "r3dm_multi_set_prefix_pruning")

    def prefix_pruning_counts(self):
        """(tiles tested, tiles pruned) summed over the contexts' last match calls"""
        out = (C.c_uint64 * 2)()
        self._check(self._L.r3dm_multi_get_prefix_pruning_counts(self._h, out), "r3dm_multi_get_prefix_pruning_counts")
        return int(out[0]), int(out[1])

    def pair_filter_counts(self):
        """tiles pruned by the pair-norm filter, summed over the contexts' last match calls"""
        out = C.c_uint64(0)
        self._check(self._L.r3dm_multi_get_pair_filter_counts(self._h, C.byref(out)), "r3dm_multi_get_pair_filter_counts")
        return int(out.value)

    def set_half_filter(self, enable: bool = True):
        """r3dm_multi_set_half_filter: Context.set_half_filter on every context"""
        self._check(self._L.r3dm_multi_set_half_filter(self._h, int(bool(enable))), "r3dm_multi_set_half_filter")

    def half_filter_counts(self):
        """tiles pruned by the f16 level, summed over the contexts' last match calls"""
        out = C.c_uint64(0)
        self._check(self._L.r3dm_multi_get_half_filter_counts(self._h, C.byref(out)), "r3dm_multi_get_half_filter_counts")
        return int(out.value)

    def level2_skip_counts(self):
        """tiles that went from the f16 level straight to the restart, summed over the contexts' last match calls"""
        out = C.c_uint64(0)
        self._check(self._L.r3dm_multi_get_level2_skip_counts(self._h, C.byref(out)), "r3dm_multi_get_level2_skip_counts")
        return int(out.value)

    def set_min_tile_test(self, enable: bool = True):
        """r3dm_multi_set_min_tile_test: Context.set_min_tile_test on every context"""
        self._check(self._L.r3dm_multi_set_min_tile_test(self._h, int(bool(enable))), "r3dm_multi_set_min_tile_test")

    def min_tile_test_counts(self):
        """(min form, general form) pairs, summed over the contexts' last match calls"""
        out = (C.c_uint64 * 2)()
        self._check(self._L.r3dm_multi_get_min_tile_test_counts(self._h, out), "r3dm_multi_get_min_tile_test_counts")
        return int(out[0]), int(out[1])

    def set_half_prefix(self, enable: bool = True):
        """r3dm_multi_set_half_prefix: Context.set_half_prefix on every context"""
        self._check(self._L.r3dm_multi_set_half_prefix(self._h, int(bool(enable))), "r3dm_multi_set_half_prefix")

    def half_prefix_counts(self):
        """(reached the f16 prefix test, pruned by it) tiles, summed over the contexts' last match calls"""
        out = (C.c_uint64 * 2)()
        self._check(self._L.r3dm_multi_get_half_prefix_counts(self._h, out), "r3dm_multi_get_half_prefix_counts")
        return int(out[0]), int(out[1])

    def set_mutual_matching(self, enable: bool = True):
        """r3dm_multi_set_mutual_matching: Context.set_mutual_matching on every context"""
        self._check(self._L.r3dm_multi_set_mutual_matching(self._h, int(bool(enable))), "r3dm_multi_set_mutual_matching")

    def set_symmetric_ratio(self, enable: bool = True):
        """r3dm_multi_set_symmetric_ratio: Context.set_symmetric_ratio on every context"""
        self._check(self._L.r3dm_multi_set_symmetric_ratio(self._h, int(bool(enable))), "r3dm_multi_set_symmetric_ratio")

    def set_kgraph_hamming(self, enable: bool = True):
        """r3dm_multi_set_kgraph_hamming: Context.set_kgraph_hamming on every context"""
        self._check(self._L.r3dm_multi_set_kgraph_hamming(self._h, int(bool(enable))), "r3dm_multi_set_kgraph_hamming")

    def set_view_priority(self, view_id: int, priority):
        """r3dm_multi_set_view_priority: Context.set_view_priority on every context"""
        p = None if priority is None else np.ascontiguousarray(priority, np.float32).reshape(-1)
        self._check(self._L.r3dm_multi_set_view_priority(self._h, view_id, None if p is None else p.ctypes.data, 0 if p is None else p.size),
                    "r3dm_multi_set_view_priority")

    def device_preselect_report(self, k: int) -> dict:
        """r3dm_preselect_report of context k: the gate of its shard of the last call"""
        s = PreselectStats()
        self._check(self._L.r3dm_preselect_report(self._L.r3dm_multi_ctx(self._h, k), C.byref(s)), "r3dm_preselect_report")
        return s.as_dict()

    def set_match_budget(self, enable: bool = True, max_rows: int = 8192):
        """r3dm_multi_set_match_budget: Context.set_match_budget on every context; each budgets its own shard"""
        self._check(self._L.r3dm_multi_set_match_budget(self._h, int(bool(enable)), max_rows), "r3dm_multi_set_match_budget")

    def device_budget_report(self, k: int) -> dict:
        """r3dm_budget_report of context k: the budget's share of its shard of the last call"""
        s = BudgetStats()
        self._check(self._L.r3dm_budget_report(self._L.r3dm_multi_ctx(self._h, k), C.byref(s)), "r3dm_budget_report")
        return s.as_dict()

    def set_preemptive_matching(self, enable: bool = True, head_rows: int = 128, min_matches: int = 4):
        """r3dm_multi_set_preemptive_matching: Context.set_preemptive_matching on every context; each gates its own shard"""
        self._check(self._L.r3dm_multi_set_preemptive_matching(self._h, int(bool(enable)), head_rows, min_matches), "r3dm_multi_set_preemptive_matching")

    def set_guided_matching(self, enable: bool = True, ratio_F: float = 0.6, ratio_E: float = 0.6, ratio_H: float = -1.0):
        self._check(self._L.r3dm_multi_set_guided_matching(self._h, int(bool(enable)), ratio_F, ratio_E, ratio_H), "r3dm_multi_set_guided_matching")

    def set_keypoint_detector(self, detector: str = "Fast-AKAZE"):
        """r3dm_multi_set_keypoint_detector: the arm of extract_features on every context ("Fast-AKAZE" or "AKAZE")"""
        _detector_flag(detector)
        self._check(self._L.r3dm_multi_set_keypoint_detector(self._h, DETECTORS[detector]), "r3dm_multi_set_keypoint_detector")

    def set_descriptor_arm(self, descriptor: str = "LIOP"):
        """r3dm_multi_set_descriptor_arm: what extract_features describes the keypoints with on every context ("LIOP", "MLDB" or "MSURF")"""
        _descriptor_flag(descriptor)
        self._check(self._L.r3dm_multi_set_descriptor_arm(self._h, DESCRIPTOR_ARMS[descriptor]), "r3dm_multi_set_descriptor_arm")

    def extract_features(self, images, feat_paths, desc_paths, threshold: float = 0.001, bgr: bool = False, batch: int = 0):
        """r3dm_multi_extract_features(_bgr8): the features stage over an image list, one BATCH of same-size images in flight per context.
        images: list of [h, w] float32 arrays (gray / 255) -- or, with bgr=True, [h, w, 3] uint8 as cv::imread decodes --
        host (numpy) or device (anything with data_ptr(): torch tensors).
        -> (n_features [N], skipped [N] bool)"""
        imgs = [im if hasattr(im, "data_ptr") else np.ascontiguousarray(im, np.uint8 if bgr else np.float32) for im in images]
        n = len(imgs)
        gp = (C.c_void_p * n)(*[(im.data_ptr() if hasattr(im, "data_ptr") else im.ctypes.data) for im in imgs])
        ws = np.array([im.shape[1] for im in imgs], np.uint32); hs = np.array([im.shape[0] for im in imgs], np.uint32)
        fp = (C.c_char_p * n)(*[p.encode() for p in feat_paths]); dp = (C.c_char_p * n)(*[p.encode() for p in desc_paths])
        nf = np.zeros(n, np.uint32); sk = np.zeros(n, np.uint32)
        err = C.create_string_buffer(512)
        if bgr or batch:
            rc = self._L.r3dm_multi_extract_features_ex(self._h, n, None if bgr else gp, gp if bgr else None, _ptr(ws), _ptr(hs), threshold, fp, dp,
                                                        _ptr(nf), _ptr(sk), batch, err, 512)
        else:
            rc = self._L.r3dm_multi_extract_features(self._h, n, gp, _ptr(ws), _ptr(hs), threshold, fp, dp, _ptr(nf), _ptr(sk), err, 512)
        if rc != 0:
            raise R3dmError(f"r3dm_multi_extract_features -> {rc}: {err.value.decode()}")
        return nf, sk.astype(bool)

    def match_pairs(self, pairs, dist_ratio: float = 0.6, squared_metric: bool = True) -> Graph:
        pairs = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2)
        h = C.c_void_p()
        self._check(self._L.r3dm_multi_match_pairs(self._h, _ptr(pairs) if pairs.size else None, pairs.shape[0],
                                                   dist_ratio, int(squared_metric), C.byref(h)), "r3dm_multi_match_pairs")
        return Graph(h.value)

    def match_pairs_kgraph(self, pairs, dist_ratio: float = 0.6, params: "KGraphParams" = None) -> Graph:
        pairs = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2)
        kp = params if params is not None else KGraphParams.preset(3)
        h = C.c_void_p()
        self._check(self._L.r3dm_multi_match_pairs_kgraph(self._h, _ptr(pairs) if pairs.size else None, pairs.shape[0], dist_ratio,
                                                          C.addressof(kp), C.byref(h)), "r3dm_multi_match_pairs_kgraph")
        return Graph(h.value)

    def match_pairs_hnsw(self, pairs, dist_ratio: float = 0.6, params: "HnswParams" = None) -> Graph:
        pairs = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2)
        hp = params if params is not None else HnswParams.preset(2)
        h = C.c_void_p()
        self._check(self._L.r3dm_multi_match_pairs_hnsw(self._h, _ptr(pairs) if pairs.size else None, pairs.shape[0], dist_ratio,
                                                        C.addressof(hp), C.byref(h)), "r3dm_multi_match_pairs_hnsw")
        return Graph(h.value)

    def _filter(self, fn, what, putative, args, want):
        h = C.c_void_p()
        buf = np.zeros((max(putative.num_pairs, 1), 9), np.float64) if want else None
        self._check(fn(self._h, putative._h, *args, C.byref(h), _ptr(buf)), what)
        g = Graph(h.value)
        return (g, buf[:g.num_pairs].copy()) if want else g

    def filter_F(self, putative: Graph, max_residual_px: float = 4.0, max_iter: int = 2048, seed: int = 5489, want_F: bool = False):
        return self._filter(self._L.r3dm_multi_filter_F, "r3dm_multi_filter_F", putative, (max_residual_px, max_iter, seed), want_F)

    def filter_H(self, putative: Graph, max_residual_px: float = 4.0, max_iter: int = 2048, seed: int = 5489, want_H: bool = False):
        return self._filter(self._L.r3dm_multi_filter_H, "r3dm_multi_filter_H", putative, (max_residual_px, max_iter, seed), want_H)

    def filter_E(self, putative: Graph, max_residual_px: float = 4.0, max_iter: int = 2048, seed: int = 5489,
                 min_count: int = 50, min_ratio: float = 0.3, want_E: bool = False):
        return self._filter(self._L.r3dm_multi_filter_E, "r3dm_multi_filter_E", putative,
                            (max_residual_px, max_iter, seed, min_count, min_ratio), want_E)


