"""ctypes binding of the C ABI declared in include/shardmerge_hip.h.

The product path binds ``libshardmerge_hip.so`` (built in-tree by
``shardmerge_amd/csrc/Makefile``) and nothing else: there is no CPU fallback.
If the library is missing, ``get_lib()`` raises.  ``SmhipLibrary`` takes an
explicit path only so that the test-suite can bind the CPU work-group emulator
it builds under ``tests/emul`` with the same declarations.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path
from typing import Optional

MAX_MODELS = 16
MAX_PAIRS = 32

OK, ERR_HIP, ERR_SHAPE, ERR_INF_IFFT, ERR_INF_MERGED, ERR_ARG, ERR_NOMEM, ERR_NONFINITE, ERR_ROW_NORM = range(9)
BF16, F16, F32 = 0, 1, 2
ADAPTER_LINEAR, ADAPTER_EMBEDDING = 0, 1
BRANCH_NAMES = {0: "add", 1: "arith", 2: "slerp", 3: "carry", 4: "early_v0", 5: "linear"}


class BlendInfo(C.Structure):
    _fields_ = [
        ("cutoff_threshold", C.c_double), ("cull_threshold", C.c_double),
        ("dot", C.c_double), ("s00", C.c_double), ("s01", C.c_double), ("s11", C.c_double),
        ("n_slerp", C.c_uint64),
        ("t", C.c_double), ("cull_pct", C.c_double),
    ]


class AdapterDesc(C.Structure):
    """smhip_adapter_desc"""
    _fields_ = [
        ("base", C.c_void_p), ("dtype", C.c_int), ("rows", C.c_int), ("cols", C.c_int),
        ("lora_a", C.c_void_p), ("lora_b", C.c_void_p), ("factor_dtype", C.c_int), ("rank", C.c_int),
        ("scale", C.c_float), ("layout", C.c_int),
        ("magnitude", C.c_void_p), ("magnitude_dtype", C.c_int),
        ("out", C.c_void_p),
    ]


class LayerDesc(C.Structure):
    _fields_ = [
        ("k", C.c_int),
        ("finetune", C.c_void_p * MAX_MODELS),
        ("base", C.c_void_p * MAX_MODELS),
        ("alpha", C.c_double * MAX_MODELS),
        ("in_dtype", C.c_int),
        ("base_out", C.c_void_p),
        ("base_out_dtype", C.c_int),
        ("rows", C.c_int), ("cols", C.c_int),
        ("target_norm_offset", C.c_double),
        ("cull_start_pct", C.c_double),
        ("cutoff_pct", C.c_double),
        ("t_sum", C.c_double),
        ("b", C.c_double),
        ("norm_mode", C.c_int),
        ("batch", C.c_int),
    ]


# the leading fields that smhip_ties_desc, smhip_dare_desc and smhip_breadcrumbs_desc share
_DELTA_DESC_FIELDS = [
    ("k", C.c_int),
    ("finetune", C.c_void_p * MAX_MODELS),
    ("base", C.c_void_p * MAX_MODELS),
    ("alpha", C.c_double * MAX_MODELS),
    ("in_dtype", C.c_int),
    ("base_out", C.c_void_p), ("base_out_dtype", C.c_int),
    ("n", C.c_size_t),
    ("density", C.c_double), ("lam", C.c_double), ("normalize", C.c_int),
]


class TiesDesc(C.Structure):
    """smhip_ties_desc"""
    _fields_ = _DELTA_DESC_FIELDS


class TiesReport(C.Structure):
    """smhip_ties_report"""
    _fields_ = [("k_keep", C.c_uint64), ("threshold", C.c_float * MAX_MODELS), ("kept", C.c_uint64 * MAX_MODELS)]


class DareDesc(C.Structure):
    """smhip_dare_desc"""
    _fields_ = _DELTA_DESC_FIELDS + [
        ("key", C.c_uint64),
        ("stream_id", C.c_uint32 * MAX_MODELS),
        ("rescale", C.c_int), ("sign_election", C.c_int),
    ]


class DareReport(C.Structure):
    """smhip_dare_report"""
    _fields_ = [("T", C.c_uint32), ("kept", C.c_uint64 * MAX_MODELS)]


class BreadcrumbsDesc(C.Structure):
    """smhip_breadcrumbs_desc"""
    _fields_ = _DELTA_DESC_FIELDS + [
        ("gamma", C.c_double), ("sign_election", C.c_int),
    ]


class BreadcrumbsReport(C.Structure):
    """smhip_breadcrumbs_report"""
    _fields_ = [("k_keep", C.c_uint64), ("n_top", C.c_uint64),
                ("threshold_lo", C.c_float * MAX_MODELS), ("threshold_hi", C.c_float * MAX_MODELS),
                ("kept", C.c_uint64 * MAX_MODELS), ("dropped_top", C.c_uint64 * MAX_MODELS)]


GEO_MODEL_STOCK, GEO_NUSLERP, GEO_SLERP = 0, 1, 2


class GeoDesc(C.Structure):
    """smhip_geo_desc"""
    _fields_ = _DELTA_DESC_FIELDS[:8] + [("mode", C.c_int), ("rowwise", C.c_int), ("rows", C.c_size_t)]


class GeoReport(C.Structure):
    """smhip_geo_report"""
    _fields_ = [("G", (C.c_double * MAX_MODELS) * MAX_MODELS), ("cos", C.c_double), ("t", C.c_double), ("omega", C.c_double),
                ("linear", C.c_int), ("c", C.c_float * MAX_MODELS),
                ("t_min", C.c_double), ("t_max", C.c_double), ("t_mean", C.c_double)]


SPHERE_ACOS, SPHERE_SIN, SPHERE_COS = 0, 1, 2
SPHERE_CONVERGED, SPHERE_LINEAR = 1, 2                # a row's flags


class SphereDesc(C.Structure):
    """smhip_sphere_desc"""
    _fields_ = _DELTA_DESC_FIELDS[:8] + [("weight_space", C.c_int), ("rowwise", C.c_int), ("rows", C.c_size_t),
                                         ("max_iter", C.c_int), ("tol", C.c_double),
                                         ("row_coef", C.c_void_p), ("row_iters", C.c_void_p), ("row_flags", C.c_void_p)]


class SphereReport(C.Structure):
    """smhip_sphere_report"""
    _fields_ = [("G", (C.c_double * MAX_MODELS) * MAX_MODELS), ("H", (C.c_double * MAX_MODELS) * MAX_MODELS),
                ("w", C.c_double * MAX_MODELS), ("a", C.c_double * MAX_MODELS), ("N", C.c_double), ("c", C.c_float * MAX_MODELS),
                ("iterations", C.c_int), ("tau", C.c_double), ("converged", C.c_int), ("linear", C.c_int),
                ("iters_max", C.c_int), ("rows_unconverged", C.c_uint64), ("rows_linear", C.c_uint64),
                ("csum_min", C.c_double), ("csum_max", C.c_double), ("csum_mean", C.c_double)]


class SceDesc(C.Structure):
    """smhip_sce_desc"""
    _fields_ = _DELTA_DESC_FIELDS[:8] + [("select_topk", C.c_double), ("lam", C.c_double)]


class SceReport(C.Structure):
    """smhip_sce_report"""
    _fields_ = [("nz", C.c_uint64), ("k_keep", C.c_uint64), ("selected", C.c_uint64), ("threshold", C.c_float),
                ("energy", C.c_double * MAX_MODELS), ("weight", C.c_float * MAX_MODELS)]


class DellaDesc(C.Structure):
    """smhip_della_desc: smhip_dare_desc, then epsilon and rows"""
    _fields_ = DareDesc._fields_ + [("epsilon", C.c_double), ("rows", C.c_size_t)]


class DellaReport(C.Structure):
    """smhip_della_report"""
    _fields_ = [("T_lo", C.c_uint32), ("T_hi", C.c_uint32), ("kept", C.c_uint64 * MAX_MODELS)]


class ConsensusDesc(C.Structure):
    """smhip_consensus_desc: smhip_ties_desc, then mask_lambda, consensus_k and ties"""
    _fields_ = _DELTA_DESC_FIELDS + [("mask_lambda", C.c_double), ("consensus_k", C.c_int), ("ties", C.c_int)]


class ConsensusReport(C.Structure):
    """smhip_consensus_report"""
    _fields_ = [("k_keep", C.c_uint64), ("threshold", C.c_float * MAX_MODELS), ("kept", C.c_uint64 * MAX_MODELS),
                ("masked", C.c_uint64 * MAX_MODELS), ("agree", C.c_uint64 * (MAX_MODELS + 1)), ("selected", C.c_uint64)]


FUSION_ARCEE, FUSION_NEARSWAP = 0, 1
FUSION_EXP, FUSION_LOG = 0, 1
FUSION_EXP_CUTOFF = -45.0       # sm_exp is +0 below it (csrc/sm_fusion.hpp)


class FusionDesc(C.Structure):
    """smhip_fusion_desc: the leading fields of the delta merges (k must be 1), then mode, rows, iqr_mult, t, kl_out"""
    _fields_ = _DELTA_DESC_FIELDS[:8] + [("mode", C.c_int), ("rows", C.c_size_t), ("iqr_mult", C.c_double), ("t", C.c_double),
                                         ("kl_out", C.c_void_p)]


class FusionReport(C.Structure):
    """smhip_fusion_report"""
    _fields_ = [("q1", C.c_float), ("q2", C.c_float), ("q3", C.c_float), ("threshold", C.c_float),
                ("selected", C.c_uint64), ("clipped", C.c_uint64), ("kl_min", C.c_float), ("kl_max", C.c_float)]


PCB_TANH = 0


class PcbDesc(C.Structure):
    """smhip_pcb_desc: the leading fields of the delta merges, then ratio, clip and lambda"""
    _fields_ = _DELTA_DESC_FIELDS[:8] + [("ratio", C.c_double), ("clip", C.c_double), ("lam", C.c_double)]


class PcbReport(C.Structure):
    """smhip_pcb_report"""
    _fields_ = [("clip_rank", C.c_uint64), ("q", C.c_uint64),
                ("lo", C.c_float * MAX_MODELS), ("hi", C.c_float * MAX_MODELS),
                ("t", C.c_float * MAX_MODELS), ("M", C.c_float * MAX_MODELS),
                ("positive", C.c_uint64 * MAX_MODELS), ("selected", C.c_uint64 * MAX_MODELS),
                ("covered", C.c_uint64), ("contested", C.c_uint64)]


STATS_MAX_DENSITIES = 4         # SMHIP_STATS_MAX_DENSITIES


class StatsDesc(C.Structure):
    """smhip_stats_desc"""
    _fields_ = [("k", C.c_int), ("finetune", C.c_void_p * MAX_MODELS), ("base", C.c_void_p * MAX_MODELS),
                ("alpha", C.c_double * MAX_MODELS), ("in_dtype", C.c_int), ("n", C.c_size_t),
                ("m", C.c_int), ("density", C.c_double * STATS_MAX_DENSITIES)]


class StatsReport(C.Structure):
    """smhip_stats_report"""
    _fields_ = [("nonzero", C.c_uint64 * MAX_MODELS), ("G", (C.c_double * MAX_MODELS) * MAX_MODELS),
                ("k_keep", C.c_uint64 * STATS_MAX_DENSITIES),
                ("tau", (C.c_float * MAX_MODELS) * STATS_MAX_DENSITIES),
                ("kept", (C.c_uint64 * MAX_MODELS) * STATS_MAX_DENSITIES),
                ("energy", (C.c_double * MAX_MODELS) * STATS_MAX_DENSITIES),
                ("opposed", (C.c_uint64 * MAX_MODELS) * STATS_MAX_DENSITIES),
                ("alone", (C.c_uint64 * MAX_MODELS) * STATS_MAX_DENSITIES),
                ("cover", (C.c_uint64 * (MAX_MODELS + 1)) * STATS_MAX_DENSITIES),
                ("conflict", C.c_uint64 * STATS_MAX_DENSITIES)]


EXTRACT_MAX_RANK, EXTRACT_MAX_L, EXTRACT_MAX_ORTH, EXTRACT_MAX_POWER = 256, 272, 9, 4
XL_FILL, XL_DELTA_MM, XL_GRAM, XL_PANEL_MM, XL_SYM_EIG = range(5)


class ExtractDesc(C.Structure):
    """smhip_extract_desc"""
    _fields_ = [("finetune", C.c_void_p), ("base", C.c_void_p), ("in_dtype", C.c_int), ("rows", C.c_int), ("cols", C.c_int),
                ("rank", C.c_int), ("power_iters", C.c_int), ("key", C.c_uint64), ("factor_dtype", C.c_int),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t)]


class ExtractReport(C.Structure):
    """smhip_extract_report"""
    _fields_ = [("L", C.c_int), ("rho", C.c_int), ("n_orth", C.c_int), ("orth_rank", C.c_int * EXTRACT_MAX_ORTH),
                ("sigma", C.c_double * EXTRACT_MAX_L), ("delta_sq", C.c_double), ("share", C.c_double)]


class XlProbeDesc(C.Structure):
    """smhip_xl_probe_desc"""
    _fields_ = [("op", C.c_int), ("finetune", C.c_void_p), ("base", C.c_void_p), ("in_dtype", C.c_int),
                ("rows", C.c_int), ("cols", C.c_int), ("L", C.c_int), ("L2", C.c_int), ("trans", C.c_int),
                ("key", C.c_uint64), ("x", C.c_void_p), ("t", C.c_void_p), ("y", C.c_void_p), ("out_dtype", C.c_int),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t)]


TSV_MAX_R = 256


class WidenDesc(C.Structure):
    """smhip_widen_desc: the leading fields of the delta merges, then rows, ratio, calibration and lambda"""
    _fields_ = _DELTA_DESC_FIELDS[:8] + [("rows", C.c_size_t), ("ratio", C.c_double), ("calibration", C.c_double), ("lam", C.c_double)]


class WidenReport(C.Structure):
    """smhip_widen_report"""
    _fields_ = [("rows", C.c_uint64), ("cols", C.c_uint64), ("vector_mode", C.c_int),
                ("mu", (C.c_double * 2) * MAX_MODELS), ("calibrated", (C.c_uint64 * 2) * MAX_MODELS)]


WIDEN_MAX_COLS = 65536          # C of smhip_widen_merge at most


class CabsDesc(C.Structure):
    """smhip_cabs_desc: the leading fields of the delta merges, then rows, n_keep, group, conflict_aware and lambda"""
    _fields_ = _DELTA_DESC_FIELDS[:8] + [("rows", C.c_size_t), ("n_keep", C.c_int), ("group", C.c_int),
                                         ("conflict_aware", C.c_int), ("lam", C.c_double)]


class CabsReport(C.Structure):
    """smhip_cabs_report"""
    _fields_ = [("groups", C.c_uint64), ("kept", C.c_uint64 * MAX_MODELS), ("short_groups", C.c_uint64 * MAX_MODELS),
                ("surplus", C.c_uint64 * MAX_MODELS), ("covered", C.c_uint64), ("overlap", C.c_uint64)]


CABS_GROUPS = (4, 8, 16, 32, 64, 128, 256, 512)     # group of smhip_cabs_merge: a power of two in 4..512


class TsvDesc(C.Structure):
    """smhip_tsv_desc: the leading fields of the delta merges, then the shape, rank, q, lambda, key and the workspace"""
    _fields_ = _DELTA_DESC_FIELDS[:8] + [("rows", C.c_int), ("cols", C.c_int), ("rank", C.c_int), ("power_iters", C.c_int),
                                         ("lam", C.c_double), ("key", C.c_uint64),
                                         ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t)]


class TsvReport(C.Structure):
    """smhip_tsv_report"""
    _fields_ = [("L", C.c_int), ("r", C.c_int), ("R", C.c_int), ("Rp", C.c_int),
                ("rho", C.c_int * MAX_MODELS), ("n_orth", C.c_int * MAX_MODELS),
                ("orth_rank", (C.c_int * EXTRACT_MAX_ORTH) * MAX_MODELS),
                ("sigma", (C.c_double * TSV_MAX_R) * MAX_MODELS),
                ("delta_sq", C.c_double * MAX_MODELS), ("share", C.c_double * MAX_MODELS),
                ("mu_U", C.c_double * TSV_MAX_R), ("mu_W", C.c_double * TSV_MAX_R),
                ("kept_U", C.c_int), ("kept_W", C.c_int)]


ISO_MAX_S, ISO_MAX_ITER = 16384, 200               # SMHIP_ISO_MAX_S, SMHIP_ISO_MAX_ITER
ISO_NT, ISO_NN = 0, 1                               # form of smhip_iso_gemm
ISO_EP_PLAIN, ISO_EP_POLY, ISO_EP_AXPY, ISO_EP_CUBIC = range(4)


class IsoDesc(C.Structure):
    """smhip_iso_desc: the leading fields of the delta merges, then the shape, lambda, tol, max_iter and the workspace"""
    _fields_ = _DELTA_DESC_FIELDS[:8] + [("rows", C.c_int), ("cols", C.c_int), ("lam", C.c_double), ("tol", C.c_double),
                                         ("max_iter", C.c_int), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t)]


class IsoReport(C.Structure):
    """smhip_iso_report"""
    _fields_ = [("s", C.c_int), ("L", C.c_int), ("transposed", C.c_int),
                ("iterations", C.c_int), ("converged", C.c_int), ("zero", C.c_int),
                ("nu", C.c_double), ("N", C.c_double), ("sigma_bar", C.c_double),
                ("e", C.c_double * (ISO_MAX_ITER + 1)), ("steps", C.c_char * (ISO_MAX_ITER + 4))]


class IsoGemmDesc(C.Structure):
    """smhip_iso_gemm_desc"""
    _fields_ = [("form", C.c_int), ("sym", C.c_int), ("epilogue", C.c_int), ("M", C.c_int), ("N", C.c_int), ("K", C.c_int),
                ("a", C.c_void_p), ("lda", C.c_int), ("b", C.c_void_p), ("ldb", C.c_int), ("e", C.c_void_p), ("lde", C.c_int),
                ("ca", C.c_float), ("cb", C.c_float), ("c", C.c_void_p), ("ldc", C.c_int)]


DPACK_ROW, DPACK_TENSOR = 0, 1                      # scale_mode of smhip_dpack_pack / smhip_dpack_apply
DPACK_SCALE_MODES = {"row": DPACK_ROW, "tensor": DPACK_TENSOR}


class DpackDesc(C.Structure):
    """smhip_dpack_desc"""
    _fields_ = [("finetune", C.c_void_p), ("base", C.c_void_p), ("dtype", C.c_int), ("rows", C.c_size_t), ("cols", C.c_size_t),
                ("bits", C.c_int), ("density", C.c_double), ("scale_mode", C.c_int)]


class DpackReport(C.Structure):
    """smhip_dpack_report"""
    _fields_ = [("rows", C.c_uint64), ("cols", C.c_uint64), ("bits", C.c_int), ("k_keep", C.c_uint64), ("threshold", C.c_float),
                ("kept", C.c_uint64), ("nonzero", C.c_uint64), ("delta_sq", C.c_double), ("resid_sq", C.c_double)]


class EmrDesc(C.Structure):
    """smhip_emr_desc: the leading fields of smhip_ties_desc up to n, then lambda"""
    _fields_ = _DELTA_DESC_FIELDS[:8] + [("lam", C.c_double)]


class EmrReport(C.Structure):
    """smhip_emr_report"""
    _fields_ = [("n", C.c_uint64), ("elected_pos", C.c_uint64), ("elected_neg", C.c_uint64), ("zero", C.c_uint64),
                ("contested", C.c_uint64), ("winner", C.c_uint64 * MAX_MODELS), ("agree", C.c_uint64 * MAX_MODELS)]


class EmrMaskDesc(C.Structure):
    """smhip_emr_mask_desc"""
    _fields_ = [("finetune", C.c_void_p), ("base", C.c_void_p), ("unified", C.c_void_p), ("dtype", C.c_int),
                ("rows", C.c_size_t), ("cols", C.c_size_t)]


class EmrMaskReport(C.Structure):
    """smhip_emr_mask_report"""
    _fields_ = [("rows", C.c_uint64), ("cols", C.c_uint64), ("A", C.c_double), ("B", C.c_double), ("D2", C.c_double),
                ("X", C.c_double), ("U2", C.c_double), ("c", C.c_uint64), ("nonzero", C.c_uint64), ("lam", C.c_float),
                ("delta_sq", C.c_double), ("resid_sq", C.c_double)]


class EmrApplyDesc(C.Structure):
    """smhip_emr_apply_desc"""
    _fields_ = [("base", C.c_void_p), ("unified", C.c_void_p), ("dtype", C.c_int), ("rows", C.c_size_t), ("cols", C.c_size_t),
                ("mask", C.c_void_p), ("scale", C.c_void_p)]


class DpackApplyDesc(C.Structure):
    """smhip_dpack_apply_desc"""
    _fields_ = [("base", C.c_void_p), ("dtype", C.c_int), ("rows", C.c_size_t), ("cols", C.c_size_t),
                ("sign", C.c_void_p), ("mask", C.c_void_p), ("scale", C.c_void_p), ("scale_mode", C.c_int)]


DELLA_MAX_COLS = 32768         # the longest row smhip_della_merge ranks (a row is sorted in LDS)


class LayerReport(C.Structure):
    _fields_ = [
        ("target_norm", C.c_double),
        ("delta_norm", C.c_double * MAX_MODELS),
        ("n_steps", C.c_int),
        ("step_x", C.c_int * MAX_PAIRS), ("step_y", C.c_int * MAX_PAIRS),
        ("step_branch", C.c_int * MAX_PAIRS),
        ("step_info", BlendInfo * MAX_PAIRS),
        ("nan_ifft", C.c_uint32), ("nan_final", C.c_uint32),
        ("merged_delta_norm", C.c_double),
    ]


class SmhipError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"smhip error {code}: {message}")
        self.code = code
        self.message = message


class SmhipLibrary:
    """One loaded shared object exposing the smhip_* C ABI."""

    def __init__(self, path: os.PathLike):
        self.path = str(path)
        self.dll = C.CDLL(self.path)
        d = self.dll
        P, I, D, F = C.c_void_p, C.c_int, C.c_double, C.POINTER(C.c_float)
        d.smhip_version.restype = C.c_char_p
        d.smhip_create.argtypes = [I, C.POINTER(P)]
        d.smhip_destroy.argtypes = [P]
        d.smhip_destroy.restype = None
        d.smhip_last_error.argtypes = [P]
        d.smhip_last_error.restype = C.c_char_p
        d.smhip_reserve.argtypes = [P, I, I]
        d.smhip_workspace_bytes.argtypes = [P]
        d.smhip_workspace_bytes.restype = C.c_size_t
        d.smhip_length_supported.argtypes = [I]
        d.smhip_shape_supported.argtypes = [I, I]
        d.smhip_fft_transform.argtypes = [P, P, I, I, P, P]
        d.smhip_ifft_transform.argtypes = [P, P, I, I, P, P]
        d.smhip_interpolate_fft_components.argtypes = [P, P, P, I, I, D, D, D, D, I, P, C.POINTER(BlendInfo), P]
        d.smhip_arithmetic_fft_components.argtypes = [P, P, P, I, I, D, I, I, P, P]
        d.smhip_merge_tensors_fft2_slerp.argtypes = [P, P, P, I, I, D, D, D, D, D, P, C.POINTER(D), C.POINTER(D),
                                                     C.POINTER(I), C.POINTER(BlendInfo), P]
        d.smhip_task_arithmetic_fft2.argtypes = [P, P, P, I, I, D, I, P, P]
        d.smhip_merge_layer.argtypes = [P, C.POINTER(LayerDesc), P, P, C.POINTER(LayerReport), P]
        d.smhip_addition_merge.argtypes = [P, I, C.POINTER(C.c_void_p), P, I, C.c_size_t, I, P, P]
        d.smhip_ties_merge.argtypes = [P, C.POINTER(TiesDesc), P, P, C.POINTER(TiesReport), P]
        d.smhip_dare_merge.argtypes = [P, C.POINTER(DareDesc), P, P, C.POINTER(DareReport), P]
        d.smhip_breadcrumbs_merge.argtypes = [P, C.POINTER(BreadcrumbsDesc), P, P, C.POINTER(BreadcrumbsReport), P]
        d.smhip_geo_merge.argtypes = [P, C.POINTER(GeoDesc), P, P, C.POINTER(GeoReport), P]
        d.smhip_sphere_merge.argtypes = [P, C.POINTER(SphereDesc), P, P, C.POINTER(SphereReport), P]
        d.smhip_sphere_fn.argtypes = [P, I, P, P, C.c_size_t, I, P]
        d.smhip_sce_merge.argtypes = [P, C.POINTER(SceDesc), P, P, C.POINTER(SceReport), P]
        d.smhip_della_merge.argtypes = [P, C.POINTER(DellaDesc), P, P, P, C.POINTER(DellaReport), P]
        d.smhip_consensus_merge.argtypes = [P, C.POINTER(ConsensusDesc), P, P, C.POINTER(ConsensusReport), P]
        d.smhip_fusion_merge.argtypes = [P, C.POINTER(FusionDesc), P, P, C.POINTER(FusionReport), P]
        d.smhip_fusion_fn.argtypes = [P, I, P, P, C.c_size_t, I, P]
        d.smhip_pcb_merge.argtypes = [P, C.POINTER(PcbDesc), P, P, C.POINTER(PcbReport), P]
        d.smhip_pcb_fn.argtypes = [P, I, P, P, C.c_size_t, I, P]
        d.smhip_delta_stats.argtypes =[P, C.POINTER(StatsDesc), C.POINTER(StatsReport), P]
        d.smhip_correlate_pairs.argtypes = [P, I, C.POINTER(C.c_void_p), I, C.c_size_t, C.c_size_t, C.POINTER(C.c_float), P]
        d.smhip_reference_cpu_norm.argtypes = [P, P, P, I, C.c_size_t, C.POINTER(C.c_float), P]
        d.smhip_slerp.argtypes = [P, P, P, C.c_size_t, C.c_size_t, C.c_float, P, P]
        d.smhip_exact_norm.argtypes = [P, P, I, C.c_size_t, C.POINTER(D), P]
        d.smhip_div_scalar.argtypes = [P, P, I, C.c_size_t, C.c_float, P, P]
        d.smhip_lora_apply.argtypes = [P, P, I, I, I, P, P, I, I, C.c_float, P, P]
        d.smhip_adapter_apply.argtypes = [P, C.POINTER(AdapterDesc), P]
        d.smhip_lora_extract_workspace.argtypes = [I, I, I]
        d.smhip_lora_extract_workspace.restype = C.c_size_t
        d.smhip_lora_extract.argtypes = [P, C.POINTER(ExtractDesc), P, P, C.POINTER(ExtractReport), P]
        d.smhip_xl_probe_workspace.argtypes = [I, I, I]
        d.smhip_xl_probe_workspace.restype = C.c_size_t
        d.smhip_xl_probe.argtypes = [P, C.POINTER(XlProbeDesc), P]
        d.smhip_tsv_workspace.argtypes = [I, I, I, I]
        d.smhip_tsv_workspace.restype = C.c_size_t
        d.smhip_tsv_merge.argtypes = [P, C.POINTER(TsvDesc), P, P, C.POINTER(TsvReport), P]
        d.smhip_tsv_probe.argtypes = [P, P, P, I, I, I, P, I, D, P, P, P]
        d.smhip_widen_merge.argtypes = [P, C.POINTER(WidenDesc), P, P, P, P, P, C.POINTER(WidenReport), P]
        d.smhip_cabs_merge.argtypes = [P, C.POINTER(CabsDesc), P, P, P, C.POINTER(CabsReport), P]
        d.smhip_iso_workspace.argtypes = [I, I]
        d.smhip_iso_workspace.restype = C.c_size_t
        d.smhip_iso_merge.argtypes = [P, C.POINTER(IsoDesc), P, P, C.POINTER(IsoReport), P]
        d.smhip_iso_gemm.argtypes = [P, C.POINTER(IsoGemmDesc), P]
        d.smhip_dpack_pack.argtypes = [P, C.POINTER(DpackDesc), P, P, P, C.POINTER(DpackReport), P]
        d.smhip_dpack_apply.argtypes = [P, C.POINTER(DpackApplyDesc), P, P]
        d.smhip_emr_merge.argtypes = [P, C.POINTER(EmrDesc), P, P, C.POINTER(EmrReport), P]
        d.smhip_emr_mask.argtypes = [P, C.POINTER(EmrMaskDesc), P, P, C.POINTER(EmrMaskReport), P]
        d.smhip_emr_apply.argtypes = [P, C.POINTER(EmrApplyDesc), P, P]
        d.smhip_emr_merge_masks.argtypes = [P, C.POINTER(EmrDesc), C.c_size_t, C.c_size_t, P, P, C.POINTER(C.c_void_p),
                                            C.POINTER(C.c_void_p), C.POINTER(EmrReport), C.POINTER(EmrMaskReport), P]
        d.smhip_debug_option.argtypes =[P, C.c_char_p, C.c_long]
        d.smhip_debug_query.argtypes = [P, C.c_char_p, C.POINTER(C.c_long)]
        d.smhip_profile_enable.argtypes = [P, I]
        d.smhip_profile_reset.argtypes = [P]
        d.smhip_profile_count.argtypes = [P]
        d.smhip_profile_get.argtypes = [P, I, C.POINTER(C.c_char_p), C.POINTER(C.c_uint64), C.POINTER(D)]

    def version(self) -> str:
        return self.dll.smhip_version().decode()

    def length_supported(self, n: int) -> bool:
        return self.dll.smhip_length_supported(int(n)) == OK

    def shape_supported(self, rows: int, cols: int) -> bool:
        """what merge_layer takes: one length planned, the other planned or p * M (include/shardmerge_hip.h)"""
        return self.dll.smhip_shape_supported(int(rows), int(cols)) == OK


class Context:
    """A smhip_ctx: one per device / caller thread.  Owns the device workspace."""

    def __init__(self, lib: SmhipLibrary, device: int = 0):
        self.lib = lib
        self.device = device
        h = C.c_void_p()
        rc = lib.dll.smhip_create(int(device), C.byref(h))
        if rc != OK or not h:
            raise SmhipError(rc, f"smhip_create(device={device}) failed")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.dll.smhip_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc: int):
        if rc != OK:
            raise SmhipError(rc, self.lib.dll.smhip_last_error(self.h).decode())

    def workspace_bytes(self) -> int:
        return int(self.lib.dll.smhip_workspace_bytes(self.h))

    def debug_option(self, key: str, value: int):
        self.check(self.lib.dll.smhip_debug_option(self.h, key.encode(), int(value)))

    def debug_query(self, key: str) -> int:
        out = C.c_long(0)
        self.check(self.lib.dll.smhip_debug_query(self.h, key.encode(), C.byref(out)))
        return int(out.value)

    def profile(self, on: bool):
        self.check(self.lib.dll.smhip_profile_enable(self.h, 1 if on else 0))

    def profile_reset(self):
        self.check(self.lib.dll.smhip_profile_reset(self.h))

    def profile_table(self):
        out = {}
        for i in range(self.lib.dll.smhip_profile_count(self.h)):
            name, n, ms = C.c_char_p(), C.c_uint64(), C.c_double()
            self.check(self.lib.dll.smhip_profile_get(self.h, i, C.byref(name), C.byref(n), C.byref(ms)))
            out[name.value.decode()] = (int(n.value), float(ms.value))
        return out


# SHARDMERGE_HIP_LIB selects another build of the same HIP library (tuning experiments)
_HIP_LIB_PATH = Path(os.environ.get("SHARDMERGE_HIP_LIB") or Path(__file__).resolve().parent / "libshardmerge_hip.so")
_lib: Optional[SmhipLibrary] = None


def hip_library_path() -> Path:
    return _HIP_LIB_PATH


def get_lib() -> SmhipLibrary:
    """The HIP library.  Raises if it has not been built: no fallback exists."""
    global _lib
    if _lib is None:
        if not _HIP_LIB_PATH.exists():
            raise RuntimeError(
                f"{_HIP_LIB_PATH} is missing: build it with `make -C shardmerge_amd/csrc` "
                "(or __graft_entry__.build()); shardmerge_amd has no CPU fallback")
        _lib = SmhipLibrary(_HIP_LIB_PATH)
    return _lib
