"""Engine: torch-tensor front end of the C ABI (include/shardmerge_hip.h).

PyTorch is used here for device memory and streams only: tensors are handed to
the HIP library as raw device pointers (``Tensor.data_ptr()``) together with the
current HIP stream; every transform, order statistic, blend and cast runs in the
hand-written gfx950 kernels behind ``libshardmerge_hip.so``.
"""
from __future__ import annotations

import ctypes as C
import logging
import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib
from .constants import DEFAULT_NORM_MODE, NORM_MODES
from ._lib import BlendInfo, Context, LayerDesc, LayerReport, SmhipError, SmhipLibrary

logger = logging.getLogger(__name__)

_DTYPE_CODE = {torch.bfloat16: _lib.BF16, torch.float16: _lib.F16, torch.float32: _lib.F32}


def _raise_like_reference(e: SmhipError, layer_name: Optional[str] = None):
    """Map C-ABI status codes to the exceptions the reference raises."""
    if e.code == _lib.ERR_INF_IFFT:
        raise ValueError("Inf in ifft output") from e                      # functions.py:217
    if e.code == _lib.ERR_INF_MERGED:
        raise ValueError(f"Inf in merged tensor for {layer_name}") from e  # fast_fourier.py:274
    if e.code == _lib.ERR_SHAPE:
        raise NotImplementedError(e.message) from e
    if e.code == _lib.ERR_NONFINITE:
        # the reference spins forever here (no pair is ever found among NaN norms,
        # fast_fourier.py:171-254); a loud error instead - INTEGRATION.md "deviations"
        raise ValueError(f"Non-finite delta norm in {layer_name}: {e.message}") from e
    raise e


@dataclass
class BlendReport:
    cutoff_threshold: float = 0.0
    cull_threshold: float = 0.0
    dot: float = 0.0
    s00: float = 0.0
    s01: float = 0.0
    s11: float = 0.0
    n_slerp: int = 0
    t: float = 0.0
    cull_pct: float = 0.0

    @classmethod
    def from_c(cls, bi: BlendInfo) -> "BlendReport":
        return cls(bi.cutoff_threshold, bi.cull_threshold, bi.dot, bi.s00, bi.s01, bi.s11, int(bi.n_slerp),
                   bi.t, bi.cull_pct)


@dataclass
class TiesMergeReport:
    k_keep: int = 0                                                  # elements each finetune was trimmed to
    thresholds: List[float] = field(default_factory=list)            # tau_i: the k_keep-th largest |finetune_i - base_i|
    kept: List[int] = field(default_factory=list)                    # elements kept (ties at tau_i included, zeros never)


@dataclass
class DareMergeReport:
    threshold: int = 0                                               # T: an element is kept iff its 16-bit draw is < T
    density: float = 0.0                                             # the effective density T / 65536
    kept: List[int] = field(default_factory=list)                    # elements kept per finetune (zero deltas never)


@dataclass
class DellaMergeReport:
    threshold_lo: int = 0                                            # T of rank 0, the smallest magnitude of a row
    threshold_hi: int = 0                                            # T of rank c - 1
    kept: List[int] = field(default_factory=list)                    # elements kept per finetune (zero deltas never)


@dataclass
class BreadcrumbsMergeReport:
    k_keep: int = 0                                                  # elements each finetune was asked to keep
    n_top: int = 0                                                   # largest magnitudes that may be dropped per finetune
    thresholds_lo: List[float] = field(default_factory=list)         # tau_lo_i: the (n_top + k_keep)-th largest |delta_i|
    thresholds_hi: List[float] = field(default_factory=list)         # tau_hi_i: the (n_top + 1)-th largest |delta_i|
    kept: List[int] = field(default_factory=list)                    # elements kept (ties at either threshold included, zeros never)
    dropped_top: List[int] = field(default_factory=list)             # elements strictly above tau_hi_i (<= n_top)


@dataclass
class GeoMergeReport:
    mode: str = "model_stock"
    rowwise: bool = False
    gram: List[List[float]] = field(default_factory=list)            # whole tensor: G[i][j], the fp64 Gram of the k vectors
    cos: float = 0.0                                                 # model_stock: the mean pairwise cosine; else cos_01
    t: float = 0.0                                                   # model_stock: the interpolation ratio t; else tau
    omega: float = 0.0                                               # nuslerp / slerp: the angle (0 in the linear case)
    linear: bool = False                                             # nuslerp / slerp: the linear case was taken
    coefficients: List[float] = field(default_factory=list)          # whole tensor: c_i (fp32)
    t_min: float = 0.0                                               # row-wise: over the rows' t
    t_max: float = 0.0
    t_mean: float = 0.0


@dataclass
class SphereMergeReport:
    mode: str = "karcher"
    rowwise: bool = False
    max_iter: int = 10
    tol: float = 1e-5
    gram: List[List[float]] = field(default_factory=list)            # whole tensor: G[i][j], the fp64 Gram of the k vectors
    cosines: List[List[float]] = field(default_factory=list)         # whole tensor: H[i][j], the normalised Gram
    weights: List[float] = field(default_factory=list)               # whole tensor: w_i, renormalised over the active vectors
    a: List[float] = field(default_factory=list)                     # whole tensor: the mean direction's coefficients
    length: float = 0.0                                              # whole tensor: N = sum w_i n_i
    coefficients: List[float] = field(default_factory=list)          # whole tensor: c_i (fp32)
    iterations: int = 0                                              # whole tensor: how often tau was evaluated
    tau: float = 0.0                                                 # whole tensor: the last tau
    converged: bool = False
    linear: bool = False                                             # the unit vectors cancel: c_i = w_i
    iters_max: int = 0                                               # row-wise: over the rows
    rows_unconverged: int = 0
    rows_linear: int = 0
    csum_min: float = 0.0                                            # row-wise: over the rows' sum of coefficients
    csum_max: float = 0.0
    csum_mean: float = 0.0
    row_coefficients: Optional[torch.Tensor] = None                  # row-wise: fp32 [R, k] (CPU)
    row_iterations: Optional[torch.Tensor] = None                    # row-wise: int32 [R]
    row_flags: Optional[torch.Tensor] = None                         # row-wise: int32 [R], bit 0 converged, bit 1 linear


@dataclass
class SceMergeReport:
    nz: int = 0                                                      # elements whose variance score q is > 0
    k_keep: int = 0                                                  # floor(select_topk * nz): elements asked for
    selected: int = 0                                                # elements selected (ties at the threshold included)
    threshold: float = 0.0                                           # tau: the k_keep-th largest q (+inf: nothing selected)
    energies: List[float] = field(default_factory=list)              # E_i: the fp64 sum of squares of what finetune i kept
    weights: List[float] = field(default_factory=list)               # w_i (fp32)


@dataclass
class ConsensusMergeReport:
    ties: bool = False                                               # consensus_ties (else consensus_ta)
    k_keep: int = 0                                                  # consensus_ties: as TiesMergeReport; 0 / empty otherwise
    thresholds: List[float] = field(default_factory=list)
    kept: List[int] = field(default_factory=list)
    masked: List[int] = field(default_factory=list)                  # elements where finetune i's TALL mask is set
    agree: List[int] = field(default_factory=list)                   # agree[c], c = 0..k: elements with exactly c masks set
    selected: int = 0                                                # elements with at least min(consensus_k, k) masks set
    n: int = 0                                                       # elements of the tensor (the sum of agree)


@dataclass
class EmrReport:
    n: int = 0                                                       # elements of the tensor
    elected_pos: int = 0                                             # elements whose elected entry is positive
    elected_neg: int = 0                                             # ... negative
    zero: int = 0                                                    # elements with no entry of the elected sign (all deltas zero)
    contested: int = 0                                               # elements with non-zero entries of both signs
    winner: List[int] = field(default_factory=list)                  # elements whose elected entry is finetune i's (the first that attains it)
    agree: List[int] = field(default_factory=list)                   # elements where finetune i's non-zero delta has the elected sign


@dataclass
class EmrMaskReport:
    rows: int = 0                                                    # R: shape[0] (1 for a 0-D or 1-D tensor)
    cols: int = 0                                                    # C: the rest
    A: float = 0.0                                                   # sum |finetune - base| (fp64, ordered, as the rest)
    B: float = 0.0                                                   # sum over the mask of |unified - base|
    D2: float = 0.0                                                  # sum (finetune - base)^2
    X: float = 0.0                                                   # sum over the mask of (finetune - base) (unified - base)
    U2: float = 0.0                                                  # sum over the mask of (unified - base)^2
    c: int = 0                                                       # mask bits set
    nonzero: int = 0                                                 # elements where the finetune differs from its base
    lam: float = 0.0                                                 # fp32(A / B), +0 when B == 0: this tensor's rescaler
    delta_sq: float = 0.0                                            # D2
    resid_sq: float = 0.0                                            # ||finetune - base - lam * mask * (unified - base)||^2


@dataclass
class FusionMergeReport:
    mode: str = "arcee"                                              # "arcee" (arcee_fusion) or "nearswap"
    n: int = 0                                                       # elements of the tensor
    q1: float = 0.0                                                  # arcee: the quartiles of the scores |d| * kappa_row,
    q2: float = 0.0                                                  #   exact order statistics (no interpolation)
    q3: float = 0.0
    threshold: float = 0.0                                           # arcee: fl32(q2 + fl32(iqr_mult * fl32(q3 - q1)))
    selected: int = 0                                                # arcee: elements with a score above the threshold
    kl_min: float = 0.0                                              # arcee: the smallest and the largest row KL
    kl_max: float = 0.0
    kl: Optional[torch.Tensor] = None                                # arcee, want_kl: fp32 [rows], the row KLs
    clipped: int = 0                                                 # nearswap: elements with |d| > t


@dataclass
class PcbMergeReport:
    n: int = 0                                                       # elements of the tensor
    clip_rank: int = 0                                               # r = floor(clip * n): magnitudes clamped at either end
    q: int = 0                                                       # max(1, floor(ratio * n)): scores asked for per finetune
    lo: List[float] = field(default_factory=list)                    # the clip bounds of |tv_i|: exact order statistics
    hi: List[float] = field(default_factory=list)
    t: List[float] = field(default_factory=list)                     # the q-th largest score of finetune i (0: fewer are positive)
    M: List[float] = field(default_factory=list)                     # its largest score
    positive: List[int] = field(default_factory=list)                # entries with a score above 0
    selected: List[int] = field(default_factory=list)                # entries with a score >= t_i and above 0
    covered: int = 0                                                 # elements that some finetune gives a weight above 0
    contested: int = 0                                               # elements that at least two do


@dataclass
class WidenMergeReport:
    rows: int = 0                                                    # R: the first dimension (1 for a 1-D tensor)
    cols: int = 0                                                    # C = n / R
    vector_mode: bool = False                                        # R == 1: one statistic, |delta|, at index 0
    mu: List[List[float]] = field(default_factory=list)              # [finetune][statistic]: the mean significance
    calibrated: List[List[int]] = field(default_factory=list)        # [finetune][statistic]: columns above ratio * mu
    stat: Optional[torch.Tensor] = None                              # want_stats: fp64 [k, 2, C] (m, d; vector mode: a, zeros)
    rank: Optional[torch.Tensor] = None                              # want_stats: int64 [k, 2, C]
    weight: Optional[torch.Tensor] = None                            # want_stats: fp32 [k, C]


@dataclass
class CabsReport:
    n: int = 0                                                       # elements of the tensor
    rows: int = 0                                                    # R: n over the last dimension (1 for a 0-D or 1-D tensor)
    cols: int = 0                                                    # C: the last dimension
    n_keep: int = 0                                                  # N of N:M
    group: int = 0                                                   # M
    conflict_aware: bool = True
    groups: int = 0                                                  # R * ceil(C / M)
    kept: List[int] = field(default_factory=list)                    # [i]: elements finetune i kept
    short_groups: List[int] = field(default_factory=list)            # [i]: groups with fewer candidates than their quota
    surplus: List[int] = field(default_factory=list)                 # [i]: elements kept beyond the quota (ties at the cut)
    covered: int = 0                                                 # elements kept by at least one finetune
    overlap: int = 0                                                 # elements kept by at least two (0 when conflict-aware)
    mask: Optional[torch.Tensor] = None                              # want_mask: int32 [*shape], bit i = finetune i kept it


@dataclass
class DeltaStatsReport:
    n: int = 0                                                       # elements of the tensor
    densities: List[float] = field(default_factory=list)             # rho_q, as given
    nonzero: List[int] = field(default_factory=list)                 # [i]: elements where finetune i differs from its base
    gram: List[List[float]] = field(default_factory=list)            # G[i][j], the fp64 Gram of the k deltas
    k_keep: List[int] = field(default_factory=list)                  # [q]: elements a trim at rho_q asks for
    thresholds: List[List[float]] = field(default_factory=list)      # [q][i]: tau, the k_keep-th largest |delta_i| (+inf: none)
    kept: List[List[int]] = field(default_factory=list)              # [q][i]: entries kept (ties at tau included, zeros never)
    energy: List[List[float]] = field(default_factory=list)          # [q][i]: the fp64 sum of squares of what is kept
    opposed: List[List[int]] = field(default_factory=list)           # [q][i]: kept entries the TIES election would discard
    alone: List[List[int]] = field(default_factory=list)             # [q][i]: kept by finetune i and by no other
    cover: List[List[int]] = field(default_factory=list)             # [q][c], c = 0..k: elements that exactly c finetunes keep
    conflict: List[int] = field(default_factory=list)                # [q]: elements with kept entries of both signs


@dataclass
class DeltaPackReport:
    rows: int = 0                                                    # R: shape[0] (1 for a 0-D or 1-D tensor)
    cols: int = 0                                                    # C: the rest
    bits: int = 1
    density: float = 1.0
    scale: str = "row"
    k_keep: int = 0                                                  # elements the trim asks for (n for bits == 1)
    threshold: float = 0.0                                           # tau (+inf: nothing kept; 0 for bits == 1)
    kept: int = 0                                                    # elements with a sign bit (ties at tau included)
    nonzero: int = 0                                                 # elements where the finetune differs from its base
    delta_sq: float = 0.0                                            # ||finetune - base||^2 (fp64, ordered)
    resid_sq: float = 0.0                                            # ||finetune - base - unpacked||^2 before the rounding of apply

    @property
    def rel_residual(self) -> float:
        """||d - q|| / ||d||, 0 for a zero delta"""
        return math.sqrt(self.resid_sq / self.delta_sq) if self.delta_sq > 0.0 else 0.0


def _shape_rows(t: torch.Tensor) -> Tuple[int, int]:
    """the delta pack's view of a tensor: R = shape[0] rows of the rest; a 0-D or 1-D tensor is one row"""
    if t.ndim <= 1:
        return 1, t.numel()
    return t.shape[0], math.prod(t.shape[1:])


@dataclass
class LoraExtractReport:
    rows: int = 0
    cols: int = 0
    rank: int = 0                                                    # r, as asked for
    power_iters: int = 0
    width: int = 0                                                   # L, the panel width
    effective_rank: int = 0                                          # rho: factor rows / columns from here on are zeros
    orth_ranks: List[int] = field(default_factory=list)              # the rank every orthonormalisation kept
    sigma: List[float] = field(default_factory=list)                 # sigma[0 .. L), the singular values of the projection
    delta_sq: float = 0.0                                            # ||finetune - base||_F^2 (fp64, ordered)
    share: float = 0.0                                               # sum_{i < r} sigma_i^2 / delta_sq

    @property
    def residual_bound(self) -> float:
        """the relative residual ||D - B A||_F / ||D||_F of the exact-arithmetic factors: sqrt(1 - share)"""
        return math.sqrt(max(0.0, 1.0 - self.share))


@dataclass
class TsvReport:
    rows: int = 0
    cols: int = 0
    rank: int = 0                                                    # as asked for
    power_iters: int = 0
    width: int = 0                                                   # L, the panel width of the subspace iterations
    r: int = 0                                                       # min(rank, rows, cols)
    R: int = 0                                                       # singular triplets kept over all finetunes
    Rp: int = 0                                                      # ceil16(R), the width of the panels U, W and B
    rho: List[int] = field(default_factory=list)                     # [i]: triplets finetune i contributes (0: inactive or no delta)
    sigma: List[List[float]] = field(default_factory=list)           # [i][0 .. r): its singular values
    delta_sq: List[float] = field(default_factory=list)              # [i]: ||finetune_i - base_i||_F^2
    share: List[float] = field(default_factory=list)                 # [i]: sum_{j < r} sigma_ij^2 / delta_sq_i
    orth_ranks: List[List[int]] = field(default_factory=list)        # [i]: the rank every orthonormalisation kept
    mu_U: List[float] = field(default_factory=list)                  # [0 .. R): eigenvalues of the Gram of the left vectors
    mu_W: List[float] = field(default_factory=list)                  # ... of the right vectors
    kept_U: int = 0                                                  # eigenvalues above 1e-6 of the largest: directions whitened
    kept_W: int = 0


@dataclass
class IsoReport:
    rows: int = 0
    cols: int = 0
    s: int = 0                                                       # min(rows, cols)
    L: int = 0                                                       # max(rows, cols)
    transposed: bool = False                                         # rows > cols: the iteration ran on the transpose
    nu: float = 0.0                                                  # ||T||_F of the summed delta (fp64, ordered)
    iterations: int = 0                                              # steps taken
    steps: str = ""                                                  # 'q' (quintic) or 'c' (cubic) per step
    e: List[float] = field(default_factory=list)                     # e_0 .. e_iterations: ||X X^T - I||_F / sqrt(s)
    converged: bool = False                                          # the last e is <= tol
    N: float = 0.0                                                   # <Q, T>
    sigma_bar: float = 0.0                                           # N / s: the mean singular value
    zero: bool = False                                               # T == 0: nothing to merge, out = base_out


@dataclass
class LayerMergeReport:
    target_norm: float = 0.0
    delta_norms: List[float] = field(default_factory=list)
    steps: List[Tuple[int, int, str]] = field(default_factory=list)   # (x, y, branch)
    infos: List[BlendReport] = field(default_factory=list)
    nan_ifft: int = 0
    nan_final: int = 0
    merged_delta_norm: float = -1.0

    @property
    def branches(self) -> List[str]:
        return [s[2] for s in self.steps]


def _shape2d(t: torch.Tensor) -> Tuple[int, int]:
    if t.ndim == 1:
        return 1, t.shape[0]
    if t.ndim == 2:
        return t.shape[0], t.shape[1]
    # (merge_layer and the plain transforms take rank > 2 through _shape3d)
    raise NotImplementedError(f"tensor of rank {t.ndim} is not supported by this entry point of the HIP path")


def _shape3d(t: torch.Tensor) -> Tuple[int, int, int]:
    """(batch, rows, cols): the reference transforms the LAST TWO dims of an N-D tensor
    (functions.py:55-58); every leading dim is batch."""
    if t.ndim <= 2:
        r, c = _shape2d(t)
        return 1, r, c
    b = 1
    for d in t.shape[:-2]:
        b *= int(d)
    return b, int(t.shape[-2]), int(t.shape[-1])


class Engine:
    """One smhip context bound to one torch device."""

    def __init__(self, lib: Optional[SmhipLibrary] = None, device: Optional[torch.device] = None):
        if lib is None:
            lib = _lib.get_lib()
            if device is None:
                device = torch.device("cuda", torch.cuda.current_device())
            if device.type != "cuda":
                raise RuntimeError("the HIP library needs a cuda (ROCm) torch device")
        self.lib = lib
        self.device = torch.device(device) if device is not None else torch.device("cpu")
        index = self.device.index if self.device.type == "cuda" and self.device.index is not None else 0
        self.ctx = Context(lib, index)

    # -- plumbing ---------------------------------------------------------------
    def _stream(self) -> Optional[int]:
        if self.device.type == "cuda":
            return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        return None

    def _dev(self, t: torch.Tensor, dtype: Optional[torch.dtype] = None) -> torch.Tensor:
        if dtype is not None and t.dtype != dtype:
            t = t.to(dtype)
        if t.device != self.device:
            t = t.to(self.device)
        return t.contiguous()

    def _call(self, rc: int, layer_name: Optional[str] = None):
        try:
            self.ctx.check(rc)
        except SmhipError as e:
            _raise_like_reference(e, layer_name)

    # -- A4 / A8 -----------------------------------------------------------------
    def fft_transform(self, x: torch.Tensor) -> torch.Tensor:
        x = self._dev(x, torch.float32)
        b, r, c = _shape3d(x)
        out = torch.empty(x.shape + (2,), dtype=torch.float32, device=self.device)
        xs, os_ = x.reshape(b, -1), out.reshape(b, -1)
        for i in range(b):                        # slices of a rank > 2 tensor are independent transforms
            self._call(self.lib.dll.smhip_fft_transform(self.ctx.h, xs[i].data_ptr(), r, c, os_[i].data_ptr(), self._stream()))
        return torch.view_as_complex(out)

    def ifft_transform(self, spec: torch.Tensor) -> torch.Tensor:
        spec = self._dev(spec, torch.complex64)
        b, r, c = _shape3d(spec)
        sr = torch.view_as_real(spec)
        out = torch.empty(spec.shape, dtype=torch.float32, device=self.device)
        ss, os_ = sr.reshape(b, -1), out.reshape(b, -1)
        for i in range(b):
            self._call(self.lib.dll.smhip_ifft_transform(self.ctx.h, ss[i].data_ptr(), r, c, os_[i].data_ptr(), self._stream()))
        return out

    # -- A5 - A7 -------------------------------------------------------------------
    def interpolate_fft_components(self, f0, f1, t, t_sum=1.0, cutoff_pct=0.0, cull_pct=0.0, interp_imag=True):
        f0 = self._dev(f0, torch.complex64)
        f1 = self._dev(f1, torch.complex64)
        r, c = _shape2d(f0)
        out = torch.empty(f0.shape + (2,), dtype=torch.float32, device=self.device)
        info = BlendInfo()
        self._call(self.lib.dll.smhip_interpolate_fft_components(
            self.ctx.h, torch.view_as_real(f0).data_ptr(), torch.view_as_real(f1).data_ptr(), r, c,
            float(t), float(t_sum), float(cutoff_pct), float(cull_pct), 1 if interp_imag else 0,
            out.data_ptr(), C.byref(info), self._stream()))
        return torch.view_as_complex(out), BlendReport.from_c(info)

    def arithmetic_fft_components(self, f0, f1, t, agreement=True, do_imag=True):
        f0 = self._dev(f0, torch.complex64)
        f1 = self._dev(f1, torch.complex64)
        r, c = _shape2d(f0)
        out = torch.empty(f0.shape + (2,), dtype=torch.float32, device=self.device)
        self._call(self.lib.dll.smhip_arithmetic_fft_components(
            self.ctx.h, torch.view_as_real(f0).data_ptr(), torch.view_as_real(f1).data_ptr(), r, c,
            float(t), 1 if agreement else 0, 1 if do_imag else 0, out.data_ptr(), self._stream()))
        return torch.view_as_complex(out)

    # -- A9 / A10 ------------------------------------------------------------------
    def merge_tensors_fft2_slerp(self, v0, v1, t, b=0.1, t_sum=1.0, cutoff_pct=0.0, cull_pct=0.0):
        v0 = self._dev(v0, torch.float32)
        v1 = self._dev(v1, torch.float32)
        r, c = _shape2d(v0)
        out = torch.empty_like(v0)
        n0, n1, br = C.c_double(), C.c_double(), C.c_int()
        info = BlendInfo()
        self._call(self.lib.dll.smhip_merge_tensors_fft2_slerp(
            self.ctx.h, v0.data_ptr(), v1.data_ptr(), r, c, float(t), float(b), float(t_sum), float(cutoff_pct),
            float(cull_pct), out.data_ptr(), C.byref(n0), C.byref(n1), C.byref(br), C.byref(info), self._stream()))
        rep = BlendReport.from_c(info)
        rep.branch = _lib.BRANCH_NAMES.get(br.value, str(br.value))
        return out, n0.value, n1.value, rep

    def task_arithmetic_fft2(self, v0, v1, t, agreement=True):
        v0 = self._dev(v0, torch.float32)
        v1 = self._dev(v1, torch.float32)
        r, c = _shape2d(v0)
        out = torch.empty_like(v0)
        self._call(self.lib.dll.smhip_task_arithmetic_fft2(
            self.ctx.h, v0.data_ptr(), v1.data_ptr(), r, c, float(t), 1 if agreement else 0, out.data_ptr(), self._stream()))
        return out

    # -- torch.norm as ATen's CPU kernel computes it (norm_mode = reference_cpu) -----------------
    def reference_cpu_norm(self, x: torch.Tensor, base: Optional[torch.Tensor] = None) -> float:
        """``torch.norm(x - base)`` exactly as the reference's ``device="cpu"`` run gets it for a contiguous
        fp32 tensor (functions.py:85, fast_fourier.py:152,209-210): bit-identical, computed in parallel."""
        dtype = x.dtype if x.dtype in _DTYPE_CODE and (base is None or base.dtype == x.dtype) else torch.float32
        xs = self._dev(x, dtype)
        bs = self._dev(base, dtype) if base is not None else None
        if bs is not None and bs.shape != xs.shape:
            raise ValueError(f"shape mismatch: {tuple(xs.shape)} vs {tuple(bs.shape)}")
        out = C.c_float(0.0)
        self._call(self.lib.dll.smhip_reference_cpu_norm(self.ctx.h, xs.data_ptr(), bs.data_ptr() if bs is not None else None,
                                                         _DTYPE_CODE[dtype], xs.numel(), C.byref(out), self._stream()))
        return float(out.value)

    # -- A1 / A8 at function level ----------------------------------------------------------------
    def slerp(self, v0: torch.Tensor, v1: torch.Tensor, t: float) -> torch.Tensor:
        """reference functions.py:24-43 (quirk Q5 kept); the relative vector is normalised along the last dimension."""
        if v0.shape != v1.shape:
            raise ValueError(f"shape mismatch: {tuple(v0.shape)} vs {tuple(v1.shape)}")
        a, b = self._dev(v0, torch.float32), self._dev(v1, torch.float32)
        out = torch.empty_like(a)
        cols = a.shape[-1] if a.dim() >= 1 else 1
        rows = a.numel() // cols if cols else 0
        self._call(self.lib.dll.smhip_slerp(self.ctx.h, a.data_ptr(), b.data_ptr(), rows, cols if a.numel() else 0, float(t),
                                            out.data_ptr(), self._stream()))
        return out

    def exact_norm(self, x: torch.Tensor) -> float:
        """||x||_2, accumulated in fp64 on the device"""
        dtype = x.dtype if x.dtype in _DTYPE_CODE else torch.float32
        xs = self._dev(x, dtype)
        out = C.c_double(0.0)
        self._call(self.lib.dll.smhip_exact_norm(self.ctx.h, xs.data_ptr(), _DTYPE_CODE[dtype], xs.numel(), C.byref(out), self._stream()))
        return float(out.value)

    def div_scalar(self, x: torch.Tensor, s: float) -> torch.Tensor:
        """``x / s`` in x's dtype, as torch divides a tensor by a Python float (fp32 division, one rounding)"""
        dtype = x.dtype if x.dtype in _DTYPE_CODE else torch.float32
        xs = self._dev(x, dtype)
        out = torch.empty_like(xs)
        self._call(self.lib.dll.smhip_div_scalar(self.ctx.h, xs.data_ptr(), _DTYPE_CODE[dtype], xs.numel(), float(s), out.data_ptr(), self._stream()))
        return out

    def normalize_tensor(self, x: torch.Tensor, norm_mode: Optional[str] = None):
        """reference functions.py:75-88: (x / norm, norm), norm = ``x.norm().item()`` - in ``reference_cpu`` mode the value
        the reference's CPU run gets (ATen's biased fp32 kernel; a 16-bit tensor's norm is rounded to its dtype), else
        the exact one.  norm == 0: x comes back unchanged."""
        mode = DEFAULT_NORM_MODE if norm_mode is None else norm_mode
        if mode not in NORM_MODES:
            raise ValueError(f"norm_mode {mode!r}: one of {NORM_MODES}")
        if mode == "reference_cpu":
            norm = self.reference_cpu_norm(x)
            if x.dtype in (torch.bfloat16, torch.float16):
                norm = float(torch.tensor(norm, dtype=torch.float32).to(x.dtype))
        else:
            norm = self.exact_norm(x)
        return (self.div_scalar(x, norm) if norm != 0 else self._dev(x, x.dtype if x.dtype in _DTYPE_CODE else torch.float32)), norm

    # -- LoRA adapters ---------------------------------------------------------------------
    def lora_apply(self, base: torch.Tensor, a: torch.Tensor, b: torch.Tensor, scale: float, *,
                   magnitude: Optional[torch.Tensor] = None, embedding: bool = False) -> torch.Tensor:
        """the finetune weight a LoRA adapter defines: ``base + scale * (b @ a)`` accumulated in fp32 and rounded once
        into base's dtype (``smhip_lora_apply``).  base [out, in], a = lora_A [r, in], b = lora_B [out, r].
        embedding: a = lora_embedding_A [r, num_embeddings], b = lora_embedding_B [dim, r] of base [num_embeddings,
        dim], ``base + scale * (a.T @ b.T)``.  magnitude [out] (DoRA, Linear only): each row of that sum scaled by
        ``magnitude / ||row||`` before the one rounding; a zero or non-finite row norm or magnitude raises SmhipError
        ERR_ROW_NORM naming the row (``smhip_adapter_apply``)."""
        if magnitude is None and not embedding:
            rows, cols, rank, bs, av, bv, fdtype = self._adapter_args(base, a, b, False)
            out = torch.empty_like(bs)
            self._call(self.lib.dll.smhip_lora_apply(self.ctx.h, bs.data_ptr(), _DTYPE_CODE[bs.dtype], rows, cols,
                                                     av.data_ptr(), bv.data_ptr(), _DTYPE_CODE[fdtype], rank,
                                                     float(scale), out.data_ptr(), self._stream()))
            return out
        return self.adapter_apply(base, a, b, scale, magnitude=magnitude, embedding=embedding)

    def adapter_apply(self, base: torch.Tensor, a: torch.Tensor, b: torch.Tensor, scale: float, *,
                      magnitude: Optional[torch.Tensor] = None, embedding: bool = False) -> torch.Tensor:
        """``lora_apply`` through the descriptor entry point ``smhip_adapter_apply`` (also with neither keyword)"""
        rows, cols, rank, bs, av, bv, fdtype = self._adapter_args(base, a, b, embedding)
        mv = None
        if magnitude is not None:
            if embedding:
                raise ValueError("lora_apply: DoRA (a magnitude) applies to Linear modules only, not embeddings")
            if magnitude.ndim != 1 or magnitude.shape[0] != rows:
                raise ValueError(f"lora_apply: magnitude {list(magnitude.shape)} does not match base {list(base.shape)}")
            if magnitude.dtype not in _DTYPE_CODE:
                raise ValueError(f"lora_apply: magnitude is {magnitude.dtype}; bf16, f16 or f32 expected")
            mv = self._dev(magnitude).contiguous()
        out = torch.empty_like(bs)
        d = _lib.AdapterDesc(bs.data_ptr(), _DTYPE_CODE[bs.dtype], rows, cols, av.data_ptr(), bv.data_ptr(),
                             _DTYPE_CODE[fdtype], rank, float(scale),
                             _lib.ADAPTER_EMBEDDING if embedding else _lib.ADAPTER_LINEAR,
                             mv.data_ptr() if mv is not None else None, _DTYPE_CODE[mv.dtype] if mv is not None else _lib.F32,
                             out.data_ptr())
        self._call(self.lib.dll.smhip_adapter_apply(self.ctx.h, C.byref(d), self._stream()))
        return out

    def _adapter_args(self, base, a, b, embedding: bool):
        if base.ndim != 2 or a.ndim != 2 or b.ndim != 2:
            raise ValueError(f"lora_apply: 2-D tensors expected, got base {list(base.shape)}, a {list(a.shape)}, b {list(b.shape)}")
        rows, cols = base.shape
        rank = a.shape[0]
        want_a, want_b = ((rank, rows), (cols, rank)) if embedding else ((rank, cols), (rows, rank))
        if tuple(a.shape) != want_a or tuple(b.shape) != want_b:
            what = "lora_embedding_A / lora_embedding_B" if embedding else "lora_A / lora_B"
            raise ValueError(f"lora_apply: base {list(base.shape)} does not match {what} {list(a.shape)} / {list(b.shape)}")
        for name, t in (("base", base), ("lora_A", a), ("lora_B", b)):
            if t.dtype not in _DTYPE_CODE:
                raise ValueError(f"lora_apply: {name} is {t.dtype}; bf16, f16 or f32 expected")
        fdtype = a.dtype if a.dtype == b.dtype else torch.promote_types(a.dtype, b.dtype)
        bs = self._dev(base).contiguous()
        av, bv = self._dev(a, fdtype).contiguous(), self._dev(b, fdtype).contiguous()
        return rows, cols, rank, bs, av, bv, fdtype

    # -- the delta pack ----------------------------------------------------------------------
    def delta_pack(self, finetune: torch.Tensor, base: torch.Tensor, *, bits: int = 1, density: float = 1.0,
                   scale: str = "row", name: str = ""):
        """One tensor's delta ``finetune - base`` as bit planes and scales (``smhip_dpack_pack``; the function is stated
        in include/shardmerge_hip.h).  bits = 1: the sign of every delta; bits = 2: a mask of its ``density`` largest
        magnitudes (the trim of ``ties_merge``, ties kept) and their signs.  scale: "row", the mean kept magnitude of
        each row of ``shape[0]``, or "tensor", one for all.  Returns ``(sign, mask | None, scale, DeltaPackReport)``:
        uint8 planes [R, ceil(C / 8)] and a float32 [R] or [1].  A NaN or Inf in the delta raises ValueError naming
        ``name``."""
        if isinstance(bits, bool) or not isinstance(bits, int) or bits not in (1, 2):
            raise ValueError(f"delta_pack: bits must be 1 or 2, not {bits!r}")
        if isinstance(density, bool) or not isinstance(density, (int, float)) or not (0.0 < float(density) <= 1.0):
            raise ValueError(f"delta_pack: density {density!r} is not in (0, 1]")
        if bits == 1 and float(density) != 1.0:
            raise ValueError(f"delta_pack: bits = 1 keeps every sign, density must be 1, not {density!r}")
        if scale not in _lib.DPACK_SCALE_MODES:
            raise ValueError(f"delta_pack: scale must be 'row' or 'tensor', not {scale!r}")
        if finetune.shape != base.shape:
            raise ValueError(f"delta_pack: shape mismatch in {name or 'tensor'}: {list(finetune.shape)} / {list(base.shape)}")
        in_dtype = finetune.dtype if finetune.dtype == base.dtype and finetune.dtype in _DTYPE_CODE else torch.float32
        ft, bs = self._dev(finetune, in_dtype), self._dev(base, in_dtype)
        rows, cols = _shape_rows(ft)
        pb = (cols + 7) // 8
        sign = torch.empty((rows, pb), dtype=torch.uint8, device=self.device)
        mask = torch.empty((rows, pb), dtype=torch.uint8, device=self.device) if bits == 2 else None
        sc = torch.empty((rows if scale == "row" else 1,), dtype=torch.float32, device=self.device)
        desc = _lib.DpackDesc(ft.data_ptr(), bs.data_ptr(), _DTYPE_CODE[in_dtype], rows, cols, bits, float(density),
                              _lib.DPACK_SCALE_MODES[scale])
        rep = _lib.DpackReport()
        try:
            self.ctx.check(self.lib.dll.smhip_dpack_pack(self.ctx.h, C.byref(desc), sign.data_ptr(),
                                                         mask.data_ptr() if mask is not None else None, sc.data_ptr(),
                                                         C.byref(rep), self._stream()))
        except SmhipError as e:
            if e.code == _lib.ERR_NONFINITE:
                raise ValueError(f"Non-finite delta in {name or 'tensor'}: {e.message}") from e
            raise
        return sign, mask, sc, DeltaPackReport(rows=rows, cols=cols, bits=bits, density=float(density), scale=scale,
                                               k_keep=int(rep.k_keep), threshold=float(rep.threshold), kept=int(rep.kept),
                                               nonzero=int(rep.nonzero), delta_sq=float(rep.delta_sq),
                                               resid_sq=float(rep.resid_sq))

    def delta_apply(self, base: torch.Tensor, sign: torch.Tensor, mask: Optional[torch.Tensor], scale: torch.Tensor) -> torch.Tensor:
        """the finetune tensor a delta pack defines: ``base + s`` or ``base - s`` where an element is kept, one fp32
        addition rounded once into base's dtype, and ``base`` bit for bit elsewhere (``smhip_dpack_apply``).  mask None:
        a 1-bit pack, every element is kept.  scale: float32 [R] (per row) or [1] (per tensor)."""
        if base.dtype not in _DTYPE_CODE:
            raise ValueError(f"delta_apply: base is {base.dtype}; bf16, f16 or f32 expected")
        rows, cols = _shape_rows(base)
        pb = (cols + 7) // 8
        for what, t in (("sign", sign), ("mask", mask)):
            if t is None:
                continue
            if t.dtype != torch.uint8 or tuple(t.shape) != (rows, pb):
                raise ValueError(f"delta_apply: {what} is {t.dtype} {list(t.shape)}; uint8 [{rows}, {pb}] expected for base {list(base.shape)}")
        if scale.dtype != torch.float32 or scale.ndim != 1 or scale.shape[0] not in (1, rows):
            raise ValueError(f"delta_apply: scale is {scale.dtype} {list(scale.shape)}; float32 [{rows}] or [1] expected")
        mode = _lib.DPACK_ROW if scale.shape[0] == rows else _lib.DPACK_TENSOR
        bs, sg, sc = self._dev(base), self._dev(sign), self._dev(scale)
        mk = self._dev(mask) if mask is not None else None
        out = torch.empty_like(bs)
        desc = _lib.DpackApplyDesc(bs.data_ptr(), _DTYPE_CODE[bs.dtype], rows, cols, sg.data_ptr(),
                                   mk.data_ptr() if mk is not None else None, sc.data_ptr(), mode)
        self._call(self.lib.dll.smhip_dpack_apply(self.ctx.h, C.byref(desc), out.data_ptr(), self._stream()))
        return out

    # -- EMR-Merging: the unified model, a task's mask and rescaler, the task's tensor --------------
    def emr_merge(self, finetunes: Sequence[torch.Tensor], bases: Sequence[torch.Tensor], base_out: torch.Tensor, *,
                  lam: float = 1.0, want_delta: bool = False, layer_name: str = ""):
        """The unified model of EMR-Merging for one tensor of any shape (``smhip_emr_merge``; the function is stated in
        include/shardmerge_hip.h): per element the deltas ``finetune_i - base_i`` are summed in order, the sign of the
        sum is elected (zero elects plus), and the entry of that sign with the largest magnitude is taken as it is,
        times ``lam``, added onto ``base_out`` in its dtype.  The method has no weights.  Returns (out, EmrReport[, the
        fp32 merged delta]).  A NaN or Inf in a delta or in the sum raises ValueError naming ``layer_name``."""
        layer_name = layer_name or "layer"
        if isinstance(lam, bool) or not isinstance(lam, (int, float)) or not math.isfinite(float(lam)):
            raise ValueError(f"emr_merge: lam {lam!r} is not a finite number")
        desc, rep, k = _lib.EmrDesc(), _lib.EmrReport(), len(finetunes)
        desc.lam = float(lam)
        keep, bo, out, delta = self._stage_delta_merge(desc, finetunes, bases, [1.0] * len(bases), base_out, layer_name,
                                                       want_delta, "emr_merge")
        desc.n = bo.numel()
        self._run_delta_merge(self.lib.dll.smhip_emr_merge, desc, rep, out, delta, layer_name)
        report = EmrReport(n=int(rep.n), elected_pos=int(rep.elected_pos), elected_neg=int(rep.elected_neg), zero=int(rep.zero),
                           contested=int(rep.contested), winner=[int(rep.winner[i]) for i in range(k)],
                           agree=[int(rep.agree[i]) for i in range(k)])
        return (out, report, delta) if want_delta else (out, report)

    def emr_mask(self, finetune: torch.Tensor, base: torch.Tensor, unified: torch.Tensor, *, name: str = ""):
        """One task's modulator for one tensor (``smhip_emr_mask``): the mask of the elements where ``finetune - base``
        and ``unified - base`` have the same sign, bit-packed as the delta pack's planes (uint8 [R, ceil(C / 8)]), and
        the rescaler ``sum |finetune - base| / sum over the mask of |unified - base|`` as a float32 [1].  Returns
        ``(mask, scale, EmrMaskReport)``; the report holds the ordered fp64 sums, from which a caller forms one rescaler
        for a whole model.  A NaN or Inf in either delta raises ValueError naming ``name``."""
        if not (finetune.shape == base.shape == unified.shape):
            raise ValueError(f"emr_mask: shape mismatch in {name or 'tensor'}: {list(finetune.shape)} / {list(base.shape)} / "
                             f"{list(unified.shape)}")
        dtypes = {finetune.dtype, base.dtype, unified.dtype}
        in_dtype = finetune.dtype if len(dtypes) == 1 and finetune.dtype in _DTYPE_CODE else torch.float32
        ft, bs, un = self._dev(finetune, in_dtype), self._dev(base, in_dtype), self._dev(unified, in_dtype)
        rows, cols = _shape_rows(ft)
        mask = torch.empty((rows, (cols + 7) // 8), dtype=torch.uint8, device=self.device)
        sc = torch.empty((1,), dtype=torch.float32, device=self.device)
        desc = _lib.EmrMaskDesc(ft.data_ptr(), bs.data_ptr(), un.data_ptr(), _DTYPE_CODE[in_dtype], rows, cols)
        rep = _lib.EmrMaskReport()
        try:
            self.ctx.check(self.lib.dll.smhip_emr_mask(self.ctx.h, C.byref(desc), mask.data_ptr(), sc.data_ptr(),
                                                       C.byref(rep), self._stream()))
        except SmhipError as e:
            if e.code == _lib.ERR_NONFINITE:
                raise ValueError(f"Non-finite delta in {name or 'tensor'}: {e.message}") from e
            raise
        return mask, sc, EmrMaskReport(rows=rows, cols=cols, A=float(rep.A), B=float(rep.B), D2=float(rep.D2), X=float(rep.X),
                                       U2=float(rep.U2), c=int(rep.c), nonzero=int(rep.nonzero), lam=float(rep.lam),
                                       delta_sq=float(rep.delta_sq), resid_sq=float(rep.resid_sq))

    def emr_merge_masks(self, finetunes: Sequence[torch.Tensor], bases: Sequence[torch.Tensor], base_out: torch.Tensor, *,
                        lam: float = 1.0, want_delta: bool = False, layer_name: str = ""):
        """The unified tensor AND every entry's modulator from one fused pass (``smhip_emr_merge_masks``): what
        ``emr_merge`` followed by ``emr_mask(finetunes[i], bases[i], out)`` for every i returns, bit for bit, while the
        finetunes and the bases are read once.  Returns ``(out, EmrReport, masks, scales, mask_reports[, delta])``:
        ``masks`` k uint8 [R, ceil(C / 8)] tensors, ``scales`` k float32 [1] tensors, ``mask_reports`` k EmrMaskReport.
        A NaN or Inf in a delta, in the sum or in ``out - base_i`` raises ValueError naming ``layer_name`` and, where
        there is one, the entry."""
        layer_name = layer_name or "layer"
        if isinstance(lam, bool) or not isinstance(lam, (int, float)) or not math.isfinite(float(lam)):
            raise ValueError(f"emr_merge_masks: lam {lam!r} is not a finite number")
        desc, rep, k = _lib.EmrDesc(), _lib.EmrReport(), len(finetunes)
        desc.lam = float(lam)
        keep, bo, out, delta = self._stage_delta_merge(desc, finetunes, bases, [1.0] * len(bases), base_out, layer_name,
                                                       want_delta, "emr_merge_masks")
        desc.n = bo.numel()
        rows, cols = _shape_rows(bo)
        pb = (cols + 7) // 8
        planes = torch.empty((k, rows, pb), dtype=torch.uint8, device=self.device)
        sc = torch.empty((k,), dtype=torch.float32, device=self.device)
        masks, scales = [planes[i] for i in range(k)], [sc[i:i + 1] for i in range(k)]
        mptr = (C.c_void_p * k)(*[m.data_ptr() for m in masks])
        sptr = (C.c_void_p * k)(*[s.data_ptr() for s in scales])
        mreps = (_lib.EmrMaskReport * k)()
        try:
            self.ctx.check(self.lib.dll.smhip_emr_merge_masks(
                self.ctx.h, C.byref(desc), rows, cols, out.data_ptr(), delta.data_ptr() if delta is not None else None,
                mptr, sptr, C.byref(rep), mreps, self._stream()))
        except SmhipError as e:
            if e.code == _lib.ERR_NONFINITE:
                raise ValueError(f"Non-finite delta in {layer_name}: {e.message}") from e
            raise
        report = EmrReport(n=int(rep.n), elected_pos=int(rep.elected_pos), elected_neg=int(rep.elected_neg), zero=int(rep.zero),
                           contested=int(rep.contested), winner=[int(rep.winner[i]) for i in range(k)],
                           agree=[int(rep.agree[i]) for i in range(k)])
        mask_reports = [EmrMaskReport(rows=rows, cols=cols, A=float(q.A), B=float(q.B), D2=float(q.D2), X=float(q.X),
                                      U2=float(q.U2), c=int(q.c), nonzero=int(q.nonzero), lam=float(q.lam),
                                      delta_sq=float(q.delta_sq), resid_sq=float(q.resid_sq)) for q in mreps]
        res = (out, report, masks, scales, mask_reports)
        return res + (delta,) if want_delta else res

    def emr_apply(self, base: torch.Tensor, unified: torch.Tensor, mask: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
        """the task tensor an EMR modulator defines: ``base + scale * (unified - base)`` where the mask bit is set, one
        rounding per operation and once into base's dtype, and ``base`` bit for bit elsewhere (``smhip_emr_apply``).
        mask: uint8 [R, ceil(C / 8)]; scale: float32 [1]."""
        if base.dtype not in _DTYPE_CODE:
            raise ValueError(f"emr_apply: base is {base.dtype}; bf16, f16 or f32 expected")
        if unified.dtype != base.dtype or unified.shape != base.shape:
            raise ValueError(f"emr_apply: unified is {unified.dtype} {list(unified.shape)}; {base.dtype} {list(base.shape)} expected")
        rows, cols = _shape_rows(base)
        pb = (cols + 7) // 8
        if mask.dtype != torch.uint8 or tuple(mask.shape) != (rows, pb):
            raise ValueError(f"emr_apply: mask is {mask.dtype} {list(mask.shape)}; uint8 [{rows}, {pb}] expected for base {list(base.shape)}")
        if scale.dtype != torch.float32 or tuple(scale.shape) != (1,):
            raise ValueError(f"emr_apply: scale is {scale.dtype} {list(scale.shape)}; float32 [1] expected")
        bs, un, mk, sc = self._dev(base), self._dev(unified), self._dev(mask), self._dev(scale)
        out = torch.empty_like(bs)
        desc = _lib.EmrApplyDesc(bs.data_ptr(), un.data_ptr(), _DTYPE_CODE[bs.dtype], rows, cols, mk.data_ptr(), sc.data_ptr())
        self._call(self.lib.dll.smhip_emr_apply(self.ctx.h, C.byref(desc), out.data_ptr(), self._stream()))
        return out

    # -- extract-lora ------------------------------------------------------------------------
    def lora_extract(self, finetune: torch.Tensor, base: torch.Tensor, rank: int, *, power_iters: int = 2,
                     factor_dtype: Optional[torch.dtype] = None, seed: int = 0, name: str = ""):
        """A rank-``rank`` adapter of one 2-D tensor: ``(A [rank, cols], B [rows, rank], LoraExtractReport)`` with
        ``B @ A`` the randomized rank-``rank`` approximation of ``finetune - base`` (``smhip_lora_extract``; the function
        is stated in include/shardmerge_hip.h), ``lora_alpha = rank``.  The sketch is keyed as the DARE mask is: the
        first 8 bytes of ``sha256(f"{seed}\\n{name}")``.  factor_dtype: of A and B, default the inputs' dtype.  A NaN or
        Inf in the delta raises ValueError naming ``name``."""
        import hashlib
        if finetune.ndim != 2 or finetune.shape != base.shape:
            raise ValueError(f"lora_extract: two 2-D tensors of one shape expected, got {list(finetune.shape)} / {list(base.shape)}")
        if isinstance(rank, bool) or not isinstance(rank, int) or not (1 <= rank <= _lib.EXTRACT_MAX_RANK):
            raise ValueError(f"lora_extract: rank must be an integer in 1..{_lib.EXTRACT_MAX_RANK}, not {rank!r}")
        if isinstance(power_iters, bool) or not isinstance(power_iters, int) or not (0 <= power_iters <= _lib.EXTRACT_MAX_POWER):
            raise ValueError(f"lora_extract: power_iters must be an integer in 0..{_lib.EXTRACT_MAX_POWER}, not {power_iters!r}")
        in_dtype = finetune.dtype if finetune.dtype == base.dtype and finetune.dtype in _DTYPE_CODE else torch.float32
        factor_dtype = factor_dtype or in_dtype
        if factor_dtype not in _DTYPE_CODE:
            raise ValueError(f"lora_extract: factor dtype {factor_dtype}; bf16, f16 or f32 expected")
        ft, bs = self._dev(finetune, in_dtype), self._dev(base, in_dtype)
        rows, cols = ft.shape
        a = torch.empty((rank, cols), dtype=factor_dtype, device=self.device)
        b = torch.empty((rows, rank), dtype=factor_dtype, device=self.device)
        ws = self._xl_workspace(int(self.lib.dll.smhip_lora_extract_workspace(rows, cols, rank)))
        key = int.from_bytes(hashlib.sha256(f"{seed}\n{name}".encode()).digest()[:8], "little")
        desc = _lib.ExtractDesc(ft.data_ptr(), bs.data_ptr(), _DTYPE_CODE[in_dtype], rows, cols, rank, power_iters, key,
                                _DTYPE_CODE[factor_dtype], ws.data_ptr(), ws.numel())
        rep = _lib.ExtractReport()
        self._call(self.lib.dll.smhip_lora_extract(self.ctx.h, C.byref(desc), a.data_ptr(), b.data_ptr(), C.byref(rep),
                                                   self._stream()), name or "tensor")
        return a, b, LoraExtractReport(rows=rows, cols=cols, rank=rank, power_iters=power_iters, width=int(rep.L),
                                       effective_rank=int(rep.rho), orth_ranks=[int(rep.orth_rank[i]) for i in range(rep.n_orth)],
                                       sigma=[float(rep.sigma[i]) for i in range(rep.L)], delta_sq=float(rep.delta_sq),
                                       share=float(rep.share))

    def _xl_workspace(self, nbytes: int) -> torch.Tensor:
        """a 256-byte aligned device buffer of at least nbytes (kept and regrown: the walk calls per tensor)"""
        ws = getattr(self, "_xl_ws", None)
        if ws is None or ws.numel() < nbytes:
            raw = torch.empty(nbytes + 256, dtype=torch.uint8, device=self.device)
            off = (-raw.data_ptr()) % 256
            ws = self._xl_ws = raw[off:off + nbytes]
        return ws

    def xl_probe(self, op: int, *, rows: int, L: int, cols: int = 1, L2: int = 0, trans: int = 0, key: int = 0,
                 finetune: Optional[torch.Tensor] = None, base: Optional[torch.Tensor] = None,
                 x: Optional[torch.Tensor] = None, t: Optional[torch.Tensor] = None,
                 out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
        """one primitive of ``lora_extract`` (``smhip_xl_probe``; tests): the Rademacher panel, a delta product with its
        fold, a panel's Gram, a panel product, or - on host arrays - the eigensolver (returns [L + L * L] fp64)"""
        d = _lib.XlProbeDesc()
        d.op, d.rows, d.cols, d.L, d.L2, d.trans, d.key, d.out_dtype = op, rows, cols, L, L2, trans, key, _DTYPE_CODE[out_dtype]
        keep = []
        if op == _lib.XL_SYM_EIG:
            xin = x.to(torch.float64).cpu().contiguous()
            y = torch.empty(L + L * L, dtype=torch.float64)
            d.x, d.y = xin.data_ptr(), y.data_ptr()
            self._call(self.lib.dll.smhip_xl_probe(self.ctx.h, C.byref(d), self._stream()))
            return y
        if op == _lib.XL_FILL:
            y = torch.empty((rows, L), dtype=torch.float32, device=self.device)
        elif op == _lib.XL_DELTA_MM:
            keep = [self._dev(finetune), self._dev(base), self._dev(x, torch.float32)]
            d.finetune, d.base, d.in_dtype, d.x = keep[0].data_ptr(), keep[1].data_ptr(), _DTYPE_CODE[keep[0].dtype], keep[2].data_ptr()
            y = torch.empty((cols if trans else rows, L), dtype=torch.float32, device=self.device)
        elif op == _lib.XL_GRAM:
            keep = [self._dev(x, torch.float32)]
            d.x = keep[0].data_ptr()
            y = torch.empty((L, L), dtype=torch.float64, device=self.device)
        else:
            keep = [self._dev(x, torch.float32), self._dev(t, torch.float32)]
            d.x, d.t = keep[0].data_ptr(), keep[1].data_ptr()
            y = torch.empty((L2, rows) if trans else (rows, L2), dtype=out_dtype, device=self.device)
        if op in (_lib.XL_DELTA_MM, _lib.XL_GRAM):
            ws = self._xl_workspace(int(self.lib.dll.smhip_xl_probe_workspace(rows, cols, L)))
            d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
        d.y = y.data_ptr()
        self._call(self.lib.dll.smhip_xl_probe(self.ctx.h, C.byref(d), self._stream()))
        return y

    # -- N3: AdditionMerge / TaskAdditionMerge ---------------------------------------------
    def addition_merge(self, finetunes: Sequence[torch.Tensor], base: torch.Tensor, sign_agreement: bool = False) -> torch.Tensor:
        """sum_i (finetune_i - base) in the tensors' dtype, optionally masked by the majority sign
        (reference addition.py:70-76 / taskaddition.py:69-79).  The base is not added back."""
        k = len(finetunes)
        if k < 1 or k > _lib.MAX_MODELS:
            raise ValueError(f"{k} models to merge: supported range is 1..{_lib.MAX_MODELS}")
        dtypes = {t.dtype for t in list(finetunes) + [base]}
        dtype = next(iter(dtypes)) if len(dtypes) == 1 else torch.promote_types(*dtypes) if len(dtypes) == 2 else torch.float32
        if dtype not in _DTYPE_CODE:
            dtype = torch.float32
        bs = self._dev(base, dtype)
        fts = [self._dev(t, dtype) for t in finetunes]
        for t in fts:
            if t.shape != bs.shape:
                raise ValueError(f"shape mismatch: {tuple(t.shape)} vs {tuple(bs.shape)}")
        ptrs = (C.c_void_p * k)(*[t.data_ptr() for t in fts])
        out = torch.empty_like(bs)
        self._call(self.lib.dll.smhip_addition_merge(self.ctx.h, k, ptrs, bs.data_ptr(), _DTYPE_CODE[dtype], bs.numel(),
                                                     1 if sign_agreement else 0, out.data_ptr(), self._stream()))
        return out

    # -- the delta merges (TIES, DARE, Breadcrumbs, the geometric ones, SCE, DELLA, Consensus, the pairwise fusion, PCB, TSV, WIDEN, CABS; merge_layer stages its inputs the same way) ---------
    def _stage_delta_merge(self, desc, finetunes, bases, alphas, base_out, layer_name: str, want_delta: bool,
                           op: Optional[str] = None, out_dtype: Optional[torch.dtype] = None):
        """Device copies of the inputs of one delta-merge call, ``desc``'s common fields (k, finetune, base, alpha,
        in_dtype, base_out, base_out_dtype) and the outputs.  ``op`` names the operator in the check that every
        finetune has a base and an alpha (merge_layer makes none).  Returns (keep, bo, out, delta): ``keep`` holds the
        copies alive until the call returns, ``bo`` is base_out on the device, ``out`` is of ``out_dtype`` (default: bo's).
        ``base_out`` None (delta_stats writes no tensor): the shapes are held to finetune 0's and only ``keep`` is returned."""
        k = len(finetunes)
        if k < 1 or k > _lib.MAX_MODELS:
            raise ValueError(f"{k} models to merge: supported range is 1..{_lib.MAX_MODELS}")
        if op is not None and (len(bases) != k or len(alphas) != k):
            raise ValueError(f"{op}: {k} finetunes, {len(bases)} bases, {len(alphas)} alphas")
        # one input dtype per call (the descriptors' in_dtype).  Mixed dtypes are PROMOTED to
        # fp32, never demoted: the reference upcasts every tensor to fp32 before subtracting
        # (base.py:128-131), so an fp32 base next to bf16 finetunes must keep its low bits
        dtypes = {t.dtype for t in list(finetunes) + list(bases)}
        in_dtype = next(iter(dtypes)) if len(dtypes) == 1 else torch.float32
        if in_dtype not in _DTYPE_CODE:
            in_dtype = torch.float32
        keep = []           # keep device copies alive until the call returns
        desc.k = k
        shape = finetunes[0].shape if base_out is None else base_out.shape
        seen: Dict[int, torch.Tensor] = {}
        for i in range(k):
            ft = self._dev(finetunes[i], in_dtype)
            bkey = id(bases[i])
            if bkey not in seen:
                seen[bkey] = self._dev(bases[i], in_dtype)
            bs = seen[bkey]
            if ft.shape != shape or bs.shape != shape:
                raise ValueError(f"shape mismatch in {layer_name}: {tuple(ft.shape)} / {tuple(bs.shape)} / {tuple(shape)}")
            keep += [ft, bs]
            desc.finetune[i] = ft.data_ptr()
            desc.base[i] = bs.data_ptr()
            desc.alpha[i] = float(alphas[i])
        desc.in_dtype = _DTYPE_CODE[in_dtype]
        if base_out is None:
            return keep, None, None, None
        bo_dtype = base_out.dtype if base_out.dtype in _DTYPE_CODE else torch.float32
        bo = seen.get(id(base_out))
        if bo is None or bo.dtype != bo_dtype:
            bo = self._dev(base_out, bo_dtype)
        keep.append(bo)
        desc.base_out = bo.data_ptr()
        desc.base_out_dtype = _DTYPE_CODE[bo_dtype]
        out = torch.empty(bo.shape, dtype=out_dtype or bo_dtype, device=self.device)
        delta = torch.empty(bo.shape, dtype=torch.float32, device=self.device) if want_delta else None
        return keep, bo, out, delta

    def _run_delta_merge(self, fn, desc, rep, out, delta, layer_name: str, *more):
        """one smhip_*_merge call of the family (``more``: the operator's own arguments between delta_out and the report);
        a NaN or Inf in a delta becomes the ValueError naming the layer"""
        try:
            self.ctx.check(fn(self.ctx.h, C.byref(desc), out.data_ptr(), delta.data_ptr() if delta is not None else None,
                              *more, C.byref(rep), self._stream()))
        except SmhipError as e:
            if e.code == _lib.ERR_NONFINITE:
                raise ValueError(f"Non-finite delta in {layer_name}: {e.message}") from e
            raise

    # -- TIES ------------------------------------------------------------------------------
    def ties_merge(self, finetunes: Sequence[torch.Tensor], bases: Sequence[torch.Tensor], alphas: Sequence[float],
                   base_out: torch.Tensor, density: float = 0.2, lam: float = 1.0, normalize: bool = True,
                   want_delta: bool = False, layer_name: str = "layer"):
        """TIES merge of one tensor of any shape (``smhip_ties_merge``; the function is stated in
        include/shardmerge_hip.h): each delta ``finetune_i - base_i`` trimmed to its ``density`` largest magnitudes
        (ties at the threshold all kept), weighted by ``alpha_i``, a sign elected per element by the weighted sum, the
        agreeing entries summed (``normalize``: divided by the sum of their weights), times ``lam``, added onto
        ``base_out`` in its dtype.  Returns (out, TiesMergeReport[, the fp32 merged delta]).  A NaN or Inf in a delta
        raises ValueError naming ``layer_name`` and the finetune."""
        if not (0.0 < float(density) <= 1.0):
            raise ValueError(f"ties_merge: density {density} is not in (0, 1]")
        desc, rep, k = _lib.TiesDesc(), _lib.TiesReport(), len(finetunes)
        desc.density, desc.lam, desc.normalize = float(density), float(lam), 1 if normalize else 0
        keep, bo, out, delta = self._stage_delta_merge(desc, finetunes, bases, alphas, base_out, layer_name, want_delta, "ties_merge")
        desc.n = bo.numel()
        self._run_delta_merge(self.lib.dll.smhip_ties_merge, desc, rep, out, delta, layer_name)
        report = TiesMergeReport(k_keep=int(rep.k_keep), thresholds=[float(rep.threshold[i]) for i in range(k)],
                                 kept=[int(rep.kept[i]) for i in range(k)])
        return (out, report, delta) if want_delta else (out, report)

    # -- DARE ------------------------------------------------------------------------------
    def dare_merge(self, finetunes: Sequence[torch.Tensor], bases: Sequence[torch.Tensor], alphas: Sequence[float],
                   base_out: torch.Tensor, *, density: float = 0.2, lam: float = 1.0, normalize: bool = True,
                   rescale: bool = True, sign_election: bool = True, key: int = 0, stream_ids: Optional[Sequence[int]] = None,
                   want_delta: bool = False, layer_name: Optional[str] = None):
        """DARE merge of one tensor of any shape (``smhip_dare_merge``; the function is stated in
        include/shardmerge_hip.h): each delta ``finetune_i - base_i`` keeps an element iff the 16-bit draw of the
        counter-based mask (Philox4x32-10 under ``key``, stream ``stream_ids[i]``, indexed by the element) is below
        ``floor(density * 65536)``, survivors are rescaled by the inverse effective density (``rescale``), weighted by
        ``alpha_i`` and either summed (``sign_election=False``: dare_linear) or merged as TIES merges (dare_ties),
        ``normalize``: divided by the weights, times ``lam``, added onto ``base_out`` in its dtype.  ``stream_ids``
        defaults to 0..k-1.  Returns (out, DareMergeReport[, the fp32 merged delta]).  A NaN or Inf in a delta raises
        ValueError naming ``layer_name`` and the finetune."""
        layer_name = layer_name or "layer"
        k = len(finetunes)
        if not (0.0 < float(density) <= 1.0):
            raise ValueError(f"dare_merge: density {density} is not in (0, 1]")
        if float(density) < 2.0 ** -16:
            raise ValueError(f"dare_merge: density {density} is below the smallest density 2^-16 = {2.0 ** -16}")
        stream_ids = list(range(k)) if stream_ids is None else [int(s) for s in stream_ids]
        if len(stream_ids) != k or any(not (0 <= s < 2 ** 32) for s in stream_ids):
            raise ValueError(f"dare_merge: stream_ids must be {k} integers in [0, 2^32)")
        if isinstance(key, bool) or not isinstance(key, int) or not (0 <= key < 2 ** 64):
            raise ValueError("dare_merge: key must be an integer in [0, 2^64)")
        desc, rep = _lib.DareDesc(), _lib.DareReport()
        desc.density, desc.lam, desc.normalize = float(density), float(lam), 1 if normalize else 0
        desc.key, desc.rescale, desc.sign_election = key, 1 if rescale else 0, 1 if sign_election else 0
        keep, bo, out, delta = self._stage_delta_merge(desc, finetunes, bases, alphas, base_out, layer_name, want_delta, "dare_merge")
        desc.n = bo.numel()
        desc.stream_id[:k] = stream_ids
        self._run_delta_merge(self.lib.dll.smhip_dare_merge, desc, rep, out, delta, layer_name)
        report = DareMergeReport(threshold=int(rep.T), density=int(rep.T) / 65536.0, kept=[int(rep.kept[i]) for i in range(k)])
        return (out, report, delta) if want_delta else (out, report)

    # -- DELLA -----------------------------------------------------------------------------
    def della_merge(self, finetunes: Sequence[torch.Tensor], bases: Sequence[torch.Tensor], alphas: Sequence[float],
                    base_out: torch.Tensor, *, density: float = 0.5, epsilon: float = 0.15, lam: float = 1.0, normalize: bool = True,
                    rescale: bool = True, sign_election: bool = True, key: int = 0, stream_ids: Optional[Sequence[int]] = None,
                    want_delta: bool = False, want_thresholds: bool = False, layer_name: Optional[str] = None):
        """DELLA merge of one tensor (``smhip_della_merge``; the function is stated in include/shardmerge_hip.h): DARE
        whose keep threshold rises with the rank of the entry's magnitude within its row (the last dimension; a 1-D
        tensor is one row) from ``density - epsilon`` to ``density + epsilon``; equal magnitudes share a rank.  The
        mask, ``key`` and ``stream_ids`` are those of ``dare_merge``, a survivor is rescaled by the inverse of ITS
        threshold (``rescale``), and the deltas are merged as dare_ties (``sign_election``: della) or dare_linear
        (della_linear) merges them.  ``epsilon=0`` is ``dare_merge`` bit for bit.  Returns (out, DellaMergeReport[, the
        fp32 merged delta][, the uint16 thresholds [k, *shape]]).  A NaN or Inf in a delta raises ValueError naming
        ``layer_name`` and the finetune; so does a row longer than 32768 when ``epsilon > 0``."""
        layer_name = layer_name or "layer"
        k = len(finetunes)
        density, epsilon = float(density), float(epsilon)
        della_arguments(density, epsilon, "della_merge")
        stream_ids = list(range(k)) if stream_ids is None else [int(s) for s in stream_ids]
        if len(stream_ids) != k or any(not (0 <= s < 2 ** 32) for s in stream_ids):
            raise ValueError(f"della_merge: stream_ids must be {k} integers in [0, 2^32)")
        if isinstance(key, bool) or not isinstance(key, int) or not (0 <= key < 2 ** 64):
            raise ValueError("della_merge: key must be an integer in [0, 2^64)")
        desc, rep = _lib.DellaDesc(), _lib.DellaReport()
        desc.density, desc.lam, desc.normalize = density, float(lam), 1 if normalize else 0
        desc.key, desc.rescale, desc.sign_election = key, 1 if rescale else 0, 1 if sign_election else 0
        keep, bo, out, delta = self._stage_delta_merge(desc, finetunes, bases, alphas, base_out, layer_name, want_delta, "della_merge")
        desc.n = bo.numel()
        cols = int(bo.shape[-1]) if bo.ndim >= 1 else 1
        if epsilon > 0.0 and cols > _lib.DELLA_MAX_COLS:
            raise ValueError(f"della_merge: the rows of {layer_name} have c = {cols} elements, above the limit of {_lib.DELLA_MAX_COLS} "
                             f"(a row is ranked in the LDS of one compute unit)")
        desc.epsilon, desc.rows = epsilon, (desc.n // cols if cols else 1) or 1
        desc.stream_id[:k] = stream_ids
        thresholds = torch.zeros((k,) + tuple(bo.shape), dtype=torch.int16, device=self.device) if want_thresholds else None
        self._run_delta_merge(self.lib.dll.smhip_della_merge, desc, rep, out, delta, layer_name,
                              thresholds.data_ptr() if thresholds is not None else None)
        report = DellaMergeReport(threshold_lo=int(rep.T_lo), threshold_hi=int(rep.T_hi), kept=[int(rep.kept[i]) for i in range(k)])
        res = (out, report) + ((delta,) if want_delta else ())
        if want_thresholds:     # (uint16 values in an int16 tensor: widened here, 65536 of density 1 does not fit and is never written)
            res += (thresholds.to(torch.int32) & 0xFFFF if density < 1.0 else torch.full_like(thresholds, 65536, dtype=torch.int32),)
        return res

    # -- Model Breadcrumbs ---------------------------------------------------------------
    def breadcrumbs_merge(self, finetunes: Sequence[torch.Tensor], bases: Sequence[torch.Tensor], alphas: Sequence[float],
                          base_out: torch.Tensor, density: float = 0.9, gamma: float = 0.01, lam: float = 1.0,
                          normalize: bool = True, sign_election: bool = False, want_delta: bool = False,
                          layer_name: Optional[str] = None):
        """Model Breadcrumbs merge of one tensor of any shape (``smhip_breadcrumbs_merge``; the function is stated in
        include/shardmerge_hip.h): each delta ``finetune_i - base_i`` loses its ``floor(gamma * n)`` largest magnitudes
        and keeps the next ``floor(density * n)`` (ties at either threshold all kept), is weighted by ``alpha_i`` and
        either summed (``sign_election=False``: breadcrumbs, ``normalize``: divided by the sum of all weights) or merged
        as TIES merges (breadcrumbs_ties), times ``lam``, added onto ``base_out`` in its dtype.  Returns
        (out, BreadcrumbsMergeReport[, the fp32 merged delta]).  A NaN or Inf in a delta raises ValueError naming
        ``layer_name`` and the finetune."""
        layer_name = layer_name or "layer"
        if not (0.0 < float(density) <= 1.0):
            raise ValueError(f"breadcrumbs_merge: density {density} is not in (0, 1]")
        if not (0.0 <= float(gamma) < 1.0):
            raise ValueError(f"breadcrumbs_merge: gamma {gamma} is not in [0, 1)")
        if not (float(density) + float(gamma) <= 1.0):
            raise ValueError(f"breadcrumbs_merge: density {density} + gamma {gamma} exceeds 1")
        desc, rep, k = _lib.BreadcrumbsDesc(), _lib.BreadcrumbsReport(), len(finetunes)
        desc.density, desc.lam, desc.normalize = float(density), float(lam), 1 if normalize else 0
        desc.gamma, desc.sign_election = float(gamma), 1 if sign_election else 0
        keep, bo, out, delta = self._stage_delta_merge(desc, finetunes, bases, alphas, base_out, layer_name, want_delta, "breadcrumbs_merge")
        desc.n = bo.numel()
        self._run_delta_merge(self.lib.dll.smhip_breadcrumbs_merge, desc, rep, out, delta, layer_name)
        report = BreadcrumbsMergeReport(k_keep=int(rep.k_keep), n_top=int(rep.n_top),
                                        thresholds_lo=[float(rep.threshold_lo[i]) for i in range(k)],
                                        thresholds_hi=[float(rep.threshold_hi[i]) for i in range(k)],
                                        kept=[int(rep.kept[i]) for i in range(k)],
                                        dropped_top=[int(rep.dropped_top[i]) for i in range(k)])
        return (out, report, delta) if want_delta else (out, report)

    # -- Model Stock, NuSLERP, SLERP -------------------------------------------------------
    GEO_MODES = {"model_stock": _lib.GEO_MODEL_STOCK, "nuslerp": _lib.GEO_NUSLERP, "slerp": _lib.GEO_SLERP}

    def geo_merge(self, finetunes: Sequence[torch.Tensor], bases: Sequence[torch.Tensor], alphas: Sequence[float],
                  base_out: torch.Tensor, *, mode: str = "model_stock", rowwise: bool = False, want_delta: bool = False,
                  layer_name: Optional[str] = None):
        """Geometric merge of one tensor of any shape (``smhip_geo_merge``; the function is stated in
        include/shardmerge_hip.h).  The fp64 Gram matrix of the vectors (the deltas ``finetune_i - base_i``; the
        finetunes themselves for ``slerp``) is summed in an order that depends on the element count only, the
        coefficients follow from it - ``model_stock``: the ratio t from the mean cosine, ``rowwise``: per row of the
        first dimension; ``nuslerp`` / ``slerp``: the spherical interpolation of two vectors at
        ``alpha_1 / (alpha_0 + alpha_1)`` - and one pass writes ``base_out + sum c_i x_i`` (``slerp``: ``sum c_i x_i``)
        in base_out's dtype.  Returns (out, GeoMergeReport[, the fp32 combination M]).  A NaN or Inf in a vector raises
        ValueError naming ``layer_name`` and the finetune."""
        layer_name = layer_name or "layer"
        if mode not in self.GEO_MODES:
            raise ValueError(f"geo_merge: mode {mode!r} is not one of {sorted(self.GEO_MODES)}")
        k = len(finetunes)
        if mode != "model_stock":
            if rowwise:
                raise ValueError(f"geo_merge: rowwise is an option of mode model_stock, not of {mode}")
            if k > 2:
                raise ValueError(f"geo_merge: mode {mode} merges at most 2 models, not {k}")
            if k == 2 and len(alphas) == 2 and not (float(alphas[0]) >= 0 and float(alphas[1]) >= 0 and float(alphas[0]) + float(alphas[1]) > 0):
                raise ValueError(f"geo_merge: mode {mode} needs alphas >= 0 with a sum > 0, not {list(alphas)}")
        desc, rep = _lib.GeoDesc(), _lib.GeoReport()
        keep, bo, out, delta = self._stage_delta_merge(desc, finetunes, bases, alphas, base_out, layer_name, want_delta, "geo_merge")
        desc.n = bo.numel()
        desc.mode, desc.rowwise = self.GEO_MODES[mode], 1 if rowwise else 0
        desc.rows = (bo.shape[0] if bo.ndim > 1 else 1) or 1
        self._run_delta_merge(self.lib.dll.smhip_geo_merge, desc, rep, out, delta, layer_name)
        report = GeoMergeReport(mode=mode, rowwise=bool(rowwise), cos=float(rep.cos), t=float(rep.t), omega=float(rep.omega),
                                linear=bool(rep.linear), t_min=float(rep.t_min), t_max=float(rep.t_max), t_mean=float(rep.t_mean))
        if not rowwise:
            report.gram = [[float(rep.G[i][j]) for j in range(k)] for i in range(k)]
            report.coefficients = [float(rep.c[i]) for i in range(k)]
        return (out, report, delta) if want_delta else (out, report)

    # -- Karcher means: karcher, multislerp -----------------------------------------------
    SPHERE_MODES = {"karcher": 1, "multislerp": 0}                # mode -> weight_space
    SPHERE_FNS = {"acos": _lib.SPHERE_ACOS, "sin": _lib.SPHERE_SIN, "cos": _lib.SPHERE_COS}

    def sphere_merge(self, finetunes: Sequence[torch.Tensor], bases: Sequence[torch.Tensor], alphas: Sequence[float],
                     base_out: torch.Tensor, *, mode: str = "karcher", rowwise: bool = False, max_iter: int = 10, tol: float = 1e-5,
                     want_delta: bool = False, layer_name: Optional[str] = None):
        """Karcher-mean merge of one tensor of any shape (``smhip_sphere_merge``; the function is stated in
        include/shardmerge_hip.h).  The directions of the k vectors (``karcher``: the finetunes themselves;
        ``multislerp``: the deltas ``finetune_i - base_i``) are averaged on the sphere with the weights
        ``alpha_i / sum alpha`` - the log map iterated at most ``max_iter`` times, until the step is below ``tol``, on k
        coefficients against the fp64 Gram matrix - and their lengths linearly; ``rowwise``: one mean per row of the
        first dimension.  One pass writes ``sum c_i x_i`` (``multislerp``: ``base_out + sum c_i x_i``) in base_out's
        dtype.  Returns (out, SphereMergeReport[, the fp32 combination M]).  A NaN or Inf in a vector raises ValueError
        naming ``layer_name`` and the finetune."""
        layer_name = layer_name or "layer"
        if mode not in self.SPHERE_MODES:
            raise ValueError(f"sphere_merge: mode {mode!r} is not one of {sorted(self.SPHERE_MODES)}")
        k = len(finetunes)
        if len(alphas) == k and not (all(float(a) >= 0 for a in alphas) and 0 < sum(float(a) for a in alphas) < float("inf")):
            raise ValueError(f"sphere_merge: mode {mode} needs alphas >= 0 with a sum > 0, not {list(alphas)}")
        if isinstance(max_iter, bool) or not isinstance(max_iter, int) or not (1 <= max_iter <= 100):
            raise ValueError(f"sphere_merge: max_iter {max_iter!r} is not an integer in 1..100")
        if not (0.0 <= float(tol) < 1.0):
            raise ValueError(f"sphere_merge: tol {tol} is not in [0, 1)")
        desc, rep = _lib.SphereDesc(), _lib.SphereReport()
        keep, bo, out, delta = self._stage_delta_merge(desc, finetunes, bases, alphas, base_out, layer_name, want_delta, "sphere_merge")
        desc.n = bo.numel()
        desc.weight_space, desc.rowwise = self.SPHERE_MODES[mode], 1 if rowwise else 0
        desc.rows = (bo.shape[0] if bo.ndim > 1 else 1) or 1
        desc.max_iter, desc.tol = int(max_iter), float(tol)
        report = SphereMergeReport(mode=mode, rowwise=bool(rowwise), max_iter=int(max_iter), tol=float(tol))
        if rowwise and desc.n:
            R = int(desc.rows)
            report.row_coefficients = torch.zeros(R, k, dtype=torch.float32)
            report.row_iterations = torch.zeros(R, dtype=torch.int32)
            report.row_flags = torch.zeros(R, dtype=torch.int32)
            desc.row_coef, desc.row_iters, desc.row_flags = (report.row_coefficients.data_ptr(), report.row_iterations.data_ptr(),
                                                             report.row_flags.data_ptr())
        self._run_delta_merge(self.lib.dll.smhip_sphere_merge, desc, rep, out, delta, layer_name)
        if rowwise:
            report.iters_max, report.rows_unconverged, report.rows_linear = int(rep.iters_max), int(rep.rows_unconverged), int(rep.rows_linear)
            report.csum_min, report.csum_max, report.csum_mean = float(rep.csum_min), float(rep.csum_max), float(rep.csum_mean)
        else:
            report.gram = [[float(rep.G[i][j]) for j in range(k)] for i in range(k)]
            report.cosines = [[float(rep.H[i][j]) for j in range(k)] for i in range(k)]
            report.weights = [float(rep.w[i]) for i in range(k)]
            report.a = [float(rep.a[i]) for i in range(k)]
            report.length = float(rep.N)
            report.coefficients = [float(rep.c[i]) for i in range(k)]
            report.iterations, report.tau = int(rep.iterations), float(rep.tau)
            report.converged, report.linear = bool(rep.converged), bool(rep.linear)
        return (out, report, delta) if want_delta else (out, report)

    def sphere_fn(self, op: str, x: torch.Tensor, on_device: bool = True) -> torch.Tensor:
        """``sm_acos`` / ``sm_sin`` / ``sm_cos`` of csrc/sm_sphere.hpp over an fp64 array (``smhip_sphere_fn``): by a
        kernel on the engine's device, or on the host.  Returns an fp64 CPU tensor."""
        if op not in self.SPHERE_FNS:
            raise ValueError(f"sphere_fn: op {op!r} is not one of {sorted(self.SPHERE_FNS)}")
        x = x.detach().to(torch.float64).contiguous().reshape(-1)
        x = x.to(self.device) if on_device else x.cpu()
        y = torch.empty_like(x)
        self.ctx.check(self.lib.dll.smhip_sphere_fn(self.ctx.h, self.SPHERE_FNS[op], x.data_ptr(), y.data_ptr(), x.numel(),
                                                    1 if on_device else 0, self._stream() if on_device else None))
        if on_device and self.device.type != "cpu":
            torch.cuda.synchronize(self.device)
        return y.cpu()

    # -- SCE ------------------------------------------------------------------------------
    def sce_merge(self, finetunes: Sequence[torch.Tensor], bases: Sequence[torch.Tensor], alphas: Sequence[float],
                  base_out: torch.Tensor, *, select_topk: float = 1.0, lam: float = 1.0, want_delta: bool = False,
                  layer_name: Optional[str] = None):
        """SCE merge of one tensor of any shape (``smhip_sce_merge``; the function is stated in
        include/shardmerge_hip.h): the elements whose deltas ``finetune_i - base_i`` vary most across the finetunes are
        selected (the ``select_topk`` share of the nonzero variances, ties at the threshold all kept; everything when
        ``select_topk`` is 1 or there is one finetune), each finetune is weighted by ``alpha_i`` times the fp64 energy of
        its selected entries, normalised over the finetunes, a sign is elected per element by the unweighted sum, the
        agreeing entries are summed and divided by the sum of their weights, times ``lam``, added onto ``base_out`` in
        its dtype.  Returns (out, SceMergeReport[, the fp32 merged delta]).  A NaN or Inf in a delta raises ValueError
        naming ``layer_name`` and the finetune."""
        layer_name = layer_name or "layer"
        if not (0.0 < float(select_topk) <= 1.0):
            raise ValueError(f"sce_merge: select_topk {select_topk} is not in (0, 1]")
        if not math.isfinite(float(lam)):
            raise ValueError(f"sce_merge: lam {lam} is not finite")
        total = 0.0
        for a in alphas:
            if not (float(a) >= 0.0) or not math.isfinite(float(a)):
                raise ValueError(f"sce_merge: the alphas must be >= 0 and finite, not {list(alphas)}")
            total += float(a)
        if len(alphas) and not (0.0 < total < math.inf):
            raise ValueError(f"sce_merge: the alphas need a sum > 0, not {list(alphas)}")
        desc, rep, k = _lib.SceDesc(), _lib.SceReport(), len(finetunes)
        desc.select_topk, desc.lam = float(select_topk), float(lam)
        keep, bo, out, delta = self._stage_delta_merge(desc, finetunes, bases, alphas, base_out, layer_name, want_delta, "sce_merge")
        desc.n = bo.numel()
        self._run_delta_merge(self.lib.dll.smhip_sce_merge, desc, rep, out, delta, layer_name)
        report = SceMergeReport(nz=int(rep.nz), k_keep=int(rep.k_keep), selected=int(rep.selected), threshold=float(rep.threshold),
                                energies=[float(rep.energy[i]) for i in range(k)], weights=[float(rep.weight[i]) for i in range(k)])
        return (out, report, delta) if want_delta else (out, report)

    # -- Consensus (TALL masks) ---------------------------------------------------------------
    def consensus_merge(self, finetunes: Sequence[torch.Tensor], bases: Sequence[torch.Tensor], alphas: Sequence[float],
                        base_out: torch.Tensor, *, ties: bool = False, density: float = 0.2, mask_lambda: float = 0.4,
                        consensus_k: int = 2, lam: float = 1.0, normalize: bool = True, want_delta: bool = False,
                        layer_name: Optional[str] = None):
        """Consensus merge of one tensor of any shape (``smhip_consensus_merge``; the function is stated in
        include/shardmerge_hip.h): the weighted entries ``tv_i = (finetune_i - base_i) * alpha_i`` are summed
        (``ties=False``: consensus_ta) or merged as TIES merges them at ``density`` (``ties=True``: consensus_ties) into
        the multi-task vector U; finetune i's TALL mask is set where ``|tv_i| >= mask_lambda * |U - tv_i|``; an element
        of U is kept where at least ``min(consensus_k, k)`` masks are set and zeroed elsewhere; ``normalize``: divided
        by the weights (consensus_ties: inside the TIES merge), times ``lam``, added onto ``base_out`` in its dtype.
        Returns (out, ConsensusMergeReport[, the fp32 merged delta]).  A NaN or Inf in a delta raises ValueError naming
        ``layer_name`` and the finetune."""
        layer_name = layer_name or "layer"
        if ties and not (0.0 < float(density) <= 1.0):
            raise ValueError(f"consensus_merge: density {density} is not in (0, 1]")
        if not (0.0 <= float(mask_lambda) <= 1e6):
            raise ValueError(f"consensus_merge: mask_lambda {mask_lambda} is not in [0, 1e6]")
        if isinstance(consensus_k, bool) or not isinstance(consensus_k, int) or not (1 <= consensus_k <= _lib.MAX_MODELS):
            raise ValueError(f"consensus_merge: consensus_k must be an integer in 1..{_lib.MAX_MODELS}, not {consensus_k!r}")
        if not math.isfinite(float(lam)):
            raise ValueError(f"consensus_merge: lam {lam} is not finite")
        desc, rep, k = _lib.ConsensusDesc(), _lib.ConsensusReport(), len(finetunes)
        desc.density, desc.lam, desc.normalize = float(density), float(lam), 1 if normalize else 0
        desc.mask_lambda, desc.consensus_k, desc.ties = float(mask_lambda), consensus_k, 1 if ties else 0
        keep, bo, out, delta = self._stage_delta_merge(desc, finetunes, bases, alphas, base_out, layer_name, want_delta, "consensus_merge")
        desc.n = bo.numel()
        self._run_delta_merge(self.lib.dll.smhip_consensus_merge, desc, rep, out, delta, layer_name)
        report = ConsensusMergeReport(ties=bool(ties), k_keep=int(rep.k_keep),
                                      thresholds=[float(rep.threshold[i]) for i in range(k)] if ties else [],
                                      kept=[int(rep.kept[i]) for i in range(k)] if ties else [],
                                      masked=[int(rep.masked[i]) for i in range(k)],
                                      agree=[int(rep.agree[c]) for c in range(k + 1)], selected=int(rep.selected), n=int(desc.n))
        return (out, report, delta) if want_delta else (out, report)

    # -- pairwise fusion: arcee_fusion, nearswap --------------------------------------------------
    FUSION_MODES = {"arcee": _lib.FUSION_ARCEE, "nearswap": _lib.FUSION_NEARSWAP}
    FUSION_FNS = {"exp": _lib.FUSION_EXP, "log": _lib.FUSION_LOG}

    def fusion_merge(self, ft: torch.Tensor, base: torch.Tensor, base_out: torch.Tensor, *, mode: str, iqr_mult: float = 1.5,
                     t: Optional[float] = None, want_delta: bool = False, want_kl: bool = False, layer_name: Optional[str] = None):
        """Pairwise fusion of ONE finetune onto a base, one tensor of any shape (``smhip_fusion_merge``; the function is
        stated in include/shardmerge_hip.h).  ``arcee``: a row of the last dimension (a 1-D tensor is one row) gets the
        fp64 KL divergence of its softmax in the finetune from its softmax in the base, an element's score is
        ``|finetune - base|`` times its row's KL, and the delta is taken where the score exceeds
        ``median + iqr_mult * (Q3 - Q1)`` of all scores (exact quartiles), dropped elsewhere.  ``nearswap``: the delta
        is clamped to ``[-t, t]``.  The gated delta is added onto ``base_out`` in its dtype.  Returns (out,
        FusionMergeReport[, the fp32 gated delta]); ``want_kl`` puts the row KLs into the report.  A NaN or Inf in
        the finetune, the base or their difference raises ValueError naming ``layer_name`` and the tensor."""
        layer_name = layer_name or "layer"
        if mode not in self.FUSION_MODES:
            raise ValueError(f"fusion_merge: mode {mode!r} is not one of {sorted(self.FUSION_MODES)}")
        arcee = mode == "arcee"
        if arcee and not math.isfinite(float(iqr_mult)):
            raise ValueError(f"fusion_merge: iqr_mult {iqr_mult} is not finite")
        if not arcee and (t is None or not (0.0 < float(t) < math.inf)):
            raise ValueError(f"fusion_merge: mode nearswap needs t > 0 and finite, not {t!r}")
        desc, rep = _lib.FusionDesc(), _lib.FusionReport()
        keep, bo, out, delta = self._stage_delta_merge(desc, [ft], [base], [1.0], base_out, layer_name, want_delta, "fusion_merge")
        desc.n = bo.numel()
        desc.mode = self.FUSION_MODES[mode]
        cols = bo.shape[-1] if bo.ndim >= 1 else 1
        desc.rows = (desc.n // cols if cols else 1) or 1
        desc.iqr_mult, desc.t = float(iqr_mult), float(t) if t is not None else 0.0
        kl = None
        if arcee and want_kl:
            kl = torch.zeros(int(desc.rows) if desc.n else 0, dtype=torch.float32, device=self.device)
            desc.kl_out = kl.data_ptr() if kl.numel() else None
        self._run_delta_merge(self.lib.dll.smhip_fusion_merge, desc, rep, out, delta, layer_name)
        report = FusionMergeReport(mode=mode, n=int(desc.n))
        if arcee:
            report.q1, report.q2, report.q3, report.threshold = float(rep.q1), float(rep.q2), float(rep.q3), float(rep.threshold)
            report.selected, report.kl_min, report.kl_max, report.kl = int(rep.selected), float(rep.kl_min), float(rep.kl_max), kl
        else:
            report.clipped = int(rep.clipped)
        return (out, report, delta) if want_delta else (out, report)

    def fusion_fn(self, op: str, x: torch.Tensor, on_device: bool = True) -> torch.Tensor:
        """``sm_exp`` / ``sm_log`` of csrc/sm_fusion.hpp over an fp64 array (``smhip_fusion_fn``): by a kernel on the
        engine's device, or on the host.  Returns an fp64 CPU tensor."""
        if op not in self.FUSION_FNS:
            raise ValueError(f"fusion_fn: op {op!r} is not one of {sorted(self.FUSION_FNS)}")
        x = x.detach().to(torch.float64).contiguous().reshape(-1)
        x = x.to(self.device) if on_device else x.cpu()
        y = torch.empty_like(x)
        self.ctx.check(self.lib.dll.smhip_fusion_fn(self.ctx.h, self.FUSION_FNS[op], x.data_ptr(), y.data_ptr(), x.numel(),
                                                    1 if on_device else 0, self._stream() if on_device else None))
        if on_device and self.device.type != "cpu":
            torch.cuda.synchronize(self.device)
        return y.cpu()

    # -- PCB (parameter competition balancing) ---------------------------------------------------
    PCB_FNS = {"tanh": _lib.PCB_TANH}

    def pcb_merge(self, finetunes: Sequence[torch.Tensor], bases: Sequence[torch.Tensor], alphas: Sequence[float],
                  base_out: torch.Tensor, *, ratio: float = 0.1, clip: float = 0.0001, lam: float = 1.0,
                  want_delta: bool = False, layer_name: str = ""):
        """PCB merge of one tensor of any shape (``smhip_pcb_merge``; the function is stated in
        include/shardmerge_hip.h): every weighted entry ``tv_i = (finetune_i - base_i) * alpha_i`` is scored by how
        large it is within its own finetune (its magnitude, clamped at the ``clip`` share of either end and min-max
        normalised, through ``exp``) times how well it agrees with the sum of all entries of its element (through
        ``tanh``, entries that oppose the sum score 0); per finetune the ``ratio`` share of the highest scores is kept,
        rescaled to [0, 1], and the clamped entries are averaged with those weights, times ``lam``, added onto
        ``base_out`` in its dtype.  Returns (out, PcbMergeReport[, the fp32 merged delta before ``lam``]).  A NaN or Inf
        in a delta raises ValueError naming ``layer_name`` and the finetune."""
        layer_name = layer_name or "layer"
        if not (0.0 < float(ratio) <= 1.0):
            raise ValueError(f"pcb_merge: ratio {ratio} is not in (0, 1]")
        if not (0.0 <= float(clip) < 0.5):
            raise ValueError(f"pcb_merge: clip {clip} is not in [0, 0.5)")
        if not math.isfinite(float(lam)):
            raise ValueError(f"pcb_merge: lam {lam} is not finite")
        desc, rep, k = _lib.PcbDesc(), _lib.PcbReport(), len(finetunes)
        desc.ratio, desc.clip, desc.lam = float(ratio), float(clip), float(lam)
        keep, bo, out, delta = self._stage_delta_merge(desc, finetunes, bases, alphas, base_out, layer_name, want_delta, "pcb_merge")
        desc.n = bo.numel()
        self._run_delta_merge(self.lib.dll.smhip_pcb_merge, desc, rep, out, delta, layer_name)
        per = lambda a, cast: [cast(a[i]) for i in range(k)]
        report = PcbMergeReport(n=int(desc.n), clip_rank=int(rep.clip_rank), q=int(rep.q), lo=per(rep.lo, float), hi=per(rep.hi, float),
                                t=per(rep.t, float), M=per(rep.M, float), positive=per(rep.positive, int),
                                selected=per(rep.selected, int), covered=int(rep.covered), contested=int(rep.contested))
        return (out, report, delta) if want_delta else (out, report)

    def pcb_fn(self, op: str, x: torch.Tensor, on_device: bool = True) -> torch.Tensor:
        """``sm_tanh`` of csrc/sm_pcb.hpp over an fp64 array (``smhip_pcb_fn``): by a kernel on the engine's device, or
        on the host.  Returns an fp64 CPU tensor."""
        if op not in self.PCB_FNS:
            raise ValueError(f"pcb_fn: op {op!r} is not one of {sorted(self.PCB_FNS)}")
        x = x.detach().to(torch.float64).contiguous().reshape(-1)
        x = x.to(self.device) if on_device else x.cpu()
        y = torch.empty_like(x)
        self.ctx.check(self.lib.dll.smhip_pcb_fn(self.ctx.h, self.PCB_FNS[op], x.data_ptr(), y.data_ptr(), x.numel(),
                                                 1 if on_device else 0, self._stream() if on_device else None))
        if on_device and self.device.type != "cpu":
            torch.cuda.synchronize(self.device)
        return y.cpu()

    # -- TSV (task singular vectors) ------------------------------------------------------------
    def tsv_merge(self, finetunes: Sequence[torch.Tensor], bases: Sequence[torch.Tensor], alphas: Sequence[float],
                  base_out: torch.Tensor, *, rank: int = 64, power_iters: int = 2, lam: float = 1.0, key: int = 0,
                  want_delta: bool = False, layer_name: str = ""):
        """TSV merge of one tensor with at least two dimensions, viewed as ``[shape[0], rest]`` (``smhip_tsv_merge``; the
        function is stated in include/shardmerge_hip.h): the ``rank`` leading singular triplets of every delta
        ``finetune_i - base_i`` by a randomized subspace iteration with ``power_iters`` power steps under ``key``, the
        singular vectors of all finetunes whitened together (Loewdin) so that overlapping subspaces are counted once, the
        merged delta rebuilt with the singular values times ``alpha_i`` and added, times ``lam``, onto ``base_out`` in its
        dtype.  An entry with ``alpha_i == 0`` is skipped; the others must satisfy ``k * min(rank, rows, cols) <= 256``.
        Returns (out, TsvReport[, the fp32 merged delta before ``lam``]).  A NaN or Inf in a delta raises ValueError
        naming ``layer_name`` and the finetune."""
        layer_name = layer_name or "layer"
        if isinstance(rank, bool) or not isinstance(rank, int) or not (1 <= rank <= _lib.EXTRACT_MAX_RANK):
            raise ValueError(f"tsv_merge: rank must be an integer in 1..{_lib.EXTRACT_MAX_RANK}, not {rank!r}")
        if isinstance(power_iters, bool) or not isinstance(power_iters, int) or not (0 <= power_iters <= _lib.EXTRACT_MAX_POWER):
            raise ValueError(f"tsv_merge: power_iters must be an integer in 0..{_lib.EXTRACT_MAX_POWER}, not {power_iters!r}")
        if not math.isfinite(float(lam)):
            raise ValueError(f"tsv_merge: lam {lam} is not finite")
        if any(not (float(a) >= 0.0) for a in alphas):
            raise ValueError(f"tsv_merge: the alphas {list(alphas)} must be >= 0")
        if base_out.ndim < 2:
            raise ValueError(f"tsv_merge: {layer_name} has shape {list(base_out.shape)}; at least two dimensions expected")
        desc, rep, k = _lib.TsvDesc(), _lib.TsvReport(), len(finetunes)
        keep, bo, out, delta = self._stage_delta_merge(desc, finetunes, bases, alphas, base_out, layer_name, want_delta, "tsv_merge")
        desc.n = bo.numel()
        rows = int(bo.shape[0])
        cols = int(desc.n // rows) if rows else 0
        desc.rows, desc.cols, desc.rank, desc.power_iters, desc.lam, desc.key = rows, cols, rank, power_iters, float(lam), int(key)
        r = min(rank, rows, cols)
        active = sum(1 for a in alphas if float(a) != 0.0)
        if active * r > _lib.TSV_MAX_R:
            raise ValueError(f"tsv_merge: {layer_name}: {active} finetunes x rank {r} = {active * r} singular vectors; at most {_lib.TSV_MAX_R}")
        if desc.n:
            ws = self._xl_workspace(int(self.lib.dll.smhip_tsv_workspace(rows, cols, k, rank)))
            desc.workspace, desc.workspace_bytes = ws.data_ptr(), ws.numel()
        self._run_delta_merge(self.lib.dll.smhip_tsv_merge, desc, rep, out, delta, layer_name)
        report = TsvReport(rows=rows, cols=cols, rank=rank, power_iters=power_iters, width=int(rep.L), r=int(rep.r), R=int(rep.R),
                           Rp=int(rep.Rp), rho=[int(rep.rho[i]) for i in range(k)],
                           sigma=[[float(rep.sigma[i][j]) for j in range(rep.r)] for i in range(k)],
                           delta_sq=[float(rep.delta_sq[i]) for i in range(k)], share=[float(rep.share[i]) for i in range(k)],
                           orth_ranks=[[int(rep.orth_rank[i][j]) for j in range(rep.n_orth[i])] for i in range(k)],
                           mu_U=[float(rep.mu_U[j]) for j in range(rep.R)], mu_W=[float(rep.mu_W[j]) for j in range(rep.R)],
                           kept_U=int(rep.kept_U), kept_W=int(rep.kept_W))
        return (out, report, delta) if want_delta else (out, report)

    def tsv_probe(self, b: torch.Tensor, w: torch.Tensor, base_out: torch.Tensor, lam: float = 1.0):
        """``tsv_apply`` alone (``smhip_tsv_probe``; tests): (out, merged) for fp32 panels ``b [rows, Rp]``, ``w [cols, Rp]``
        and ``base_out [rows, cols]``, which are used where they lie when they are contiguous on the engine's device"""
        place = lambda t: t if (t.device == self.device and t.is_contiguous()) else self._dev(t)
        bv, wv, bo = place(b), place(w), place(base_out)
        rows, cols = bo.shape
        out = torch.empty_like(bo)
        merged = torch.empty((rows, cols), dtype=torch.float32, device=self.device)
        self._call(self.lib.dll.smhip_tsv_probe(self.ctx.h, bv.data_ptr(), wv.data_ptr(), rows, cols, int(bv.shape[1]), bo.data_ptr(),
                                                _DTYPE_CODE[bo.dtype], float(lam), out.data_ptr(), merged.data_ptr(), self._stream()))
        return out, merged

    # -- Iso-C (isotropic merging) ----------------------------------------------------------------
    def iso_merge(self, finetunes: Sequence[torch.Tensor], bases: Sequence[torch.Tensor], alphas: Sequence[float],
                  base_out: torch.Tensor, *, lam: float = 1.0, tol: float = 1e-4, max_iter: int = 40,
                  want_delta: bool = False, layer_name: str = ""):
        """Iso-C merge of one tensor with at least two dimensions, viewed as ``[shape[0], rest]`` (``smhip_iso_merge``; the
        function is stated in include/shardmerge_hip.h): the sum ``T`` of the deltas ``finetune_i - base_i`` times
        ``alpha_i`` with its singular values replaced by their mean - ``mean(S) U V^T``, the polar factor of ``T`` by a
        Newton-Schulz iteration on fp32 MFMA that stops at ``||X X^T - I||_F / sqrt(s) <= tol`` or after ``max_iter``
        steps (which is reported, not raised) - added, times ``lam``, onto ``base_out`` in its dtype.
        ``min(rows, cols) <= 16384``.  Returns (out, IsoReport[, the fp32 merged delta before ``lam``]).  A NaN or Inf in
        a delta or in the sum raises ValueError naming ``layer_name``."""
        layer_name = layer_name or "layer"
        if not math.isfinite(float(lam)):
            raise ValueError(f"iso_merge: lam {lam} is not finite")
        if not (0.0 < float(tol) <= 1.0):
            raise ValueError(f"iso_merge: tol {tol} is not in (0, 1]")
        if isinstance(max_iter, bool) or not isinstance(max_iter, int) or not (0 <= max_iter <= _lib.ISO_MAX_ITER):
            raise ValueError(f"iso_merge: max_iter must be an integer in 0..{_lib.ISO_MAX_ITER}, not {max_iter!r}")
        if base_out.ndim < 2:
            raise ValueError(f"iso_merge: {layer_name} has shape {list(base_out.shape)}; at least two dimensions expected")
        rows = int(base_out.shape[0])
        cols = int(base_out.numel() // rows) if rows else 0
        if min(rows, cols) > _lib.ISO_MAX_S:        # (before anything is staged)
            raise ValueError(f"iso_merge: {layer_name} has shape {list(base_out.shape)}: min(rows, cols) = {min(rows, cols)}, at most {_lib.ISO_MAX_S}")
        desc, rep = _lib.IsoDesc(), _lib.IsoReport()
        keep, bo, out, delta = self._stage_delta_merge(desc, finetunes, bases, alphas, base_out, layer_name, want_delta, "iso_merge")
        desc.n = bo.numel()
        desc.rows, desc.cols, desc.lam, desc.tol, desc.max_iter = rows, cols, float(lam), float(tol), max_iter
        if desc.n:
            ws = self._xl_workspace(int(self.lib.dll.smhip_iso_workspace(rows, cols)))
            desc.workspace, desc.workspace_bytes = ws.data_ptr(), ws.numel()
        self._run_delta_merge(self.lib.dll.smhip_iso_merge, desc, rep, out, delta, layer_name)
        it = int(rep.iterations)
        report = IsoReport(rows=rows, cols=cols, s=int(rep.s), L=int(rep.L), transposed=bool(rep.transposed), nu=float(rep.nu),
                           iterations=it, steps=rep.steps.decode(), e=[float(rep.e[t]) for t in range(it + 1)] if rep.nu > 0.0 else [],
                           converged=bool(rep.converged), N=float(rep.N), sigma_bar=float(rep.sigma_bar), zero=bool(rep.zero))
        return (out, report, delta) if want_delta else (out, report)

    def iso_gemm(self, a: torch.Tensor, b: torch.Tensor, *, form: int = 0, sym: bool = False, epilogue: int = 0,
                 ca: float = 0.0, cb: float = 0.0, e: Optional[torch.Tensor] = None, ldc: Optional[int] = None) -> torch.Tensor:
        """``iso_gemm`` alone (``smhip_iso_gemm``; tests and tools): ``ep(a b^T)`` (form 0, ``b [N, K]``) or ``ep(a b)``
        (form 1, ``b [K, N]``) for 2-D fp32 tensors whose rows are contiguous - views with an offset or a pitch are used
        where they lie when they are on the engine's device.  Returns ``c [M, N]`` (a view of pitch ``ldc`` when given)."""
        def place(t):
            if t is None:
                return None
            if t.dtype != torch.float32 or t.device != self.device or t.ndim != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
                return self._dev(t, torch.float32)
            return t
        av, bv, ev = place(a), place(b), place(e)
        M, K = av.shape
        N = bv.shape[0] if form == _lib.ISO_NT else bv.shape[1]
        pitch = lambda t: int(t.stride(0)) if t.shape[0] > 1 else int(t.shape[1])
        ldc = int(ldc or N)
        store = torch.zeros((M, ldc), dtype=torch.float32, device=self.device)
        d = _lib.IsoGemmDesc()
        d.form, d.sym, d.epilogue, d.M, d.N, d.K = int(form), 1 if sym else 0, int(epilogue), M, N, K
        d.a, d.lda, d.b, d.ldb = av.data_ptr(), pitch(av), bv.data_ptr(), pitch(bv)
        if ev is not None:
            d.e, d.lde = ev.data_ptr(), pitch(ev)
        d.ca, d.cb, d.c, d.ldc = float(ca), float(cb), store.data_ptr(), ldc
        self._call(self.lib.dll.smhip_iso_gemm(self.ctx.h, C.byref(d), self._stream()))
        return store[:, :N]

    # -- WIDEN (weight disentanglement) ----------------------------------------------------------
    def widen_merge(self, finetunes: Sequence[torch.Tensor], bases: Sequence[torch.Tensor], alphas: Sequence[float],
                    base_out: torch.Tensor, *, ratio: float = 1.0, calibration: float = 1.0, lam: float = 1.0,
                    layer_name: str = "", want_stats: bool = False, want_delta: bool = False):
        """WIDEN merge of one tensor viewed as ``[shape[0], rest]`` (``smhip_widen_merge``; the function is stated in
        include/shardmerge_hip.h): per column and finetune the divergence of the column's magnitude and of its direction
        from the base's, both ranked within the finetune, the ranks turned into weights by a softmax across the finetunes
        - a column ranked above ``ratio`` times the finetune's mean rank takes ``calibration`` instead - and the deltas
        added with those per-column weights times ``alpha_i``, times ``lam``, onto ``base_out`` in its dtype.  A tensor
        whose first dimension is 1 (and a 1-D tensor) ranks the magnitudes of its delta's entries.  At most 65536
        columns.  Returns (out, WidenMergeReport[, the fp32 merged delta times ``lam``]); ``want_stats`` adds every
        column's statistics, ranks and weights to the report (CPU tensors).  A NaN or Inf in a finetune or a base raises
        ValueError naming ``layer_name`` and the finetune."""
        layer_name = layer_name or "layer"
        if not math.isfinite(float(ratio)):
            raise ValueError(f"widen_merge: ratio {ratio} is not finite")
        if not (0.0 <= float(calibration) < math.inf):
            raise ValueError(f"widen_merge: calibration {calibration} is not a finite number >= 0")
        if not math.isfinite(float(lam)):
            raise ValueError(f"widen_merge: lam {lam} is not finite")
        desc, rep, k = _lib.WidenDesc(), _lib.WidenReport(), len(finetunes)
        desc.ratio, desc.calibration, desc.lam = float(ratio), float(calibration), float(lam)
        keep, bo, out, delta = self._stage_delta_merge(desc, finetunes, bases, alphas, base_out, layer_name, want_delta, "widen_merge")
        desc.n = bo.numel()
        rows = int(bo.shape[0]) if bo.ndim >= 2 else 1
        desc.rows = rows
        cols = int(desc.n // rows) if rows else 0
        if cols > _lib.WIDEN_MAX_COLS:
            raise ValueError(f"widen_merge: {layer_name} has shape {list(bo.shape)}: {cols} columns, at most {_lib.WIDEN_MAX_COLS}")
        stat = rank = weight = None
        if want_stats:
            stat = torch.zeros((k, 2, cols), dtype=torch.float64, device=self.device)
            rank = torch.zeros((k, 2, cols), dtype=torch.int32, device=self.device)
            weight = torch.zeros((k, cols), dtype=torch.float32, device=self.device)
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
        self._run_delta_merge(self.lib.dll.smhip_widen_merge, desc, rep, out, delta, layer_name, ptr(stat), ptr(rank), ptr(weight))
        report = WidenMergeReport(rows=int(rep.rows), cols=int(rep.cols), vector_mode=bool(rep.vector_mode),
                                  mu=[[float(rep.mu[i][s]) for s in range(2)] for i in range(k)],
                                  calibrated=[[int(rep.calibrated[i][s]) for s in range(2)] for i in range(k)])
        if want_stats:
            report.stat, report.rank, report.weight = stat.cpu(), rank.cpu().to(torch.int64), weight.cpu()
        return (out, report, delta) if want_delta else (out, report)

    # -- CABS (conflict-aware, balanced n:m sparsification) -----------------------------------------
    def cabs_merge(self, finetunes: Sequence[torch.Tensor], bases: Sequence[torch.Tensor], alphas: Sequence[float],
                   base_out: torch.Tensor, *, n_keep: int, group: int, conflict_aware: bool = True, lam: float = 1.0,
                   layer_name: str = "", want_delta: bool = False, want_mask: bool = False):
        """CABS merge of one tensor viewed as rows of its last dimension (``smhip_cabs_merge``; the function is stated in
        include/shardmerge_hip.h): every group of ``group`` consecutive weights of a row keeps the ``n_keep`` largest
        magnitudes of each delta ``finetune_i - base_i`` (ties at the cut all kept), the finetunes IN THE ORDER GIVEN and,
        when ``conflict_aware``, each only where no earlier one kept an entry; the kept entries are weighted by
        ``alpha_i``, summed without normalisation, times ``lam``, added onto ``base_out`` in its dtype.  ``group`` is a
        power of two in 4..512, ``1 <= n_keep <= group``.  Returns (out, CabsReport[, the fp32 merged delta times
        ``lam``]); ``want_mask`` adds the kept bits of every element to the report.  A NaN or Inf in a delta raises
        ValueError naming ``layer_name`` and the finetune."""
        layer_name = layer_name or "layer"
        for name, v in (("n_keep", n_keep), ("group", group)):
            if isinstance(v, bool) or not isinstance(v, int):
                raise ValueError(f"cabs_merge: {name} must be an integer, not {v!r}")
        if group not in _lib.CABS_GROUPS:
            raise ValueError(f"cabs_merge: group {group} is not a power of two in 4..512")
        if not (1 <= n_keep <= group):
            raise ValueError(f"cabs_merge: n_keep {n_keep} is not in 1..{group}")
        if not math.isfinite(float(lam)):
            raise ValueError(f"cabs_merge: lam {lam} is not finite")
        desc, rep, k = _lib.CabsDesc(), _lib.CabsReport(), len(finetunes)
        desc.n_keep, desc.group, desc.conflict_aware, desc.lam = n_keep, group, 1 if conflict_aware else 0, float(lam)
        keep, bo, out, delta = self._stage_delta_merge(desc, finetunes, bases, alphas, base_out, layer_name, want_delta, "cabs_merge")
        desc.n = bo.numel()
        cols = int(bo.shape[-1]) if bo.ndim >= 1 else 1
        rows = (desc.n // cols if cols else 1) or 1
        desc.rows = rows
        mask = torch.zeros(bo.shape, dtype=torch.int16, device=self.device) if want_mask else None
        self._run_delta_merge(self.lib.dll.smhip_cabs_merge, desc, rep, out, delta, layer_name,
                              mask.data_ptr() if mask is not None and mask.numel() else None)
        report = CabsReport(n=int(desc.n), rows=int(rows), cols=cols, n_keep=n_keep, group=group, conflict_aware=bool(conflict_aware),
                            groups=int(rep.groups), kept=[int(rep.kept[i]) for i in range(k)],
                            short_groups=[int(rep.short_groups[i]) for i in range(k)],
                            surplus=[int(rep.surplus[i]) for i in range(k)], covered=int(rep.covered), overlap=int(rep.overlap))
        if want_mask:           # (uint16 values in an int16 tensor: widened here)
            report.mask = mask.to(torch.int32) & 0xFFFF
        return (out, report, delta) if want_delta else (out, report)

    # -- task-vector statistics ----------------------------------------------------------------
    def delta_stats(self, finetunes: Sequence[torch.Tensor], bases: Sequence[torch.Tensor], alphas: Sequence[float],
                    densities: Sequence[float], layer_name: Optional[str] = None) -> DeltaStatsReport:
        """Statistics of the deltas ``finetune_i - base_i`` of one tensor of any shape (``smhip_delta_stats``; the
        function is stated in include/shardmerge_hip.h), no tensor is written: their fp64 Gram and, for up to four
        candidate ``densities`` at once, every finetune's exact trim threshold, what that trim keeps in elements and
        in energy, how the kept sets overlap (``alone``, ``cover``) and what the TIES election under ``alphas`` would
        discard (``opposed``, ``conflict``).  A NaN or Inf in a delta raises ValueError naming ``layer_name`` and the
        finetune."""
        layer_name = layer_name or "layer"
        k, dens = len(finetunes), [float(x) for x in densities]
        if k < 1 or k > _lib.MAX_MODELS:
            raise ValueError(f"{k} models to analyse: supported range is 1..{_lib.MAX_MODELS}")
        if len(bases) != k or len(alphas) != k:
            raise ValueError(f"delta_stats: {k} finetunes, {len(bases)} bases, {len(alphas)} alphas")
        if not (1 <= len(dens) <= _lib.STATS_MAX_DENSITIES):
            raise ValueError(f"delta_stats: {len(dens)} densities, supported range is 1..{_lib.STATS_MAX_DENSITIES}")
        for rho in dens:
            if not (0.0 < rho <= 1.0):
                raise ValueError(f"delta_stats: density {rho} is not in (0, 1]")
        desc, rep, m = _lib.StatsDesc(), _lib.StatsReport(), len(dens)
        keep = self._stage_delta_merge(desc, finetunes, bases, alphas, None, layer_name, False)[0]
        desc.n, desc.m = keep[0].numel(), m
        for q in range(m):
            desc.density[q] = dens[q]
        try:
            self.ctx.check(self.lib.dll.smhip_delta_stats(self.ctx.h, C.byref(desc), C.byref(rep), self._stream()))
        except SmhipError as e:
            if e.code == _lib.ERR_NONFINITE:
                raise ValueError(f"Non-finite delta in {layer_name}: {e.message}") from e
            raise
        per = lambda a, cast, cols=k: [[cast(a[q][i]) for i in range(cols)] for q in range(m)]
        return DeltaStatsReport(
            n=int(desc.n), densities=dens, nonzero=[int(rep.nonzero[i]) for i in range(k)],
            gram=[[float(rep.G[i][j]) for j in range(k)] for i in range(k)],
            k_keep=[int(rep.k_keep[q]) for q in range(m)], thresholds=per(rep.tau, float), kept=per(rep.kept, int),
            energy=per(rep.energy, float), opposed=per(rep.opposed, int), alone=per(rep.alone, int),
            cover=per(rep.cover, int, k + 1), conflict=[int(rep.conflict[q]) for q in range(m)])

    def correlate_pairs(self, tensors) -> torch.Tensor:
        """K x K matrix of mean column-wise cosine similarities (reference functions.py:304-314);
        `tensors`: a stacked tensor [K, ...] or a sequence of K equally shaped tensors."""
        ts = list(tensors.unbind(0)) if isinstance(tensors, torch.Tensor) else list(tensors)
        k = len(ts)
        if k < 2 or k > 8:
            raise ValueError("correlate_pairs: 2..8 tensors")
        dtype = ts[0].dtype if ts[0].dtype in _DTYPE_CODE and all(t.dtype == ts[0].dtype for t in ts) else torch.float32
        ts = [self._dev(t, dtype) for t in ts]
        rows = ts[0].shape[0] if ts[0].ndim >= 1 else 1
        cols = ts[0].numel() // max(rows, 1)
        ptrs = (C.c_void_p * k)(*[t.data_ptr() for t in ts])
        out = (C.c_float * (k * k))()
        self._call(self.lib.dll.smhip_correlate_pairs(self.ctx.h, k, ptrs, _DTYPE_CODE[dtype], rows, cols, out, self._stream()))
        return torch.tensor(list(out), dtype=torch.float32).reshape(k, k)

    # -- A1 - A13 fused ------------------------------------------------------------------
    def merge_layer(self, finetunes: Sequence[torch.Tensor], bases: Sequence[torch.Tensor], alphas: Sequence[float],
                    base_out: torch.Tensor, target_norm_offset: float = 1e-10, cull_start_pct: float = 0.20,
                    cutoff_pct: float = 0.08, t_sum: float = 1.0, want_delta: bool = False,
                    layer_name: str = "layer", b: float = 0.1, norm_mode: Optional[str] = None):
        desc, k = LayerDesc(), len(finetunes)
        keep, bo, out, delta = self._stage_delta_merge(desc, finetunes, bases, alphas, base_out, layer_name, want_delta,
                                                       out_dtype=torch.bfloat16)
        nb, r, c = _shape3d(bo)
        desc.rows, desc.cols = r, c
        desc.target_norm_offset = float(target_norm_offset)
        desc.cull_start_pct = float(cull_start_pct)
        desc.cutoff_pct = float(cutoff_pct)
        desc.t_sum = float(t_sum)
        desc.b = float(b)
        if norm_mode is None:
            norm_mode = DEFAULT_NORM_MODE            # one default everywhere (constants.py)
        if norm_mode not in NORM_MODES:
            raise ValueError(f"norm_mode {norm_mode!r}: 'exact' or 'reference_cpu'")
        desc.norm_mode = 1 if norm_mode == "reference_cpu" else 0
        desc.batch = nb
        rep = LayerReport()
        self._call(self.lib.dll.smhip_merge_layer(self.ctx.h, C.byref(desc), out.data_ptr(),
                                                  delta.data_ptr() if delta is not None else None,
                                                  C.byref(rep), self._stream()), layer_name)
        report = LayerMergeReport(
            target_norm=rep.target_norm,
            delta_norms=[rep.delta_norm[i] for i in range(k)],
            steps=[(rep.step_x[i], rep.step_y[i], _lib.BRANCH_NAMES.get(rep.step_branch[i], "?")) for i in range(rep.n_steps)],
            infos=[BlendReport.from_c(rep.step_info[i]) for i in range(rep.n_steps)],
            nan_ifft=int(rep.nan_ifft), nan_final=int(rep.nan_final), merged_delta_norm=rep.merged_delta_norm)
        if report.nan_ifft or report.nan_final:
            logger.info(f"Warning: NaN replaced by 0 in {layer_name}: {report.nan_ifft} after ifft, {report.nan_final} after add-back")
        if want_delta:
            return out, report, delta
        return out, report


def della_arguments(density: float, epsilon: float, what: str) -> None:
    """the argument rules of smhip_della_merge (step 2), in fp64; ``what`` names the caller in the message"""
    if not (0.0 < density <= 1.0):
        raise ValueError(f"{what}: density {density} is not in (0, 1]")
    if not (epsilon >= 0.0):
        raise ValueError(f"{what}: epsilon {epsilon} must be >= 0")
    if density == 1.0:
        if epsilon != 0.0:
            raise ValueError(f"{what}: density 1 keeps everything and requires epsilon 0, not epsilon {epsilon}")
        return
    if not (density + epsilon < 1.0):
        raise ValueError(f"{what}: density {density} + epsilon {epsilon} must be below 1")
    if not (math.floor((density - epsilon) * 65536.0) >= 1):
        raise ValueError(f"{what}: floor((density - epsilon) * 65536) must be at least 1 (the mask draws 16 bits per element), "
                    f"not density {density}, epsilon {epsilon}")


_engines: Dict[str, Engine] = {}


def resolve_device(device) -> torch.device:
    """'cuda', 'cuda:1', 'cpu' (ignored with a warning: this build computes on the GPU)."""
    d = torch.device(device) if device is not None else torch.device("cuda")
    if d.type != "cuda":
        logger.warning("device=%s requested; shardmerge_amd computes on the MI355X (HIP) only - using cuda", device)
        d = torch.device("cuda")
    if d.index is None:
        d = torch.device("cuda", torch.cuda.current_device())
    return d


def get_engine(device=None) -> Engine:
    """Engine for a torch device; raises when the HIP library or a GPU is missing."""
    _lib.get_lib()                                   # fail loudly before touching torch.cuda
    if not torch.cuda.is_available():
        raise RuntimeError("no ROCm GPU visible: shardmerge_amd has no CPU path")
    d = resolve_device(device)
    key = str(d)
    if key not in _engines:
        _engines[key] = Engine(device=d)
    return _engines[key]
