"""YAML merge configuration: same keys, defaults and override rules as the
reference's shard/config.py:24-126, so existing config files work unchanged.

    output_base_model: org/base
    finetune_merge:
      - {model: org/ft1, base: org/base, alpha: 0.5, is_input: true}
      - {model: org/ft2, base: org/base, alpha: 0.3, start_layer: 2, end_layer: 30}
    output_dir: merged
    output_dtype: bfloat16      # optional
    device: cuda                # optional (this build always computes on the MI355X)
    cache_dir / storage_dir / clean_cache: optional
    merge_options:              # optional, additive: the operator's hard-coded
      cutoff_pct: 0.08          # hyper-parameters (fast_fourier.py:84-85,238-240); defaults as there
      cull_start_pct: 0.20
      t_sum: 1.0
      target_norm_offset: 1.0e-10
      b: 0.1                    # merge_tensors_fft2_slerp's linear-blend threshold (functions.py:164)
      norm_mode: reference_cpu  # reference_cpu (default: every norm as torch's CPU kernel returns it - the reference's
                                # device="cpu" output) | exact (accurate norms: the reference's device="cuda" numerics)
      operator: fourier         # fourier (default: what the reference CLI hard-wires, __main__.py:22,67)
                                # | addition | task_addition (shard/merge/addition.py, taskaddition.py)
                                # | ties (TIES-Merging, Yadav et al. 2023; no counterpart in the reference)
      density: 0.2              # operator ties only (and the spectral keys above and norm_mode are rejected with it):
      ties_lambda: 1.0          #   each delta keeps its `density` largest magnitudes (0 < density <= 1; ties at the
      ties_normalize: 1         #   threshold all kept), the merged delta is scaled by ties_lambda; ties_normalize = 1
                                #   divides the sum of the agreeing entries by the sum of their alphas, 0 leaves the sum
                                # | dare_ties | dare_linear (DARE, Yu et al. 2023; no counterpart in the reference): each
                                #   delta entry is dropped at random with probability 1 - density, the survivors rescaled
                                #   by 1 / density, then merged as ties merges (dare_ties) or added (dare_linear).  Keys,
                                #   these operators only (the spectral keys, norm_mode and the ties_* keys are rejected):
      # density: 0.2            #   2^-16 <= density <= 1; the mask draws 16 bits per element, so the density in effect
                                #   is floor(density * 65536) / 65536 (the README of the output states it)
      # dare_lambda: 1.0        #   scales the merged delta
      # dare_normalize: 1       #   1: divide by the sum of the weights (dare_ties: of the agreeing entries), 0: plain sum
      # dare_rescale: 1         #   1: survivors times 1 / effective density, 0: left as they are
      # seed: 0                 #   an integer in [0, 2^63): with the tensor's name it keys the mask, which is a function
                                #   of (seed, tensor name, position of the entry in finetune_merge, element index) - the
                                #   same config gives the same bytes in one process, in place and on any number of ranks
                                # | breadcrumbs | breadcrumbs_ties (Model Breadcrumbs, Davari & Belilovsky 2023; no
                                #   counterpart in the reference): each delta loses its `gamma` share of LARGEST magnitudes
                                #   and keeps the next `density` share (the small rest is dropped as ties drops it; ties at
                                #   either threshold all kept), then the weighted deltas are added (breadcrumbs) or merged
                                #   as ties merges (breadcrumbs_ties).  Keys, these operators only (the spectral keys,
                                #   norm_mode, task_add_models, ties_*, dare_* and seed are rejected):
      # density: 0.9            #   0 < density <= 1
      # gamma: 0.01             #   0 <= gamma < 1, density + gamma <= 1
      # breadcrumbs_lambda: 1.0 #   scales the merged delta
      # breadcrumbs_normalize: 1  # 1: divide by the sum of the weights (breadcrumbs_ties: of the agreeing entries), 0: plain sum
                                # | model_stock | nuslerp | slerp (the geometric operators; no counterpart in the reference):
                                #   the coefficients come from the norms of the deltas and the angles between them, summed in
                                #   fp64 in a fixed order.  model_stock (Jang et al. 2024): the alpha-weighted average of the
                                #   deltas, pulled towards the base by t = k cos / (1 + (k - 1) cos), cos the mean cosine
                                #   between them.  nuslerp: exactly two finetune_merge entries, alphas >= 0 with a sum > 0; the
                                #   deltas' directions are interpolated on the sphere at alpha_1 / (alpha_0 + alpha_1), their
                                #   lengths linearly.  slerp: the same interpolation of the two models' WEIGHTS (the bases and
                                #   output_base_model do not enter a block tensor).  Every key above is rejected; the one key:
      # stock_filter_wise: 0    #   operator model_stock only - 1: one cosine, one t per ROW of each tensor, 0: per tensor
                                # | sce (SCE, Wan et al. 2024, mergekit's merge_method sce; no counterpart in the reference):
                                #   per tensor, the parameters whose deltas vary most across the finetunes are selected, each
                                #   finetune is weighted by alpha times the energy (sum of squares) of its selected entries,
                                #   normalised over the finetunes, and the entries whose sign disagrees with the majority are
                                #   erased.  alphas >= 0 with a sum > 0 (an alpha is a prior on the weight, not a scale of
                                #   the delta).  Every key above is rejected; its keys, this operator only:
      # select_topk: 1.0        #   0 < select_topk <= 1: the share of the nonzero variances that is selected (ties at the
                                #   threshold all kept); 1: everything (mergekit's name and default)
      # sce_lambda: 1.0         #   scales the merged delta
                                # | della | della_linear (DELLA, Deep et al. 2024, mergekit's della / della_linear; no
                                #   counterpart in the reference): dare_ties / dare_linear whose keep probability rises
                                #   with the rank of the entry's magnitude within its row (the tensor's last dimension), from
                                #   density - epsilon for the smallest to density + epsilon for the largest; equal
                                #   magnitudes share a rank; a survivor is rescaled by the inverse of its own probability.
                                #   Rows of more than 32768 elements are an error.  The spectral keys, norm_mode,
                                #   task_add_models and every other family's keys are rejected; its keys:
      # density: 0.5            #   0 < density <= 1; density 1 requires epsilon 0
      # epsilon: 0.15           #   >= 0, density + epsilon < 1 and floor((density - epsilon) * 65536) >= 1 (the mask draws
                                #   16 bits per element); 0: dare_ties / dare_linear bit for bit
      # della_lambda: 1.0       #   scales the merged delta
      # della_normalize: 1      #   1: divide by the sum of the weights (della: of the agreeing entries), 0: plain sum
      # della_rescale: 1        #   1: survivors times 1 / their effective probability, 0: left as they are
      # seed: 0                 #   as with dare_ties: an integer in [0, 2^63)
                                # | consensus_ta | consensus_ties (Consensus Merging with TALL masks, Wang et al. 2024; no
                                #   counterpart in the reference): the weighted deltas are added (consensus_ta) or merged as
                                #   ties merges (consensus_ties) into a multi-task vector; a finetune's mask is set where its
                                #   own weighted entry is at least mask_lambda times what the others did to the same weight;
                                #   an element of the multi-task vector is kept where at least consensus_k masks are set.  The
                                #   spectral keys, norm_mode, task_add_models and every other family's keys are rejected; keys:
      # mask_lambda: 0.4        #   0 <= mask_lambda <= 1e6; 0 sets every mask
      # consensus_k: 2          #   an integer in 1..16: masks that must agree (all of them where fewer finetunes cover a tensor)
      # consensus_lambda: 1.0   #   scales the merged delta
      # consensus_normalize: 1  #   1: divide by the sum of the weights (consensus_ties: of the agreeing entries), 0: plain sum
      # density: 0.2            #   operator consensus_ties only: the trim of ties, 0 < density <= 1
                                # | karcher | multislerp (Karcher means; no counterpart in the reference): slerp / nuslerp for
                                #   any number of finetune_merge entries (1..16).  The DIRECTIONS of the vectors - karcher: the
                                #   models' weights, as slerp; multislerp: the deltas, as nuslerp - are averaged on the sphere
                                #   with the weights alpha_i / sum alpha (the log map iterated to its fixed point, on the fp64
                                #   Gram matrix), their LENGTHS linearly.  alphas >= 0 with a sum > 0.  The spectral keys,
                                #   norm_mode, task_add_models and every other family's keys are rejected; keys:
      # karcher_max_iter: 10    #   an integer in 1..100: iterations at most (two entries need one)
      # karcher_tol: 1.0e-5     #   0 <= karcher_tol < 1: the iteration stops when its step on the sphere is shorter
      # sphere_row_wise: 0      #   1: one mean per ROW of each tensor (multislerp with two entries: row-wise nuslerp), 0: per tensor
                                # | arcee_fusion | nearswap (the pairwise operators, after mergekit's methods of those names; no
                                #   counterpart in the reference): ONE model is grafted onto its base, element by element, so
                                #   every block tensor must be covered by EXACTLY ONE finetune_merge entry (entries with
                                #   disjoint layer windows fuse different models into different layers; two entries on one
                                #   layer are an error before anything is written).  They take no weight: an entry alpha other
                                #   than 1 is rejected.  arcee_fusion: a row of a tensor (its last dimension) is scored by the
                                #   KL divergence of its softmax in the model from its softmax in the base, an element by
                                #   |delta| times its row's score, and the delta is taken only where that exceeds
                                #   median + fusion_iqr * (Q3 - Q1) of the tensor's scores.  nearswap: the delta is clamped to
                                #   [-nearswap_t, nearswap_t].  The spectral keys, norm_mode, task_add_models and every other
                                #   family's keys are rejected; keys:
      # fusion_iqr: 1.5         #   operator arcee_fusion only: -1e6 <= fusion_iqr <= 1e6 (mergekit's 1.5)
      # nearswap_t: 0.001       #   operator nearswap only, REQUIRED: 0 < nearswap_t <= 1e6
                                # | pcb (PCB-Merging, Du et al. 2024; no counterpart in the reference): every entry of every
                                #   weighted delta gets a continuous score - its magnitude within its own finetune (clamped
                                #   at both ends, min-max normalised, through exp) times its agreement with the sum of all
                                #   deltas at that weight (through tanh; an entry that opposes the sum scores 0) - each
                                #   finetune keeps its pcb_ratio highest scores per tensor, and the clamped entries are
                                #   averaged with their rescaled scores as weights.  alphas of any sign.  The spectral keys,
                                #   norm_mode, task_add_models and every other family's keys are rejected; keys:
      # pcb_ratio: 0.1          #   0 < pcb_ratio <= 1: the share of each finetune's scores that is kept
      # pcb_clip: 0.0001        #   0 <= pcb_clip < 0.5: the share of magnitudes clamped at either end
      # pcb_lambda: 1.0         #   scales the merged delta
                                # | tsv (TSV-Merge, Gargiulo et al. 2025; no counterpart in the reference): a block tensor's
                                #   delta is taken as a MATRIX ([shape[0] x the rest]): its tsv_rank leading singular
                                #   triplets by a randomized subspace iteration, the singular vectors of all covering
                                #   finetunes whitened together so that overlapping subspaces count once, the delta rebuilt
                                #   with the singular values times alpha.  1-D tensors and tensors one entry covers take the
                                #   normalised weighted mean of their deltas (dare_linear at density 1) times tsv_lambda.
                                #   alphas >= 0 with a sum > 0.  A layer whose k covering entries give
                                #   k * min(tsv_rank, rows, cols) > 256 is an error before anything is written.  The
                                #   spectral keys, norm_mode, task_add_models and every other family's keys are rejected; keys:
      # tsv_rank: 64            #   an integer in 1..256: singular triplets kept per finetune
      # tsv_power_iters: 2      #   an integer in 0..4: power steps of the subspace iteration
      # tsv_lambda: 1.0         #   scales the merged delta
      # seed: 0                 #   an integer in [0, 2^63): keys the sketch with the tensor's name (no position enters)
                                # | widen (WIDEN, Yu et al. 2024; no counterpart in the reference): a block tensor is taken as
                                #   a MATRIX ([shape[0] x the rest]) and weighed per COLUMN (per input feature of a Linear
                                #   weight): how far each finetune moved the column's magnitude and its direction, both
                                #   RANKED within the finetune (so a delta a hundred times larger ranks the same), the ranks
                                #   turned into weights by a softmax across the covering finetunes; a column ranked above
                                #   widen_ratio times its finetune's mean rank takes widen_calibration instead.  A tensor
                                #   whose first dimension is 1 (norm weights) ranks the magnitudes of its delta's entries.
                                #   alphas of any sign.  A block tensor with more than 65536 columns is an error before
                                #   anything is written.  The spectral keys, norm_mode, task_add_models and every other
                                #   family's keys are rejected; keys:
      # widen_ratio: 1.0        #   -1e6 <= widen_ratio <= 1e6: the cut, in units of the mean rank (below 0: every column)
      # widen_calibration: 1.0  #   0 <= widen_calibration <= 1e6: the score of a column above the cut
      # widen_lambda: 1.0       #   scales the merged delta
                                # | cabs (CABS, Yang et al. 2025; no counterpart in the reference): n:m sparsification of the
                                #   deltas - every group of cabs_m consecutive weights of a ROW (the last dimension) keeps
                                #   the cabs_n largest magnitudes of a finetune's delta (ties at the cut all kept), so the
                                #   budget is spent evenly over the tensor - applied to the covering finetunes ONE AFTER
                                #   ANOTHER IN THE ORDER OF finetune_merge, each allowed only the positions that no earlier
                                #   one kept (cabs_conflict_aware: 1), so the kept sets are disjoint; the sparse deltas are
                                #   added with their alphas, without normalisation.  alphas of any sign.  The spectral keys,
                                #   norm_mode, task_add_models and every other family's keys are rejected; keys:
      # cabs_n: 64              #   an integer in 1..cabs_m: magnitudes kept per group and finetune
      # cabs_m: 256             #   a power of two in 4..512: the group (64:256 keeps a quarter)
      # cabs_conflict_aware: 1  #   1: later finetunes take only what is left; 0: every finetune is pruned on its own
      # cabs_lambda: 1.0        #   scales the merged delta
                                # | iso_c (Iso-C, Marczak et al. 2025; no counterpart in the reference): a block tensor's
                                #   deltas are summed with their alphas into ONE task matrix ([shape[0] x the rest]) whose
                                #   singular values are all replaced by their mean, the singular vectors kept: every
                                #   direction any finetune moved gets the same weight.  No SVD is taken: the polar factor
                                #   comes from a Newton-Schulz iteration on an fp32 MFMA GEMM.  1-D tensors take the
                                #   normalised weighted mean of their deltas (dare_linear at density 1) times iso_lambda.
                                #   alphas of any sign.  A block tensor with min(rows, cols) > 16384 is an error before
                                #   anything is written.  The spectral keys, norm_mode, task_add_models and every other
                                #   family's keys are rejected; keys:
      # iso_lambda: 1.0         #   scales the merged delta
      # iso_tol: 0.0001         #   0 < iso_tol <= 1: the iteration stops at ||X X^T - I||_F / sqrt(min(rows, cols)) <= iso_tol
      # iso_max_iter: 40        #   an integer in 0..200: steps at most (reaching it is reported, not an error)
                                # | emr (EMR-Merging, Huang et al. 2024; no counterpart in the reference): the UNIFIED model -
                                #   per element the deltas are summed, the sign of the sum is elected (a zero sum elects
                                #   plus), and the entry of that sign with the largest magnitude is taken as it is.  It takes
                                #   no weight: an entry alpha other than 1 is rejected.  A task's 1-bit mask and its rescaler
                                #   are computed afterwards by `python -m shard emr-task` from the finetune, its base and the
                                #   merged model.  The spectral keys, norm_mode, task_add_models and every other family's keys
                                #   are rejected; the one key:
      # emr_lambda: 1.0         #   scales the elected delta

A finetune_merge `model` may also name a LoRA adapter directory (adapter_config.json +
adapter_model.safetensors, no model.safetensors.index.json): the entry then stands for
base + s * lora_B @ lora_A applied to its own `base` (shardmerge_amd/adapter.py): embedding LoRA
factors transposed, DoRA (use_dora) rows rescaled to their magnitude vector.  Same keys; no new
option.  Or a delta pack directory (delta_config.json + delta_model.safetensors, written by
`python -m shard compress-delta`): the entry then stands for its `base` plus or minus a scale per
row where the pack's planes keep an element (shardmerge_amd/deltapack.py).  Same keys; no new option.  Or an EMR pack
directory (emr_config.json + emr_model.safetensors, written by `python -m shard emr-task`): the entry then stands for
its `base` moved towards the pack's unified model by the pack's rescaler where the pack's mask is set
(shardmerge_amd/emrpack.py).  Same keys; no new option.
"""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass, field
from pathlib import Path
from typing import Any, Callable, Dict, List, Optional, Union

import click
import torch
import yaml

from .constants import DEFAULT_NORM_MODE, NORM_MODES

_REQUIRED = ("output_base_model", "finetune_merge", "output_dir")
# the FFT operator's hyper-parameters and the values the reference hard-codes for them
MERGE_OPTION_DEFAULTS = {"cutoff_pct": 0.08, "cull_start_pct": 0.20, "t_sum": 1.0, "target_norm_offset": 1e-10, "b": 0.1}
MERGE_OPTION_RANGES = {"cutoff_pct": (0.0, 1.0), "cull_start_pct": (0.0, 1.0), "t_sum": (-1e6, 1e6), "target_norm_offset": (0.0, 1e6),
                       "b": (0.0, 1e6)}
OPERATORS = ("fourier", "addition", "task_addition", "fourier_legacy", "ties", "dare_ties", "dare_linear", "breadcrumbs", "breadcrumbs_ties",
             "model_stock", "nuslerp", "slerp", "sce", "della", "della_linear", "consensus_ta", "consensus_ties",
             "karcher", "multislerp", "arcee_fusion", "nearswap", "pcb", "tsv", "widen", "cabs", "iso_c", "emr")
# The delta-merge operator families: ties, DARE, Model Breadcrumbs.  A family's keys are accepted with its operators only
# (all of them but consensus_ta take `density`), seed and consensus_k stay ints (they must survive exactly), every
# other value becomes a float.
TIES_OPTION_DEFAULTS = {"density": 0.2, "ties_lambda": 1.0, "ties_normalize": 1.0}
DARE_OPERATORS = ("dare_ties", "dare_linear")
DARE_OPTION_DEFAULTS = {"density": 0.2, "dare_lambda": 1.0, "dare_normalize": 1.0, "dare_rescale": 1.0, "seed": 0}
DARE_MIN_DENSITY = 2.0 ** -16                       # the mask draws 16 bits per element
BREADCRUMBS_OPERATORS = ("breadcrumbs", "breadcrumbs_ties")
BREADCRUMBS_OPTION_DEFAULTS = {"density": 0.9, "gamma": 0.01, "breadcrumbs_lambda": 1.0, "breadcrumbs_normalize": 1.0}
GEO_OPERATORS = ("model_stock", "nuslerp", "slerp")      # the geometric family: coefficients from norms and angles
GEO_PAIR_OPERATORS = ("nuslerp", "slerp")                # ... of exactly two finetune_merge entries
GEO_OPTION_DEFAULTS = {"stock_filter_wise": 0.0}
SCE_OPTION_DEFAULTS = {"select_topk": 1.0, "sce_lambda": 1.0}
DELLA_OPERATORS = ("della", "della_linear")
DELLA_OPTION_DEFAULTS = {"density": 0.5, "epsilon": 0.15, "della_lambda": 1.0, "della_normalize": 1.0, "della_rescale": 1.0, "seed": 0}
CONSENSUS_OPERATORS = ("consensus_ta", "consensus_ties")
CONSENSUS_OPTION_DEFAULTS = {"density": 0.2, "mask_lambda": 0.4, "consensus_k": 2, "consensus_lambda": 1.0, "consensus_normalize": 1.0}
SPHERE_OPERATORS = ("karcher", "multislerp")             # Karcher means: slerp / nuslerp for any number of entries
SPHERE_OPTION_DEFAULTS = {"karcher_max_iter": 10, "karcher_tol": 1e-5, "sphere_row_wise": 0.0}
FUSION_OPERATORS = ("arcee_fusion", "nearswap")          # the pairwise family: one model onto its base, no weights
FUSION_OPTION_DEFAULTS = {"fusion_iqr": 1.5, "nearswap_t": None}      # nearswap_t has no default: it is required
PCB_OPTION_DEFAULTS = {"pcb_ratio": 0.1, "pcb_clip": 0.0001, "pcb_lambda": 1.0}
TSV_OPTION_DEFAULTS = {"tsv_rank": 64, "tsv_power_iters": 2, "tsv_lambda": 1.0, "seed": 0}
WIDEN_OPERATORS = ("widen",)
WIDEN_OPTION_DEFAULTS = {"widen_ratio": 1.0, "widen_calibration": 1.0, "widen_lambda": 1.0}
CABS_OPERATORS = ("cabs",)
CABS_OPTION_DEFAULTS = {"cabs_n": 64, "cabs_m": 256, "cabs_conflict_aware": 1.0, "cabs_lambda": 1.0}
CABS_GROUPS = (4, 8, 16, 32, 64, 128, 256, 512)     # cabs_m: a group is selected inside one work-group
WIDEN_MAX_COLS = 65536                              # columns of a block tensor at most: the ranks are counted over all pairs
ISO_OPERATORS = ("iso_c",)
ISO_OPTION_DEFAULTS = {"iso_lambda": 1.0, "iso_tol": 1e-4, "iso_max_iter": 40}
ISO_MAX_S = 16384                                   # min(rows, cols) of a block tensor at most
EMR_OPERATORS = ("emr",)                            # the elected unified model; it takes no weights
EMR_OPTION_DEFAULTS = {"emr_lambda": 1.0}
TSV_MAX_VECTORS = 256                               # k * min(tsv_rank, rows, cols) at most: the width of the whitened panels


def _breadcrumbs_band(opts: Dict[str, Any]) -> None:
    density = float(opts.get("density", BREADCRUMBS_OPTION_DEFAULTS["density"]))
    gamma = float(opts.get("gamma", BREADCRUMBS_OPTION_DEFAULTS["gamma"]))
    if not (density + gamma <= 1.0):
        raise click.BadParameter(f"merge_options.density + merge_options.gamma must not exceed 1 (density {density:g}, gamma {gamma:g}): "
                                 "the dropped top and the kept band cannot overlap")


def della_thresholds(density: float, epsilon: float, cols: int = 2):
    """(T_lo, T_hi) of smhip_della_merge, step 4 in fp64: the thresholds of rank 0 and of rank cols - 1"""
    if density == 1:
        return 65536, 65536
    if epsilon == 0:
        return (int(float(density) * 65536.0),) * 2
    p_lo, w = float(density) - float(epsilon), 2.0 * float(epsilon)
    t = lambda r: min(int((p_lo + (w * float(r)) / float(cols - 1) if cols > 1 else p_lo) * 65536.0), 65535)
    return t(0), t(cols - 1)


def _della_window(opts: Dict[str, Any]) -> None:
    """the argument rules of smhip_della_merge (include/shardmerge_hip.h, step 2), in fp64"""
    density = float(opts.get("density", DELLA_OPTION_DEFAULTS["density"]))
    epsilon = float(opts.get("epsilon", DELLA_OPTION_DEFAULTS["epsilon"]))
    if density == 1.0:
        if epsilon != 0.0:
            raise click.BadParameter(f"merge_options.density 1 keeps everything and requires merge_options.epsilon 0 (epsilon {epsilon:g})")
        return
    if not (density + epsilon < 1.0):
        raise click.BadParameter(f"merge_options.density + merge_options.epsilon must be below 1 (density {density:g}, epsilon {epsilon:g}): "
                                 "the largest magnitude of a row is kept with probability density + epsilon")
    if not (int((density - epsilon) * 65536.0) >= 1):
        raise click.BadParameter(f"floor((merge_options.density - merge_options.epsilon) * 65536) must be at least 1 (density {density:g}, "
                                 f"epsilon {epsilon:g}): the mask draws 16 bits per element")


def _cabs_n_of_m(opts: Dict[str, Any]) -> None:
    """the argument rules of smhip_cabs_merge (include/shardmerge_hip.h): the group a power of two, 1 <= n <= m"""
    n, m = opts.get("cabs_n", CABS_OPTION_DEFAULTS["cabs_n"]), opts.get("cabs_m", CABS_OPTION_DEFAULTS["cabs_m"])
    if m not in CABS_GROUPS:
        raise click.BadParameter(f"merge_options.cabs_m must be a power of two in 4..512, not {m}")
    if not (1 <= n <= m):
        raise click.BadParameter(f"merge_options.cabs_n must be an integer in 1..cabs_m = {m}, not {n}")


@dataclass(frozen=True)
class _OptionFamily:
    """One family's merge_options.  rules: key -> "flag" (0 or 1), "seed" (an exact integer in [0, 2^63)), ("int", lo, hi)
    (an exact integer in lo..hi, kept an int) or a range (lo, hi, brackets[, the message's own wording of the range]).
    earlier: what the message says after a key of an earlier family, by that family's first operator.  only: a key that
    not every operator of the family takes.  required: keys that have no default.  check: a rule over several keys."""
    operators: tuple
    defaults: Dict[str, Union[int, float]]
    rules: Dict[str, Any]
    earlier: Dict[str, str] = field(default_factory=dict)
    only: Dict[str, tuple] = field(default_factory=dict)        # key -> the operators of the family that take it (default: all)
    required: tuple = ()                                        # keys without a default: the operators that take them must give them
    check: Optional[Callable[[Dict[str, Any]], None]] = None


_DENSITY, _LAMBDA = (0, 1, "(]"), (-1e6, 1e6, "[]")
_OPTION_FAMILIES = (                                # in the order they were added: a later family knows the earlier ones
    _OptionFamily(("ties",), TIES_OPTION_DEFAULTS, {"density": _DENSITY, "ties_lambda": _LAMBDA, "ties_normalize": "flag"}),
    _OptionFamily(DARE_OPERATORS, DARE_OPTION_DEFAULTS,
                  {"density": (DARE_MIN_DENSITY, 1, "[]", f"[2^-16 = {DARE_MIN_DENSITY}, 1] with operator {{operator}} (the mask draws 16 bits per element)"),
                   "dare_lambda": _LAMBDA, "dare_normalize": "flag", "dare_rescale": "flag", "seed": "seed"},
                  earlier={"ties": "(its keys: dare_lambda, dare_normalize)"}),
    _OptionFamily(BREADCRUMBS_OPERATORS, BREADCRUMBS_OPTION_DEFAULTS,
                  {"density": _DENSITY, "gamma": (0, 1, "[)"), "breadcrumbs_lambda": _LAMBDA, "breadcrumbs_normalize": "flag"},
                  earlier={"ties": "(its keys: breadcrumbs_lambda, breadcrumbs_normalize)", "dare_ties": "(its trim is by magnitude, not random)"},
                  check=_breadcrumbs_band),
    _OptionFamily(GEO_OPERATORS, GEO_OPTION_DEFAULTS, {"stock_filter_wise": "flag"},
                  earlier={"ties": "(it trims nothing and scales by the deltas' geometry)", "dare_ties": "(it drops nothing)",
                           "breadcrumbs": "(it trims nothing)"},
                  only={"stock_filter_wise": ("model_stock",)}),
    _OptionFamily(("sce",), SCE_OPTION_DEFAULTS, {"select_topk": (0, 1, "(]"), "sce_lambda": _LAMBDA},
                  earlier={"ties": "(its keys: select_topk, sce_lambda)", "dare_ties": "(it drops nothing at random)",
                           "breadcrumbs": "(it selects by the variance across the finetunes, not by magnitude)",
                           "model_stock": "(its weights come from the energies, per tensor)"}),
    _OptionFamily(DELLA_OPERATORS, DELLA_OPTION_DEFAULTS,
                  {"density": _DENSITY, "epsilon": (0, 1, "[)"), "della_lambda": _LAMBDA, "della_normalize": "flag", "della_rescale": "flag",
                   "seed": "seed"},
                  earlier={"ties": "(its keys: della_lambda, della_normalize)", "dare_ties": "(its keys: della_lambda, della_normalize, della_rescale)",
                           "breadcrumbs": "(its drop is random, by the rank of the magnitude within the row)",
                           "model_stock": "(it drops at random and weights by alpha)", "sce": "(it selects nothing by variance)"},
                  check=_della_window),
    _OptionFamily(CONSENSUS_OPERATORS, CONSENSUS_OPTION_DEFAULTS,
                  {"density": _DENSITY, "mask_lambda": (0, 1e6, "[]"), "consensus_k": ("int", 1, 16), "consensus_lambda": _LAMBDA,
                   "consensus_normalize": "flag"},
                  earlier={"ties": "(its keys: consensus_lambda, consensus_normalize)", "dare_ties": "(it drops nothing at random)",
                           "breadcrumbs": "(it drops by the agreement of the masks, not by magnitude)",
                           "model_stock": "(it weights by alpha and drops by the agreement of the masks)",
                           "sce": "(it selects by the agreement of the masks, not by variance)",
                           "della": "(it drops nothing at random)"},
                  only={"density": ("consensus_ties",)}),
    _OptionFamily(SPHERE_OPERATORS, SPHERE_OPTION_DEFAULTS,
                  {"karcher_max_iter": ("int", 1, 100), "karcher_tol": (0, 1, "[)"), "sphere_row_wise": "flag"},
                  earlier={"ties": "(it trims nothing and averages directions on the sphere)", "dare_ties": "(it drops nothing)",
                           "breadcrumbs": "(it trims nothing)",
                           "model_stock": "(its granularity key is sphere_row_wise)",
                           "sce": "(its weights are the alphas, not energies)",
                           "della": "(it drops nothing at random)",
                           "consensus_ta": "(it masks nothing)"}),
    _OptionFamily(FUSION_OPERATORS, FUSION_OPTION_DEFAULTS,
                  {"fusion_iqr": (-1e6, 1e6, "[]"), "nearswap_t": (0, 1e6, "(]")},
                  earlier={"ties": "(it trims by an importance score or clamps, and takes no weight)", "dare_ties": "(it drops nothing at random)",
                           "breadcrumbs": "(it trims by an importance score or clamps)",
                           "model_stock": "(it fuses one model, row scores come from the softmax)",
                           "sce": "(it fuses one model: nothing varies across finetunes)",
                           "della": "(it drops nothing at random)",
                           "consensus_ta": "(it fuses one model: no masks to agree)"},
                  only={"fusion_iqr": ("arcee_fusion",), "nearswap_t": ("nearswap",)}, required=("nearswap_t",)),
    _OptionFamily(("pcb",), PCB_OPTION_DEFAULTS,
                  {"pcb_ratio": (0, 1, "(]"), "pcb_clip": (0, 0.5, "[)"), "pcb_lambda": _LAMBDA},
                  earlier={"ties": "(its keys: pcb_ratio, pcb_lambda)", "dare_ties": "(it drops nothing at random)",
                           "breadcrumbs": "(it clamps the largest magnitudes and drops by score: pcb_clip, pcb_ratio)",
                           "model_stock": "(its weights are per element, from the scores)",
                           "sce": "(it selects by score, per finetune: pcb_ratio)",
                           "della": "(it drops nothing at random)",
                           "consensus_ta": "(it weighs by agreement with the sum, without masks)",
                           "arcee_fusion": "(it merges several models by their scores)"}),
    _OptionFamily(("tsv",), TSV_OPTION_DEFAULTS,
                  {"tsv_rank": ("int", 1, 256), "tsv_power_iters": ("int", 0, 4), "tsv_lambda": _LAMBDA, "seed": "seed"},
                  earlier={"ties": "(it truncates by singular value, not by magnitude: tsv_rank, tsv_lambda)",
                           "dare_ties": "(it drops nothing at random; its seed keys the sketch)",
                           "breadcrumbs": "(it truncates by singular value, not by magnitude)",
                           "model_stock": "(it whitens singular vectors and weights by alpha)",
                           "sce": "(it selects singular triplets, not entries: tsv_rank)",
                           "della": "(it drops nothing at random)",
                           "consensus_ta": "(it masks nothing)",
                           "arcee_fusion": "(it merges several models by their singular vectors)"}),
    _OptionFamily(WIDEN_OPERATORS, WIDEN_OPTION_DEFAULTS,
                  {"widen_ratio": (-1e6, 1e6, "[]"), "widen_calibration": (0, 1e6, "[]"), "widen_lambda": _LAMBDA},
                  earlier={"ties": "(it trims nothing and weighs by column: widen_ratio, widen_lambda)",
                           "dare_ties": "(it drops nothing at random)",
                           "breadcrumbs": "(it trims nothing)",
                           "model_stock": "(its weights are per column, from the ranks)",
                           "sce": "(it selects nothing: every column gets a weight)",
                           "della": "(it drops nothing at random; its ranks are per column, not per entry)",
                           "consensus_ta": "(it masks nothing)",
                           "arcee_fusion": "(it merges several models by their columns' ranks)"}),
    _OptionFamily(CABS_OPERATORS, CABS_OPTION_DEFAULTS,
                  {"cabs_n": ("int", 1, 512), "cabs_m": ("int", 4, 512), "cabs_conflict_aware": "flag", "cabs_lambda": _LAMBDA},
                  earlier={"ties": "(its trim is n:m within groups of a row: cabs_n, cabs_m, cabs_lambda)",
                           "dare_ties": "(it drops nothing at random)",
                           "breadcrumbs": "(it trims n:m within groups of a row and never the largest)",
                           "model_stock": "(it weights by alpha and sparsifies n:m)",
                           "sce": "(it selects by magnitude within groups, per finetune)",
                           "della": "(it drops nothing at random)",
                           "consensus_ta": "(it masks by order: earlier finetunes keep their positions)",
                           "arcee_fusion": "(it merges several models by n:m sparsification)"},
                  check=_cabs_n_of_m),
    _OptionFamily(ISO_OPERATORS, ISO_OPTION_DEFAULTS,
                  {"iso_lambda": _LAMBDA, "iso_tol": (0, 1, "(]"), "iso_max_iter": ("int", 0, 200)},
                  earlier={"ties": "(it trims nothing and flattens the spectrum of the summed delta: iso_lambda)",
                           "dare_ties": "(it drops nothing at random)",
                           "breadcrumbs": "(it trims nothing)",
                           "model_stock": "(it weights by alpha and flattens the spectrum of the sum)",
                           "sce": "(it selects nothing: every singular direction gets the mean singular value)",
                           "della": "(it drops nothing at random)",
                           "consensus_ta": "(it masks nothing)",
                           "arcee_fusion": "(it merges several models by the spectrum of their summed delta)"}),
    _OptionFamily(EMR_OPERATORS, EMR_OPTION_DEFAULTS, {"emr_lambda": _LAMBDA},
                  earlier={"ties": "(it trims nothing and takes the largest agreeing entry: emr_lambda)",
                           "dare_ties": "(it drops nothing at random)",
                           "breadcrumbs": "(it trims nothing)",
                           "model_stock": "(it takes no weights and elects one entry per element)",
                           "sce": "(it selects nothing by variance)",
                           "della": "(it drops nothing at random)",
                           "consensus_ta": "(its masks are per task, computed by emr-task afterwards)",
                           "arcee_fusion": "(it merges several models by election)"}),
)


def _one_of(names) -> str:
    return names[0] if len(names) == 1 else f"{', '.join(names[:-1])} or {names[-1]}"


def _family_options(opts: Dict[str, Any], norm_mode: str, task_add: List[str], operator: str) -> Optional[Dict[str, Union[int, float]]]:
    """merge_options of a delta-merge operator: its family's keys only - an option the operator would ignore is an
    error that names it.  None for an operator of no family, once the families' keys are ruled out."""
    own = next((i for i, f in enumerate(_OPTION_FAMILIES) if operator in f.operators), -1)
    for i in reversed(range(own + 1, len(_OPTION_FAMILIES))):          # the families added after the operator's, the latest first
        new = set(_OPTION_FAMILIES[i].defaults).difference(*(e.defaults for e in _OPTION_FAMILIES[:i]))    # the keys it brought
        for key in sorted(set(opts) & new):
            names = [op for f in _OPTION_FAMILIES if new & set(f.defaults) for op in f.only.get(key, f.operators)]
            raise click.BadParameter(f"merge_options.{key} is accepted only with operator: {_one_of(names)} "
                                     f"(operator {operator!r} would ignore it)")
    if own < 0:
        return None
    fam = _OPTION_FAMILIES[own]
    if task_add:
        raise click.BadParameter(f"merge_options.task_add_models is an option of operator fourier_legacy; operator {operator!r} would ignore it")
    for key in sorted(set(opts) & set(MERGE_OPTION_DEFAULTS)):
        raise click.BadParameter(f"merge_options.{key} is an option of the spectral operators; operator {operator!r} would ignore it")
    if norm_mode != DEFAULT_NORM_MODE:
        raise click.BadParameter(f"merge_options.norm_mode is an option of the spectral operators; operator {operator!r} takes no norm")
    for e in _OPTION_FAMILIES[:own]:
        for key in sorted((set(opts) & set(e.defaults)) - set(fam.defaults)):
            if e.operators[0] not in fam.earlier:          # no remark of this family on that one: the plain wording
                raise click.BadParameter(f"merge_options.{key} is accepted only with operator: {_one_of(e.only.get(key, e.operators))} "
                                         f"(operator {operator!r} would ignore it)")
            raise click.BadParameter(f"merge_options.{key} is an option of operator{'s' if len(e.operators) > 1 else ''} {' / '.join(e.operators)}; "
                                     f"operator {operator!r} would ignore it {fam.earlier[e.operators[0]]}")
    for key in sorted(k for k in set(opts) & set(fam.only) if operator not in fam.only[k]):
        raise click.BadParameter(f"merge_options.{key} is accepted only with operator: {_one_of(fam.only[key])} "
                                 f"(operator {operator!r} would ignore it)")
    unknown = set(opts) - set(fam.defaults)
    if unknown:
        raise click.BadParameter(f"merge_options: unknown keys {sorted(unknown)}; known with operator {operator}: {sorted(fam.defaults) + ['operator']}")
    out: Dict[str, Union[int, float]] = {}
    for key, value in opts.items():
        rule = fam.rules[key]
        number = isinstance(value, (int, float)) and not isinstance(value, bool)
        if rule == "seed":
            if not isinstance(value, int) or isinstance(value, bool) or not (0 <= value < 2 ** 63):
                raise click.BadParameter(f"merge_options.{key} must be an integer in [0, 2^63)")
            out[key] = int(value)
            continue
        if rule[0] == "int":
            if not isinstance(value, int) or isinstance(value, bool) or not (rule[1] <= value <= rule[2]):
                raise click.BadParameter(f"merge_options.{key} must be an integer in {rule[1]}..{rule[2]}")
            out[key] = int(value)
            continue
        if rule == "flag":
            if not number or float(value) not in (0.0, 1.0):
                raise click.BadParameter(f"merge_options.{key} must be 0 or 1")
        else:
            lo, hi, (left, right) = rule[:3]
            text = rule[3].format(operator=operator) if len(rule) > 3 else f"{left}{lo}, {hi}{right}"
            if not number or not (lo <= float(value) <= hi) or (left == "(" and value == lo) or (right == ")" and value == hi):
                raise click.BadParameter(f"merge_options.{key} must be a number in {text}")
        out[key] = float(value)
    for key in fam.required:
        if operator in fam.only.get(key, fam.operators) and key not in opts:
            raise click.BadParameter(f"merge_options.{key} is required with operator {operator} (it has no default)")
    if fam.check:
        fam.check(opts)
    return out


@dataclass
class MergeModel:
    """One finetune taking part in the merge (reference config.py:24-40)."""
    model: str
    base: str
    alpha: float = 1.0
    is_input: bool = False      # provides model.embed_tokens.weight
    is_output: bool = False     # provides model.norm.weight / lm_head.weight
    is_norm: bool = False       # parsed for compatibility; the reference never reads it
    start_layer: int = 0
    end_layer: int = -1         # -1: no upper bound

    def use_layer_index(self, layer_index: int) -> bool:
        below = layer_index < self.start_layer
        above = self.end_layer != -1 and layer_index > self.end_layer
        return not (below or above)


@dataclass
class MergeConfig:
    finetune_merge: List[MergeModel]
    output_base_model: str
    output_dir: str
    output_dtype: str = "bfloat16"
    device: str = "cpu"
    clean_cache: bool = False
    cache_dir: str = "cache"
    storage_dir: str = "storage"
    merge_options: Dict[str, Union[int, float]] = field(default_factory=dict)    # (an int: seed of the DARE operators)
    operator: str = "fourier"
    norm_mode: str = DEFAULT_NORM_MODE
    task_add_models: List[str] = field(default_factory=list)      # operator fourier_legacy only (reference fourier.py:39,115)

    # -- derived views ------------------------------------------------------------
    def _first(self, flag: str) -> Optional[MergeModel]:
        return next((m for m in self.finetune_merge if getattr(m, flag)), None)

    @property
    def input_model(self) -> Optional[MergeModel]:
        return self._first("is_input")

    @property
    def output_model(self) -> Optional[MergeModel]:
        return self._first("is_output")

    @property
    def output_path(self) -> Path:
        return Path(self.output_dir)

    @property
    def cache_path(self) -> Path:
        return Path(self.cache_dir)

    @property
    def storage_path(self) -> Path:
        return Path(self.storage_dir)

    @property
    def output_astype(self) -> torch.dtype:
        return getattr(torch, self.output_dtype)

    # -- mutation / export (reference config.py:83-101) ------------------------------
    def update(self, config: Optional[Dict[str, Any]] = None, **kwargs):
        """Set known attributes from a dict and/or keywords; unknown keys are ignored."""
        for source in (config or {}, kwargs):
            for key, value in source.items():
                if hasattr(self, key):
                    setattr(self, key, value)

    def to_dict(self) -> Dict[str, Any]:
        """What run_merge receives as **kwargs: note finetune_merge collapses to model names."""
        return {
            "output_base_model": self.output_base_model,
            "finetune_merge": [m.model for m in self.finetune_merge],
            "output_dir": self.output_dir,
            "device": self.device,
            "clean_cache": self.clean_cache,
            "cache_dir": self.cache_dir,
            "storage_dir": self.storage_dir,
        }

    @classmethod
    def from_yaml(cls, config_path) -> "MergeConfig":
        with open(config_path) as fh:
            raw = yaml.safe_load(fh) or {}
        absent = [k for k in _REQUIRED if k not in raw]
        if absent:
            raise click.BadParameter(f"Missing required configuration fields: {', '.join(absent)}")
        if not isinstance(raw["finetune_merge"], list):
            raise click.BadParameter("finetune_merge must be a list of model URIs")
        raw["finetune_merge"] = [MergeModel(**entry) for entry in raw["finetune_merge"]]
        opts = dict(raw.get("merge_options") or {})
        norm_mode = opts.pop("norm_mode", DEFAULT_NORM_MODE)
        if norm_mode not in NORM_MODES:
            raise click.BadParameter("merge_options.norm_mode must be 'exact' or 'reference_cpu'")
        raw["norm_mode"] = norm_mode
        task_add = opts.pop("task_add_models", [])
        if not isinstance(task_add, list) or not all(isinstance(x, str) for x in task_add):
            raise click.BadParameter("merge_options.task_add_models must be a list of model names")
        raw["task_add_models"] = task_add
        operator = opts.pop("operator", "fourier")
        if operator not in OPERATORS:
            raise click.BadParameter(f"merge_options.operator must be one of {list(OPERATORS)}")
        raw["operator"] = operator
        family_options = _family_options(opts, norm_mode, task_add, operator)
        if operator in GEO_PAIR_OPERATORS:
            entries = raw["finetune_merge"]
            if len(entries) != 2:
                raise click.BadParameter(f"operator {operator} interpolates between exactly two finetune_merge entries, not {len(entries)}")
            alphas = [m.alpha for m in entries]
            if any(isinstance(a, bool) or not isinstance(a, (int, float)) or not (a >= 0) for a in alphas) or not (0 < sum(alphas) < float("inf")):
                raise click.BadParameter(f"operator {operator} needs finetune_merge alphas >= 0 with a sum > 0 (the interpolation "
                                         f"point is alpha_1 / (alpha_0 + alpha_1)), not {alphas}")
        if operator in SPHERE_OPERATORS:
            alphas = [m.alpha for m in raw["finetune_merge"]]
            if not alphas or any(isinstance(a, bool) or not isinstance(a, (int, float)) or not (a >= 0) for a in alphas) \
                    or not (0 < sum(alphas) < float("inf")):
                raise click.BadParameter(f"operator {operator} needs finetune_merge alphas >= 0 with a sum > 0 (the weight of a "
                                         f"direction on the sphere is alpha_i / sum alpha), not {alphas}")
        if operator == "sce":
            alphas = [m.alpha for m in raw["finetune_merge"]]
            if any(isinstance(a, bool) or not isinstance(a, (int, float)) or not (a >= 0) for a in alphas) or not (0 < sum(alphas) < float("inf")):
                raise click.BadParameter(f"operator sce needs finetune_merge alphas >= 0 with a sum > 0 (an alpha is a prior on the "
                                         f"finetune's weight), not {alphas}")
        if operator == "tsv":
            alphas = [m.alpha for m in raw["finetune_merge"]]
            if any(isinstance(a, bool) or not isinstance(a, (int, float)) or not (a >= 0) for a in alphas) or not (0 < sum(alphas) < float("inf")):
                raise click.BadParameter(f"operator tsv needs finetune_merge alphas >= 0 with a sum > 0 (an alpha scales the "
                                         f"finetune's singular values; 0 leaves the finetune out), not {alphas}")
        if operator in FUSION_OPERATORS + EMR_OPERATORS:
            for m in raw["finetune_merge"]:
                if isinstance(m.alpha, bool) or not isinstance(m.alpha, (int, float)) or m.alpha != 1:
                    raise click.BadParameter(f"operator {operator} takes no weight: finetune_merge alpha of {m.model} must be 1 "
                                             f"(or absent), not {m.alpha!r} - the operator would ignore it")
        if family_options is not None:
            raw["merge_options"] = family_options
            return cls(**raw)
        unknown = set(opts) - set(MERGE_OPTION_DEFAULTS)
        if not isinstance(opts, dict) or unknown:
            raise click.BadParameter(f"merge_options: unknown keys {sorted(unknown)}; known: {sorted(MERGE_OPTION_DEFAULTS) + ['norm_mode', 'operator']}")
        for key, value in opts.items():
            lo, hi = MERGE_OPTION_RANGES[key]
            if not isinstance(value, (int, float)) or isinstance(value, bool) or not (lo <= float(value) <= hi):
                raise click.BadParameter(f"merge_options.{key} must be a number in [{lo}, {hi}]")
        raw["merge_options"] = {k: float(v) for k, v in opts.items()}
        return cls(**raw)
