/* shardmerge_hip.h - C ABI of the MI355X-native spectral-merge hot path.
 *
 * This is the drop-in boundary for shardmerge's per-layer merge
 * (reference: shard/merge/fast_fourier.py:103-276 calling
 * shard/tensor/functions.py:24-302).  Every pointer marked "device" is a HIP
 * device pointer (e.g. torch.Tensor.data_ptr() on PyTorch-ROCm); `stream` is a
 * hipStream_t passed as void* (NULL = default stream).  The library borrows
 * input pointers for the duration of a call, never mutates inputs, writes only
 * into caller-provided outputs and owns nothing but its internal workspace
 * (grown on demand with hipMalloc, reused across calls).  One context serves
 * one caller thread / one device.
 *
 * All functions return SMHIP_OK (0) or an error code; smhip_last_error() gives
 * the message.  The Python wrapper maps SMHIP_ERR_INF_IFFT / _INF_MERGED to the
 * reference's ValueError texts (functions.py:217, fast_fourier.py:274).
 */
#ifndef SHARDMERGE_HIP_H
#define SHARDMERGE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct smhip_ctx smhip_ctx;

enum {
    SMHIP_OK = 0,
    SMHIP_ERR_HIP = 1,         /* a HIP runtime call failed */
    SMHIP_ERR_SHAPE = 2,       /* unsupported shape, see smhip_length_supported / smhip_shape_supported */
    SMHIP_ERR_INF_IFFT = 3,    /* "Inf in ifft output"            (functions.py:215-217) */
    SMHIP_ERR_INF_MERGED = 4,  /* "Inf in merged tensor for ..."  (fast_fourier.py:273-274) */
    SMHIP_ERR_ARG = 5,
    SMHIP_ERR_NOMEM = 6,
    SMHIP_ERR_NONFINITE = 7,   /* a delta norm is NaN/Inf (K >= 2): the reference's tournament loop
                                  (fast_fourier.py:171-254) never terminates on such input; smhip_ties_merge,
                                  smhip_dare_merge: a finetune's delta holds a NaN or an Inf */
    SMHIP_ERR_ROW_NORM = 8     /* smhip_adapter_apply, DoRA: a row of base + scale * B @ A has a zero or non-finite
                                  norm, or its magnitude is not finite (the message names the first such row) */
};

enum { SMHIP_BF16 = 0, SMHIP_F16 = 1, SMHIP_F32 = 2 };

/* branch taken by a pair merge (fast_fourier.py:223 / :226 / :233) */
enum { SMHIP_BRANCH_ADD = 0, SMHIP_BRANCH_ARITH = 1, SMHIP_BRANCH_SLERP = 2, SMHIP_BRANCH_CARRY = 3,
       SMHIP_BRANCH_EARLY_V0 = 4 /* functions.py:184-190 */, SMHIP_BRANCH_LINEAR = 5 /* functions.py:199-202 */ };

#define SMHIP_MAX_MODELS 16
#define SMHIP_MAX_PAIRS 32

/* ---- lifetime ---------------------------------------------------------- */
int smhip_create(int device, smhip_ctx** out);
void smhip_destroy(smhip_ctx* ctx);
const char* smhip_last_error(smhip_ctx* ctx);
const char* smhip_version(void);
/* pre-size the workspace for [rows x cols] tensors (optional; it grows on demand) */
int smhip_reserve(smhip_ctx* ctx, int rows, int cols);
size_t smhip_workspace_bytes(smhip_ctx* ctx);
/* 0 if a length-n transform has a work-group plan (n <= 32768 with prime factors <= 13; what the
 * function-level entry points A4-A10 need of both lengths), SMHIP_ERR_SHAPE otherwise */
int smhip_length_supported(int n);
/* 0 if smhip_merge_layer takes a [rows x cols] tensor (rows = 1 for 1-D): one length must have a
 * plan; the other may also be p * M with M planned and even and p <= 256 - 11008 = 43 * 256,
 * 18944 = 37 * 512, 65536 = 2 * 32768, 128256 = 167 * 768 - which costs one extra pass over the
 * row spectra each way (and, when it is the ROW length, a transpose of the operands).  A tensor without
 * any planned length (Falcon-7B: 4544 = 71 * 64, 4672 = 73 * 64) is taken when one length splits as
 * above and the other, of any factorisation and parity, is <= 16384: its rows go through the chirp-z
 * row passes (sm_bluestein.hpp), 3-4x the arithmetic of a planned length.  The function-level entry
 * points A4-A10 take such a ROW length too (their column length needs a plan). */
int smhip_shape_supported(int rows, int cols);

/* ---- A4 / A8: transforms (reference fft_transform / ifft_transform,
 *      functions.py:45-73).  x: device float[rows*cols] (rows = 1 for 1-D);
 *      spectrum: device interleaved complex64 [rows][cols]. ------------------- */
int smhip_fft_transform(smhip_ctx* ctx, const float* x, int rows, int cols, float* spectrum, void* stream);
int smhip_ifft_transform(smhip_ctx* ctx, const float* spectrum, int rows, int cols, float* real_out, void* stream);

/* ---- A5-A7: spectrum-level blends on full complex spectra
 *      (interpolate_fft_components functions.py:90-162,
 *       arithmetic_fft_components functions.py:256-302). --------------------- */
typedef struct {
    double cutoff_threshold, cull_threshold;
    double dot, s00, s01, s11;
    uint64_t n_slerp;
    double t;          /* slerp fraction used (fast_fourier.py:234: weights NOT swapped with a/b, quirk Q4) */
    double cull_pct;   /* cull fraction used (halved every tournament round, fast_fourier.py:254) */
} smhip_blend_info;
int smhip_interpolate_fft_components(smhip_ctx* ctx, const float* f0, const float* f1, int rows, int cols,
                                     double t, double t_sum, double cutoff_pct, double cull_pct, int interp_imag,
                                     float* out_spectrum, smhip_blend_info* info, void* stream);
int smhip_arithmetic_fft_components(smhip_ctx* ctx, const float* f0, const float* f1, int rows, int cols,
                                    double t, int agreement, int do_imag, float* out_spectrum, void* stream);

/* ---- A9: merge_tensors_fft2_slerp (functions.py:164-221).
 *      v0, v1, out: device float[rows*cols].  *branch reports which path ran
 *      (SLERP, EARLY_V0 or LINEAR). ------------------------------------------ */
int smhip_merge_tensors_fft2_slerp(smhip_ctx* ctx, const float* v0, const float* v1, int rows, int cols,
                                   double t, double b, double t_sum, double cutoff_pct, double cull_pct,
                                   float* out, double* norm0, double* norm1, int* branch,
                                   smhip_blend_info* info, void* stream);

/* ---- A10: task_arithmetic_fft2 (functions.py:224-254) ------------------- */
int smhip_task_arithmetic_fft2(smhip_ctx* ctx, const float* v0, const float* v1, int rows, int cols,
                               double t, int agreement, float* out, void* stream);

/* ---- A1-A13 fused: the block-tensor branch of FourierMerge._merge_layer
 *      (fast_fourier.py:132-276 + base.py:117-137). ------------------------- */
typedef struct {
    int k;                                  /* models that pass use_layer_index */
    const void* finetune[SMHIP_MAX_MODELS]; /* device, in_dtype, [rows*cols] */
    const void* base[SMHIP_MAX_MODELS];     /* device, in_dtype: each model's own base */
    double alpha[SMHIP_MAX_MODELS];
    int in_dtype;
    const void* base_out;                   /* device: output_base_model's tensor */
    int base_out_dtype;
    int rows, cols;                         /* rows = 1 for 1-D tensors */
    double target_norm_offset;              /* 1e-10 */
    double cull_start_pct;                  /* 0.20 */
    double cutoff_pct;                      /* 0.08 */
    double t_sum;                           /* 1.0  */
    double b;                               /* 0.1: merge_tensors_fft2_slerp's norm-ratio threshold below which
                                               the pair is blended linearly, R = F0 + t F1 (functions.py:164,196-202);
                                               unreachable at the default (the layer's own rule routes ratios < 0.1
                                               to Arithmetic-FFT first, fast_fourier.py:226) */
    int norm_mode;                          /* 1 "reference_cpu" - what every host entry point of this package passes by
                                               default (shardmerge_amd/constants.py: DEFAULT_NORM_MODE): every norm the
                                               reference takes as torch's CPU kernel returns it - acc = fma(x, x, acc)
                                               serially in 8 fp32 lanes, biased by -5e-3 at 67 M elements - which the
                                               reference's device="cpu" output depends on at the 1e-2 level.  EXACT (bit
                                               for bit, csrc/sm_aten_norm.hpp) for spatial tensors: the deltas and
                                               materialised intermediates; MODELLED for what has no spatial form here:
                                               the gathered slerp-class vectors (sampled statistics, 1e-6 ... 4e-6 of
                                               torch's value) and a K >= 3 intermediate kept in the spectral domain
                                               (Gaussian model of its exact Parseval norm, ~1e-5).  Costs ~0.3 ms per
                                               8192 x 8192 layer.  Inputs that are not 16-byte aligned are loaded element
                                               by element; the mode never falls back to other numerics silently (an
                                               input it cannot handle is SMHIP_ERR_ARG).
                                               0 "exact": accurate L2 norms - the reference's device="cuda" numerics */
    int batch;                              /* 0 / 1: one [rows x cols] tensor.  > 1: a rank > 2 tensor, `batch` contiguous
                                               slices [rows x cols]: each slice is transformed on its own (the reference's
                                               fftn(dim=(-2,-1)), functions.py:58) while every norm, order statistic and
                                               slerp sum runs over the whole tensor, as the reference's flat ops do */
} smhip_layer_desc;

typedef struct {
    double target_norm;
    double delta_norm[SMHIP_MAX_MODELS];
    int n_steps;                            /* pair merges + carries, in order */
    int step_x[SMHIP_MAX_PAIRS], step_y[SMHIP_MAX_PAIRS];   /* stack indices (y = -1: carry) */
    int step_branch[SMHIP_MAX_PAIRS];
    smhip_blend_info step_info[SMHIP_MAX_PAIRS];
    uint32_t nan_ifft, nan_final;           /* NaNs replaced by 0 (functions.py:211-213, fast_fourier.py:270-271) */
    double merged_delta_norm;               /* || result before add-back || when available, else -1 */
} smhip_layer_report;

/* out: device bf16 [rows*cols] (the reference hard-casts block tensors to bf16,
 * fast_fourier.py:276).  delta_out (optional, may be NULL): device float of the
 * merged delta before add-back, for parity checks. */
int smhip_merge_layer(smhip_ctx* ctx, const smhip_layer_desc* desc, void* out_bf16, float* delta_out,
                      smhip_layer_report* report, void* stream);

/* ---- N3: AdditionMerge / TaskAdditionMerge (reference shard/merge/addition.py:70-76,
 *      shard/merge/taskaddition.py:69-79): out = sum_i (finetune_i - base), optionally keeping per
 *      element only the deltas whose sign equals the majority sign.  All tensors: device, `dtype`,
 *      n elements; the arithmetic is the dtype's, as torch does it on CPU (16-bit ops are fp32 ops
 *      rounded to the dtype).  The base is NOT added back (the reference does not). ------------ */
int smhip_addition_merge(smhip_ctx* ctx, int k, const void* const* finetunes, const void* base, int dtype, size_t n,
                         int sign_agreement, void* out, void* stream);

/* ---- TIES merge (Yadav et al., "TIES-Merging", 2023).  The reference has no such operator; this section IS its
 *      definition.  For one tensor of n elements (any shape, flat), finetunes i = 0..k-1 in order (1 <= k <= 16):
 *        1. d_i = fp32(finetune_i) - fp32(base_i).  A NaN or Inf in any d_i fails the call with SMHIP_ERR_NONFINITE
 *           (the message lists the finetunes); out is then unspecified.
 *        2. k_keep = n if density == 1, else (uint64) floor(density * n) in fp64.  tau_i = the k_keep-th largest |d_i|,
 *           exact; +inf when k_keep == 0.  An element is KEPT iff |d_i| >= tau_i and d_i != 0.  TIE RULE: every element
 *           that ties with the threshold is kept (kept[i] may exceed k_keep), so the result does not depend on any
 *           traversal order - unlike a top-k, which keeps an arbitrary subset of the tied elements.
 *        3. tv_i = fl32(d_i * fp32(alpha_i)) where kept, 0 elsewhere.
 *        4. S = ((0 + tv_0) + tv_1) + ... in fp32; the elected sign is +1 if S >= 0, else -1.
 *        5. m_i = [sign(tv_i) == elected sign] (a zero agrees with nothing); M = sum_i m_i tv_i, D = sum_i m_i fp32(alpha_i),
 *           fp32, same order, from 0.
 *        6. normalize: D := 1 where |D| < fp32(1e-8); M := M / D (IEEE fp32 division).
 *        7. out = round_to(base_out_dtype, fp32(base_out) + fl32(fp32(lambda) * M)): rounded product, rounded sum,
 *           one round-to-nearest-even cast.
 *      Every step is one correctly rounded fp32 operation or an exact order statistic: the result is defined bit for bit.
 *      The selection is a radix select over the 31 magnitude bits (histogram passes, no sort, 64-bit counts) that forms
 *      the deltas on the fly; thresholds stay on the device and the call synchronises the stream once, at its end, to
 *      fetch the report.  Inputs may alias each other; out (and delta_out) must not overlap an input.  n == 0 is a
 *      no-op.  Pointers need only the alignment of their element type (16-byte aligned ones take the fast path).
 *      Profile names: "ties_hist", "ties_select", "ties_merge". ---- */
typedef struct {
    int k;
    const void* finetune[SMHIP_MAX_MODELS]; /* device, in_dtype, [n] */
    const void* base[SMHIP_MAX_MODELS];     /* device, in_dtype: each finetune's own base */
    double alpha[SMHIP_MAX_MODELS];
    int in_dtype;                           /* SMHIP_BF16 / F16 / F32, finetunes and their bases */
    const void* base_out; int base_out_dtype;
    size_t n;
    double density, lambda; int normalize;
} smhip_ties_desc;
typedef struct {
    uint64_t k_keep;
    float threshold[SMHIP_MAX_MODELS];      /* tau_i */
    uint64_t kept[SMHIP_MAX_MODELS];        /* elements of finetune i that were kept (>= k_keep through ties, less
                                               where the threshold is 0) */
} smhip_ties_report;
/* out: device, base_out_dtype, [n].  delta_out (optional): device float [n], fl32(lambda * M).  report (optional): HOST. */
int smhip_ties_merge(smhip_ctx* ctx, const smhip_ties_desc* desc, void* out, float* delta_out,
                     smhip_ties_report* report, void* stream);

/* ---- DARE merge (Yu et al., "Language Models are Super Mario", 2023): drop each delta entry at random with
 *      probability 1 - density, rescale the survivors by 1 / density, then add the weighted deltas (dare_linear) or
 *      elect a sign and merge the agreeing entries as TIES does (dare_ties).  The reference has no such operator; this
 *      section IS its definition.  The random mask is a FUNCTION of (key, stream id, element index) - a counter-based
 *      generator, no stream and no state - so the same call gives the same bytes whatever the grid, the traversal
 *      order or the number of processes.  For one tensor of n elements (any shape, flat), finetunes i = 0..k-1 in
 *      order (1 <= k <= 16):
 *        1. d_i = fp32(finetune_i) - fp32(base_i).  A NaN or Inf in any d_i fails the call with SMHIP_ERR_NONFINITE
 *           (the message lists the finetunes); out is then unspecified.
 *        2. T = 65536 if density == 1, else (uint32) floor(density * 65536) in fp64.  T == 0 (density < 2^-16) is
 *           SMHIP_ERR_ARG.  The EFFECTIVE density is q = T / 65536: it is what the report carries and what the rescale
 *           uses, so the expectation is unbiased for the mask actually drawn.
 *        3. Mask.  For element index j (flat, 64-bit) of finetune i:
 *             blk = Philox4x32-10(counter = (lo32(j >> 3), hi32(j >> 3), stream_id[i], 0), key = (lo32(key), hi32(key)))
 *           (Salmon et al. 2011: multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85, ten
 *           rounds); w = blk[(j & 7) >> 1]; h = (j & 1) ? w >> 16 : w & 0xffff.  The element is KEPT iff h < T and
 *           d_i != 0.  One block decides one octet of eight consecutive elements; the mask is monotone in T.
 *        4. r = 1 if rescale == 0, else fp32(65536.0 / T) (fp64 division, one rounding).
 *           tv_i = fl32(fl32(d_i * r) * fp32(alpha_i)) where kept, +0 elsewhere.
 *        5. sign_election == 1 (dare_ties): steps 4-6 of smhip_ties_merge on these tv_i (S, the elected sign, M and D
 *           over the agreeing entries, |D| < 1e-8 -> 1, M / D when normalize).
 *           sign_election == 0 (dare_linear): M = ((0 + tv_0) + tv_1) + ... in fp32; D = ((0 + fp32(alpha_0)) + ...)
 *           over ALL finetunes, kept or not; the same |D| < 1e-8 -> 1 and division when normalize.
 *        6. out = round_to(base_out_dtype, fp32(base_out) + fl32(fp32(lambda) * M)), delta_out = fl32(lambda * M):
 *           step 7 of smhip_ties_merge.
 *      Every step is an integer function or one correctly rounded fp32 operation: the result is defined bit for bit.
 *      With density = 1 and sign_election = 1 the result equals smhip_ties_merge at density 1 for any key.  ONE kernel,
 *      one pass over the inputs; the call synchronises the stream once, at its end, to fetch the report.  Aliasing,
 *      alignment and n == 0: the rules of smhip_ties_merge.  Profile name: "dare_merge". ---- */
typedef struct {
    int k;
    const void* finetune[SMHIP_MAX_MODELS]; /* device, in_dtype, [n] */
    const void* base[SMHIP_MAX_MODELS];     /* device, in_dtype: each finetune's own base */
    double alpha[SMHIP_MAX_MODELS];
    int in_dtype;                           /* SMHIP_BF16 / F16 / F32, finetunes and their bases */
    const void* base_out; int base_out_dtype;
    size_t n;
    double density, lambda; int normalize;
    uint64_t key;                           /* the generator's key: the same for every finetune of the tensor */
    uint32_t stream_id[SMHIP_MAX_MODELS];   /* word 2 of finetune i's counter: what tells the finetunes' masks apart */
    int rescale;                            /* 1: survivors times fp32(65536 / T); 0: left as they are */
    int sign_election;                      /* 1: dare_ties; 0: dare_linear */
} smhip_dare_desc;
typedef struct {
    uint32_t T;                             /* the keep threshold on the 16-bit draw; effective density T / 65536 */
    uint64_t kept[SMHIP_MAX_MODELS];        /* elements of finetune i that were kept */
} smhip_dare_report;
/* out: device, base_out_dtype, [n].  delta_out (optional): device float [n], fl32(lambda * M).  report (optional): HOST. */
int smhip_dare_merge(smhip_ctx* ctx, const smhip_dare_desc* desc, void* out, float* delta_out,
                     smhip_dare_report* report, void* stream);

/* ---- Model Breadcrumbs merge (Davari & Belilovsky, "Model Breadcrumbs", 2023): trim each finetune's delta at BOTH
 *      ends - drop the smallest magnitudes, as TIES does, and also the few largest ones, the outliers - then add the
 *      weighted masked deltas (breadcrumbs) or elect a sign and merge the agreeing entries as TIES does
 *      (breadcrumbs_ties).  The reference has no such operator; this section IS its definition.  For one tensor of n
 *      elements (any shape, flat), finetunes i = 0..k-1 in order (1 <= k <= 16):
 *        1. d_i = fp32(finetune_i) - fp32(base_i).  A NaN or Inf in any d_i fails the call with SMHIP_ERR_NONFINITE
 *           (the message lists the finetunes); out is then unspecified.
 *        2. k_keep = n if density == 1, else (uint64) floor(density * n) in fp64 (the rule of smhip_ties_merge).
 *           n_top = min((uint64) floor(gamma * n), n - k_keep) in fp64: the number of largest magnitudes that may be
 *           dropped.  Arguments: 0 < density <= 1, 0 <= gamma < 1, density + gamma <= 1 evaluated in fp64, else
 *           SMHIP_ERR_ARG.
 *        3. With the magnitudes ranked from the largest: tau_hi_i = the (n_top + 1)-th largest |d_i|, tau_lo_i = the
 *           (n_top + k_keep)-th largest, both exact; both +inf when k_keep == 0.  An element is KEPT iff
 *           tau_lo_i <= |d_i| <= tau_hi_i and d_i != 0.  TIE RULE: an element that ties with either threshold is kept,
 *           so the result does not depend on any traversal order; at most n_top elements (those strictly above
 *           tau_hi_i) are dropped at the top, and at least k_keep are kept unless tau_lo_i == 0 (zeros are never
 *           kept).  With n_top == 0, tau_hi_i is the maximum and the upper test is vacuous - there is no special case.
 *        4. tv_i = fl32(d_i * fp32(alpha_i)) where kept, +0 elsewhere.
 *        5. sign_election == 1 (breadcrumbs_ties): steps 4-6 of smhip_ties_merge on these tv_i.
 *           sign_election == 0 (breadcrumbs): M = ((0 + tv_0) + tv_1) + ... in fp32; D = ((0 + fp32(alpha_0)) + ...)
 *           over ALL finetunes, kept or not; D := 1 where |D| < fp32(1e-8); M := M / D when normalize - step 5 of
 *           smhip_dare_merge for dare_linear.
 *        6. out = round_to(base_out_dtype, fp32(base_out) + fl32(fp32(lambda) * M)), delta_out = fl32(lambda * M):
 *           step 7 of smhip_ties_merge.
 *      Every step is one correctly rounded fp32 operation or an exact order statistic: the result is defined bit for
 *      bit.  Two identities follow: gamma == 0 with sign_election == 1 equals smhip_ties_merge with the same density,
 *      lambda and normalize; gamma == 0, density == 1, sign_election == 0 equals smhip_dare_merge with density 1 and
 *      sign_election 0 (any key, either rescale).  Both order statistics of a finetune are found in the same three
 *      histogram passes that smhip_ties_merge spends on one, so the call moves the same 4k + 5 tensors (shared base).
 *      Aliasing, alignment, n == 0 and the size limit: the rules of smhip_ties_merge; the call synchronises the stream
 *      once, at its end, to fetch the report.  Profile names: "crumbs_hist", "crumbs_select", "crumbs_merge". ---- */
typedef struct {
    int k;
    const void* finetune[SMHIP_MAX_MODELS]; /* device, in_dtype, [n] */
    const void* base[SMHIP_MAX_MODELS];     /* device, in_dtype: each finetune's own base */
    double alpha[SMHIP_MAX_MODELS];
    int in_dtype;                           /* SMHIP_BF16 / F16 / F32, finetunes and their bases */
    const void* base_out; int base_out_dtype;
    size_t n;
    double density, lambda; int normalize;
    double gamma;                           /* the share of largest magnitudes that may be dropped */
    int sign_election;                      /* 1: breadcrumbs_ties; 0: breadcrumbs */
} smhip_breadcrumbs_desc;
typedef struct {
    uint64_t k_keep, n_top;
    float threshold_lo[SMHIP_MAX_MODELS];   /* tau_lo_i */
    float threshold_hi[SMHIP_MAX_MODELS];   /* tau_hi_i */
    uint64_t kept[SMHIP_MAX_MODELS];        /* elements of finetune i that were kept */
    uint64_t dropped_top[SMHIP_MAX_MODELS]; /* elements strictly above tau_hi_i (<= n_top) */
} smhip_breadcrumbs_report;
/* out: device, base_out_dtype, [n].  delta_out (optional): device float [n], fl32(lambda * M).  report (optional): HOST. */
int smhip_breadcrumbs_merge(smhip_ctx* ctx, const smhip_breadcrumbs_desc* desc, void* out, float* delta_out,
                            smhip_breadcrumbs_report* report, void* stream);

/* ---- Geometric merges: Model Stock (Jang et al., "Model Stock: All we need is just a few fine-tuned models", 2024),
 *      SLERP and NuSLERP.  The coefficients come from the geometry of the vectors - their norms and the angles between
 *      them - not from a per-element decision.  The reference has no such operators; this section IS their definition.
 *      One tensor of n elements viewed as R x C: R = `rows` (the first dimension, 1 for a 1-D tensor), C = n / R.
 *      Finetunes i = 0..k-1 in order, 1 <= k <= 16.
 *        1. Vectors.  Delta space (mode MODEL_STOCK, NUSLERP): x_i = fl32(fp32(finetune_i) - fp32(base_i)).  Weight
 *           space (mode SLERP): x_i = fp32(finetune_i); base_i and base_out are not read (they may be NULL).  A NaN or
 *           Inf in any x_i fails the call with SMHIP_ERR_NONFINITE (the message lists the finetunes); out is then
 *           unspecified.
 *        2. Gram.  G[i][j] = sum_e (double) x_i[e] * (double) x_j[e], i <= j, over the whole tensor (rowwise == 0) or
 *           over each row (rowwise == 1, MODEL_STOCK only).  A product of two fp32 values is exact in fp64; every
 *           addition is one correctly rounded fp64 addition, in THIS order:
 *             - the elements are cut into SEGMENTS: whole tensor, segment s = elements [32768 s, min(n, 32768 (s + 1)));
 *               row-wise, segment s = row s (C elements);
 *             - inside a segment, the element with segment-local index c belongs to octet o = c / 8 and to LANE
 *               t = o % 256.  A lane starts from +0 and adds the products of its elements in ascending index order:
 *               p_t = (...((0 + x_i[c_0] x_j[c_0]) + x_i[c_1] x_j[c_1]) + ...), c_0 < c_1 < ...; a lane without
 *               elements is +0;
 *             - the 256 lanes are reduced by a binary tree: for s = 128, 64, 32, 16, 8, 4, 2, 1 in turn,
 *               p_t = p_t + p_(t+s) for every t < s; the segment's value is p_0;
 *             - whole tensor: G = (...((0 + S_0) + S_1) + ...) over the segments' values in ascending index order;
 *               row-wise: the Gram of row r is S_r.
 *           The order is a function of n alone (of C alone for a row): it does not depend on the device, the grid, the
 *           stream or the number of processes, and no floating-point atomic takes part.
 *        3. Coefficients, in fp64, every operation one IEEE operation (no fused multiply-add), each coefficient rounded
 *           once to fp32.  n_i = sqrt(G[i][i]); cos_ij = clamp(G[i][j] / (n_i * n_j), -1, 1), or 0 when n_i * n_j is 0
 *           or not finite (two parallel vectors reach +-1 only up to the rounding of the two square roots).
 *           MODEL_STOCK: k == 1: t = 1.  Else cos = (((0 + cos_01) + cos_02) + ... over i < j, lexicographic)
 *             / (double)(k (k - 1) / 2); den = 1 + (k - 1) * cos; t = (k * cos) / den when den > 0 and the quotient is
 *             finite, else 0.  A = ((0 + alpha_0) + alpha_1) + ..., A := 1 where |A| < 1e-8.
 *             c_i = fp32((t * alpha_i) / A).  Equal alphas: the plain average of the finetunes, interpolated towards
 *             the base by t, as in the paper.  Row-wise: cos, t and c_i exist per row (computed on the device; the
 *             formulas need + - * / sqrt only).
 *           NUSLERP, SLERP: k <= 2, rowwise == 0.  k == 1: c_0 = 1.  k == 2: both alphas >= 0 and their sum > 0, else
 *             SMHIP_ERR_ARG; tau = alpha_1 / (alpha_0 + alpha_1).  LINEAR case (n_0 == 0, n_1 == 0 or
 *             |cos_01| > 0.9995): s_0 = 1 - tau, s_1 = tau.  Else Omega = acos(cos_01), s_0 = sin((1 - tau) * Omega)
 *             / sin(Omega), s_1 = sin(tau * Omega) / sin(Omega), with the C library's acos and sin in double.
 *             SLERP (the classic form, on the weights): c_i = fp32(s_i).
 *             NUSLERP (the direction is slerped between the unit vectors, the length interpolated linearly):
 *             N = (1 - tau) * n_0 + tau * n_1, c_i = fp32((s_i * N) / n_i); in the linear case c_i = fp32(s_i).
 *        4. Combine.  M = ((0 + fl32(c_0 * x_0)) + fl32(c_1 * x_1)) + ... in fp32, product and sum rounded separately.
 *           Delta space: out = round_to(base_out_dtype, fp32(base_out) + M).  Weight space: out =
 *           round_to(base_out_dtype, M).  delta_out (optional) = M.
 *      Aliasing, alignment, n == 0, dtypes and the size limit: the rules of smhip_ties_merge (n > 0 needs rows >= 1
 *      that divides n).  Whole-tensor calls synchronise the stream once, after the Gram, to fetch it and compute the
 *      coefficients on the host; row-wise calls once, at their end.  Profile names: "geo_gram", "geo_gram_fold" (whole
 *      tensor), "geo_coef" (row-wise), "geo_combine". ---- */
enum { SMHIP_GEO_MODEL_STOCK = 0, SMHIP_GEO_NUSLERP = 1, SMHIP_GEO_SLERP = 2 };
typedef struct {
    int k;
    const void* finetune[SMHIP_MAX_MODELS]; /* device, in_dtype, [n] */
    const void* base[SMHIP_MAX_MODELS];     /* device, in_dtype: each finetune's own base (SLERP: not read) */
    double alpha[SMHIP_MAX_MODELS];
    int in_dtype;                           /* SMHIP_BF16 / F16 / F32, finetunes and their bases */
    const void* base_out; int base_out_dtype;   /* (SLERP: base_out is not read, base_out_dtype is out's dtype) */
    size_t n;
    int mode;                               /* SMHIP_GEO_* */
    int rowwise;                            /* 1: a Gram, a t and coefficients per row (MODEL_STOCK only) */
    size_t rows;                            /* R */
} smhip_geo_desc;
typedef struct {
    double G[SMHIP_MAX_MODELS][SMHIP_MAX_MODELS];   /* whole tensor: the Gram, both triangles */
    double cos;                             /* whole tensor: MODEL_STOCK the mean cosine, else cos_01 (0 when k == 1) */
    double t;                               /* whole tensor: MODEL_STOCK t, else tau */
    double omega;                           /* NUSLERP / SLERP: Omega, 0 in the linear case */
    int linear;                             /* NUSLERP / SLERP: 1 in the linear case (and when k == 1) */
    float c[SMHIP_MAX_MODELS];              /* whole tensor: the coefficients */
    double t_min, t_max, t_mean;            /* row-wise: over the rows' t; the mean is (((0 + t_0) + t_1) + ...) / R */
} smhip_geo_report;
/* out: device, base_out_dtype, [n].  delta_out (optional): device float [n], M.  report (optional): HOST. */
int smhip_geo_merge(smhip_ctx* ctx, const smhip_geo_desc* desc, void* out, float* delta_out,
                    smhip_geo_report* report, void* stream);

/* ---- Karcher-mean merges (operators karcher and multislerp): the DIRECTIONS of k vectors are averaged on the unit sphere
 *      - the weighted Karcher (Frechet) mean, found by iterating the log map - and their LENGTHS linearly.  They
 *      generalise NuSLERP (weight_space == 0), and its rule applied to the weights themselves (weight_space == 1), from
 *      two vectors to 1 <= k <= 16; with k == 2 the first iteration lands on the SLERP direction, so the coefficients are
 *      NUSLERP's c_i = s_i * N / n_i - and SLERP's c_i = s_i where the two norms are equal (SLERP leaves the length to its
 *      two sines).  The reference has no such operators; this section IS their definition.  The mean of k unit vectors lies in their span, so every inner product the iteration takes is a
 *      combination of Gram entries: the iteration runs on k coefficients and reads no tensor.
 *        1. Vectors, 2. Gram, 4. Combine: steps 1, 2 and 4 of smhip_geo_merge with x_i in delta space (weight_space == 0)
 *           or weight space (weight_space == 1; base_i and base_out are not read), the Gram over the whole tensor
 *           (rowwise == 0) or over each of the R rows (rowwise == 1), the combination with the coefficients of step 3
 *           (one set per row when rowwise == 1).
 *        3. Coefficients.  Every operation below is ONE IEEE fp64 operation (no fused multiply-add); every sum runs in
 *           ascending index order starting from +0; "v^T H v" is sum_i v_i * (sum_j H_ij * v_j).
 *           Weights.  Every alpha must be >= 0 and A = ((0 + alpha_0) + alpha_1) + ... > 0, else SMHIP_ERR_ARG.
 *             n_i = sqrt(G_ii), w_i = alpha_i / A.  Vector i is ACTIVE when n_i > 0 and w_i > 0; W = the sum of the active
 *             w_i; w_i := w_i / W for an active vector and 0 for an inactive one.  N = sum_i w_i * n_i.
 *           Normalised Gram.  H_ij = cos_ij of smhip_geo_merge (clamp(G_ij / (n_i * n_j), -1, 1), 0 when n_i * n_j is 0
 *             or not finite) for i != j, H_ii = 1.  a is the coefficient vector of the current point m = sum a_i u_i,
 *             u_i = x_i / n_i.
 *           Start.  a = w.  With no active vector or one, c_i = fp32(a_i) (all 0, or a single 1): no iteration,
 *             converged.  Else q = a^T H a; q <= 1e-16 (or not finite) is the LINEAR case: the unit vectors cancel,
 *             c_i = fp32(w_i), no iteration.  Else a_i = a_i / sqrt(q).
 *           Iterations it = 0 .. max_iter - 1 (`iterations` counts how often tau was evaluated):
 *             d_j = clamp(sum_i a_i * H_ij, -1, 1); theta_j = sm_acos(d_j);
 *             f_j = 1 when theta_j < 1e-8; else f_j = 0 when sm_sin(theta_j) < 1e-8 (antipodal: the log map is
 *             undefined), else f_j = theta_j / sm_sin(theta_j);
 *             p_j = w_j * f_j; g = sum_j p_j * d_j; t_i = p_i - a_i * g;
 *             tau = sqrt(max(t^T H t, 0)), at most fp64(pi); tau < tol: converged, stop;
 *             a_i = sm_cos(tau) * a_i + s * t_i with s = 1 when tau < 1e-8, else sm_sin(tau) / tau;
 *             q = a^T H a, a_i = a_i / sqrt(q).
 *             A t^T H t that is not finite, or a q that is <= 1e-16 or not finite, ends the iteration in the LINEAR
 *             case: c_i = fp32(w_i).  Not converging within max_iter is no error: the report says so.  (Two antipodal
 *             vectors reach H_ij = -1 only up to the rounding of the two square roots: with equal weights their q is 0
 *             or a few 1e-16, on either side of the threshold.  Past it the iteration runs on a direction that is
 *             rounding noise, as the mean of antipodal points is any point of their equator; the combination stays
 *             bounded by N.)
 *           Coefficients.  c_i = fp32((a_i * N) / n_i) for an active vector, 0 for an inactive one.
 *           sm_acos on [-1, 1], sm_sin and sm_cos on [0, pi] are DEFINED in csrc/sm_sphere.hpp: Horner evaluations of
 *           truncated Taylor series (asin to degree 47 on [-1/2, 1/2] behind the half-angle reduction; sin to degree 23
 *           and cos to degree 24 on [0, pi/2] behind the reflection at pi/2) over the four operations + * / sqrt, the
 *           coefficients written as hex floats, so that every implementation gives the same bits.  Their absolute error
 *           is below 2^-40 (measured: below 2^-50).  Row-wise, step 3 runs per row on the device; rows stop
 *           independently.
 *      Arguments: 1 <= max_iter <= 100, 0 <= tol < 1.  Aliasing, alignment, n == 0, dtypes, SMHIP_ERR_NONFINITE and the
 *      size limit: the rules of smhip_geo_merge (n > 0 needs rows >= 1 that divides n).  One synchronisation per call,
 *      as there.  Profile names: "geo_gram", "geo_gram_fold" (whole tensor), "sphere_coef" (row-wise), "geo_combine",
 *      each ONE launch per call. ---- */
typedef struct {
    int k;
    const void* finetune[SMHIP_MAX_MODELS]; /* device, in_dtype, [n] */
    const void* base[SMHIP_MAX_MODELS];     /* device, in_dtype: each finetune's own base (weight space: not read) */
    double alpha[SMHIP_MAX_MODELS];
    int in_dtype;                           /* SMHIP_BF16 / F16 / F32, finetunes and their bases */
    const void* base_out; int base_out_dtype;   /* (weight space: base_out is not read, base_out_dtype is out's dtype) */
    size_t n;
    int weight_space;                       /* 1: karcher (x_i = finetune_i), 0: multislerp (x_i = finetune_i - base_i) */
    int rowwise;                            /* 1: a Gram, an iteration and coefficients per row */
    size_t rows;                            /* R */
    int max_iter;                           /* 1..100 */
    double tol;                             /* [0, 1): the iteration stops when tau < tol */
    float* row_coef;                        /* row-wise, optional, HOST: [R][k] coefficients */
    int32_t* row_iters;                     /* row-wise, optional, HOST: [R] iterations */
    int32_t* row_flags;                     /* row-wise, optional, HOST: [R], bit 0 converged, bit 1 linear */
} smhip_sphere_desc;
typedef struct {
    double G[SMHIP_MAX_MODELS][SMHIP_MAX_MODELS];   /* whole tensor: the Gram, both triangles */
    double H[SMHIP_MAX_MODELS][SMHIP_MAX_MODELS];   /* whole tensor: the normalised Gram */
    double w[SMHIP_MAX_MODELS];             /* whole tensor: the renormalised weights */
    double a[SMHIP_MAX_MODELS];             /* whole tensor: the final coefficient vector of the mean direction */
    double N;                               /* whole tensor: the length, sum w_i n_i */
    float c[SMHIP_MAX_MODELS];              /* whole tensor: the coefficients */
    int iterations;                         /* whole tensor: how often tau was evaluated */
    double tau;                             /* whole tensor: the last tau evaluated (0 when none was) */
    int converged, linear;                  /* whole tensor: tau < tol was reached (or nothing to iterate) / the LINEAR case */
    int iters_max;                          /* row-wise: the largest iteration count of a row */
    uint64_t rows_unconverged, rows_linear; /* row-wise: rows that did not converge / that took the LINEAR case */
    double csum_min, csum_max, csum_mean;   /* row-wise: over s_r = ((0 + c_r0) + c_r1) + ... in fp64; the mean is
                                               (((0 + s_0) + s_1) + ...) / R */
} smhip_sphere_report;
/* out: device, base_out_dtype, [n].  delta_out (optional): device float [n], M.  report (optional): HOST. */
int smhip_sphere_merge(smhip_ctx* ctx, const smhip_sphere_desc* desc, void* out, float* delta_out,
                       smhip_sphere_report* report, void* stream);
/* The probe of the three defined functions: y[i] = sm_acos / sm_sin / sm_cos (x[i]), i < n.  on_device == 0: x and y
 * are HOST arrays, evaluated on the host; 1: DEVICE arrays, evaluated by a kernel ("sphere_fn") on the stream. */
enum { SMHIP_SPHERE_ACOS = 0, SMHIP_SPHERE_SIN = 1, SMHIP_SPHERE_COS = 2 };
int smhip_sphere_fn(smhip_ctx* ctx, int op, const double* x, double* y, size_t n, int on_device, void* stream);

/* ---- SCE merge (Wan et al., "FuseChat: Knowledge Fusion of Chat Models", 2024; mergekit's merge_method sce with
 *      select_topk): SELECT the parameters whose deltas vary most across the finetunes, CALCULATE a weight per finetune
 *      from the energy of what it kept, ERASE the entries whose sign disagrees with the majority.  The reference has no
 *      such operator; this section IS its definition.  For one tensor of n elements (any shape, flat), finetunes
 *      i = 0..k-1 in order (1 <= k <= 16):
 *        1. Deltas.  d_i = fp32(finetune_i) - fp32(base_i).  A NaN or Inf in any d_i fails the call with
 *           SMHIP_ERR_NONFINITE (the message lists the finetunes); out is then unspecified.  Arguments:
 *           0 < select_topk <= 1, every alpha_i >= 0 and finite, their fp64 sum ((0 + alpha_0) + ...) > 0 and finite,
 *           lambda finite, else SMHIP_ERR_ARG.
 *        2. Select.  SKIPPED - every element is selected - when select_topk == 1 or k == 1; the report then carries
 *           nz = k_keep = selected = n and a threshold of 0.  Else the score of an element is the sum of squared
 *           deviations across the finetunes, every operation one rounded fp32 operation, no fused multiply-add:
 *             s = ((0 + d_0) + d_1) + ...;  mean = s / fp32(k) (IEEE division);  e_i = d_i - mean;
 *             q = ((0 + fl32(e_0 * e_0)) + fl32(e_1 * e_1)) + ...
 *           q is never NaN for finite deltas; a q that overflowed to +inf is an ordinary value that sorts above all
 *           others.  nz = the number of elements with q > 0.  k_keep = (uint64) floor(select_topk * nz) in fp64 (one
 *           multiplication, one truncation).  tau = the k_keep-th largest q, exact.  An element is SELECTED iff
 *           k_keep > 0, q >= tau and q > 0.  TIE RULE: every element that ties with tau is selected (selected >= k_keep),
 *           so the result does not depend on any traversal order.  k_keep == 0 selects nothing; the report's threshold
 *           is then +inf.  Counting by nz follows mergekit, which takes the top share of the NONZERO variances.
 *           k == 1 deviates from mergekit on purpose: a single model has zero variance everywhere and mergekit keeps
 *           nothing; here a layer that a window leaves with one entry takes that entry, as the geometric operators do.
 *        3. Calculate.  x_i = d_i where selected, +0 elsewhere (the mask is Select's only; it is applied before Erase,
 *           as in mergekit).  E_i = sum_e (double) x_i[e] * (double) x_i[e] over the whole tensor, accumulated in
 *           exactly the order of step 2 of smhip_geo_merge: 32768-element segments, octet o to lane o % 256, ascending
 *           index inside a lane, the binary tree over the 256 lanes, the segments added in index order.  In fp64, one
 *           IEEE operation each: P_i = alpha_i * E_i, Z = ((0 + P_0) + P_1) + ...; w_i = fp32(P_i / Z) when Z > 0 and
 *           finite, else w_i = fp32(1.0 / k).  Equal alphas of any value give the paper's weights: alpha is a prior on
 *           the weight, not a scale of the delta.
 *        4. Erase and merge, each operation one rounded fp32 operation.  S = ((0 + x_0) + x_1) + ..., unweighted as in the
 *           paper; the elected sign is +1 if S >= 0, else -1.  m_i = [sign(x_i) == elected sign] (a zero agrees with
 *           nothing).  M = sum_i m_i fl32(x_i * w_i), D = sum_i m_i w_i, both from 0 in order.  D := 1 where
 *           |D| < fp32(1e-8); M := M / D (IEEE fp32 division).
 *        5. out = round_to(base_out_dtype, fp32(base_out) + fl32(fp32(lambda) * M)), delta_out = fl32(lambda * M):
 *           step 7 of smhip_ties_merge.
 *      Every step is one correctly rounded operation or an exact order statistic in a stated order: the result is
 *      defined bit for bit.  The selection is ONE radix select over the 31 bits of q (11 + 10 + 10, 64-bit counts)
 *      whatever k; nz, k_keep, tau and the selected count stay on the device.  With a shared base the call moves 5k + 6
 *      tensors (three levels of k + 1, the energy pass k + 1, the merge k + 2), 2k + 3 when the selection is skipped.
 *      Aliasing, alignment, n == 0, dtypes and the size limit: the rules of smhip_ties_merge.  The call synchronises
 *      the stream once, after the energies, to fetch them with the selection's results and compute the weights on the
 *      host.  Profile names: "sce_hist", "sce_select" (three launches each, none when the selection is skipped),
 *      "sce_energy", "sce_energy_fold", "sce_merge". ---- */
typedef struct {
    int k;
    const void* finetune[SMHIP_MAX_MODELS]; /* device, in_dtype, [n] */
    const void* base[SMHIP_MAX_MODELS];     /* device, in_dtype: each finetune's own base */
    double alpha[SMHIP_MAX_MODELS];
    int in_dtype;                           /* SMHIP_BF16 / F16 / F32, finetunes and their bases */
    const void* base_out; int base_out_dtype;
    size_t n;
    double select_topk, lambda;
} smhip_sce_desc;
typedef struct {
    uint64_t nz, k_keep, selected;
    float threshold;                        /* tau; +inf when k_keep == 0; 0 when the selection was skipped */
    double energy[SMHIP_MAX_MODELS];        /* E_i */
    float weight[SMHIP_MAX_MODELS];         /* w_i */
} smhip_sce_report;
/* out: device, base_out_dtype, [n].  delta_out (optional): device float [n], fl32(lambda * M).  report (optional): HOST. */
int smhip_sce_merge(smhip_ctx* ctx, const smhip_sce_desc* desc, void* out, float* delta_out,
                    smhip_sce_report* report, void* stream);

/* ---- DELLA merge (Deep et al., "DELLA-Merging", 2024; mergekit's della and della_linear): DARE whose keep probability
 *      rises with the rank of each entry's magnitude WITHIN ITS ROW, from density - epsilon for the smallest magnitude
 *      of a row to density + epsilon for the largest, then merged as dare_ties (della) or dare_linear (della_linear)
 *      merges.  The reference has no such operator; this section IS its definition.  For one tensor of n elements seen as
 *      R = rows rows of c elements (n = R * c), finetunes i = 0..k-1 in order (1 <= k <= 16):
 *        1. Deltas.  d_i = fp32(finetune_i) - fp32(base_i).  A NaN or Inf in any d_i fails the call with
 *           SMHIP_ERR_NONFINITE (the message lists the finetunes); out is then unspecified.
 *        2. Arguments.  0 < density <= 1 and 0 <= epsilon; density == 1 requires epsilon == 0; otherwise
 *           density + epsilon < 1 and floor((density - epsilon) * 65536) >= 1, evaluated in fp64; rows >= 1 divides n;
 *           anything else is SMHIP_ERR_ARG.  c > 32768 with epsilon > 0 is SMHIP_ERR_SHAPE (the message gives c and
 *           the limit): a row is sorted in the 160 KiB LDS of one compute unit.
 *        3. Rank.  For element j in row rho of finetune i, r_ij is the number of elements of that row of d_i whose
 *           magnitude is STRICTLY SMALLER than |d_ij|: 0 <= r_ij <= c - 1.  The comparison is on the 31 magnitude bits as
 *           unsigned integers (-0 == +0).  TIE RULE: equal magnitudes share a rank, so the result does not depend on
 *           any traversal or sort order - unlike an argsort, which ranks tied elements arbitrarily.
 *        4. Threshold, in fp64, each operation rounded once, in this order: p_lo = density - epsilon; w = 2 * epsilon;
 *           p_ij = p_lo + (w * (double) r_ij) / (double)(c - 1), or p_lo when c == 1;
 *           T_ij = min((uint32) floor(p_ij * 65536), 65535).  density == 1: T_ij = 65536.  epsilon == 0:
 *           T_ij = floor(density * 65536) for every element and no ranking runs.
 *        5. Mask.  The draw h of smhip_dare_merge step 3, unchanged: Philox4x32-10, counter (j >> 3, stream_id[i], 0)
 *           under key, j the element's FLAT index in the whole tensor.  The element is KEPT iff h < T_ij and d_ij != 0.
 *        6. s_ij = 1 if rescale == 0, else fp32(65536.0 / T_ij) (fp64 division, rounded once, then to fp32);
 *           tv_ij = fl32(fl32(d_ij * s_ij) * fp32(alpha_i)) where kept, +0 elsewhere.
 *        7. Steps 5 and 6 of smhip_dare_merge, unchanged: sign_election == 1 is della, 0 is della_linear; normalize,
 *           lambda, out and delta_out as there.
 *      Every step is an integer function, an exact count or one correctly rounded operation: the result is defined bit
 *      for bit.  IDENTITY: with epsilon == 0 the call equals smhip_dare_merge with the same remaining arguments, for
 *      either sign_election and any key; it then runs that kernel and ranks nothing (so does density == 1).  Otherwise
 *      the tensor is processed in slabs of whole rows (at most 2^26 elements per finetune): one work-group per finetune
 *      and row sorts the row's magnitude keys in LDS and writes T_ij as uint16 to a workspace of 2 k bytes per slab
 *      element, then one fused pass merges the slab.  threshold_out (optional, a debugging output in the spirit of
 *      delta_out): device uint16 [k][n], receives T_ij; written only when density < 1.  Aliasing, alignment, n == 0 and
 *      the one synchronisation at the end of the call: the rules of smhip_ties_merge.  Profile names: "della_table"
 *      (T as a function of the rank, once per call), "della_rank" and "della_merge" (once per slab each). ---- */
typedef struct {
    int k;
    const void* finetune[SMHIP_MAX_MODELS]; /* device, in_dtype, [n] */
    const void* base[SMHIP_MAX_MODELS];     /* device, in_dtype: each finetune's own base */
    double alpha[SMHIP_MAX_MODELS];
    int in_dtype;                           /* SMHIP_BF16 / F16 / F32, finetunes and their bases */
    const void* base_out; int base_out_dtype;
    size_t n;
    double density, lambda; int normalize;
    uint64_t key;
    uint32_t stream_id[SMHIP_MAX_MODELS];
    int rescale;                            /* 1: a survivor times fp32(65536 / T_ij); 0: left as it is */
    int sign_election;                      /* 1: della; 0: della_linear */
    double epsilon;                         /* half the width of the keep-probability window */
    size_t rows;                            /* R: the rows the ranks are taken in, c = n / rows */
} smhip_della_desc;
typedef struct {
    uint32_t T_lo, T_hi;                    /* the thresholds of rank 0 and of rank c - 1 */
    uint64_t kept[SMHIP_MAX_MODELS];        /* elements of finetune i that were kept */
} smhip_della_report;
/* out: device, base_out_dtype, [n].  delta_out (optional): device float [n].  threshold_out (optional): device uint16
 * [k][n].  report (optional): HOST. */
int smhip_della_merge(smhip_ctx* ctx, const smhip_della_desc* desc, void* out, float* delta_out, uint16_t* threshold_out,
                      smhip_della_report* report, void* stream);

/* ---- Consensus merge (Wang et al., "Localizing Task Information for Improved Model Merging and Compression", ICML
 *      2024): per finetune a TALL mask marks where its own entry outweighs what the other tasks did to the same weight,
 *      and an element of the multi-task vector survives only where at least consensus_k of those masks agree - the
 *      "selfish" weights that serve one task and the "catastrophic" ones that serve none are dropped.  Two flavours: on
 *      top of task arithmetic (ties == 0, consensus_ta) and on top of TIES (ties == 1, consensus_ties).  The reference
 *      has no such operator; this section IS its definition.  For one tensor of n elements (any shape, flat), finetunes
 *      i = 0..k-1 in order (1 <= k <= 16):
 *        1. d_i = fp32(finetune_i) - fp32(base_i).  A NaN or Inf in any d_i fails the call with SMHIP_ERR_NONFINITE
 *           (the message lists the finetunes), detected as smhip_dare_merge detects it; out is then unspecified.
 *        2. tv_i = fl32(d_i * fp32(alpha_i)), for EVERY element: the trim of ties == 1 does not touch tv_i.
 *        3. The multi-task vector U.
 *           ties == 0: U = ((0 + tv_0) + tv_1) + ... in fp32, in order.
 *           ties == 1: U = M of smhip_ties_merge steps 2-6 at `density`, `normalize` as given: the same tie rule, thresholds,
 *           election, division by the agreeing weights and |D| < 1e-8 -> 1.
 *        4. m_i = [ |tv_i| >= fl32(fp32(mask_lambda) * |fl32(U - tv_i)|) ], an IEEE comparison: a NaN on the right
 *           (0 * inf) compares false.  An element whose deltas are all zero has every mask set (0 >= 0): it changes
 *           nothing in the output, but it does count in masked[] and in agree[k].
 *        5. c = sum_i m_i, an integer.  The element is SELECTED iff c >= min(consensus_k, k): a tensor that a layer
 *           window leaves with fewer entries than consensus_k needs all of them to agree, so one entry is taken as it
 *           is (ties == 0: U - tv_0 = 0 and its mask always holds) - the convention of the other operators.
 *        6. ties == 0: M = U / D when normalize, D = ((0 + fp32(alpha_0)) + ...) over all finetunes, D := 1 where
 *           |D| < fp32(1e-8) (the linear variants' divisor); M = U otherwise.  ties == 1: M = U.
 *           M := +0 where the element is not selected.
 *        7. out = round_to(base_out_dtype, fp32(base_out) + fl32(fp32(lambda) * M)), delta_out = fl32(lambda * M):
 *           step 7 of smhip_ties_merge.
 *      Every step is one correctly rounded fp32 operation, a comparison, an integer count or (ties == 1) an exact order
 *      statistic: the result is defined bit for bit.  With mask_lambda = 0 and consensus_k = 1 every finite element is
 *      selected: ties == 0 then equals smhip_dare_merge (sign_election 0) at density 1, ties == 1 equals
 *      smhip_ties_merge at the same density.  The selected sets are nested in consensus_k.  ties == 0 is ONE kernel, one
 *      pass over the inputs (k + 2 tensor passes); ties == 1 adds the three selection levels of TIES (4k + 5).  The k
 *      entries of an element stay in registers between the sum and the masks: no finetune is read twice by the kernel.
 *      Counters are integers (LDS, then one global atomic per counter and work-group), no floating-point atomics; the
 *      call synchronises the stream once, at its end.  Aliasing, alignment, n == 0, dtypes and the size limit: the
 *      rules of smhip_ties_merge.  SMHIP_ERR_ARG: k or consensus_k outside 1..16, mask_lambda negative, NaN or above
 *      1e6, density outside (0, 1] when ties, lambda or an alpha not finite, out overlapping an input, a bad dtype, a
 *      null descriptor.  Profile names: "consensus_merge" and, ties == 1, "ties_hist" / "ties_select". ---- */
typedef struct {
    int k;
    const void* finetune[SMHIP_MAX_MODELS]; /* device, in_dtype, [n] */
    const void* base[SMHIP_MAX_MODELS];     /* device, in_dtype: each finetune's own base */
    double alpha[SMHIP_MAX_MODELS];
    int in_dtype;                           /* SMHIP_BF16 / F16 / F32, finetunes and their bases */
    const void* base_out; int base_out_dtype;
    size_t n;
    double density, lambda; int normalize;  /* density: ties == 1 only */
    double mask_lambda;                     /* lambda of the TALL mask, 0 <= mask_lambda <= 1e6 */
    int consensus_k;                        /* masks that must agree, 1..16 (min(consensus_k, k) in effect) */
    int ties;                               /* 1: consensus_ties; 0: consensus_ta */
} smhip_consensus_desc;
typedef struct {
    uint64_t k_keep;                        /* ties == 1: as smhip_ties_report; zero otherwise, as threshold and kept */
    float threshold[SMHIP_MAX_MODELS];
    uint64_t kept[SMHIP_MAX_MODELS];
    uint64_t masked[SMHIP_MAX_MODELS];      /* elements with m_i set */
    uint64_t agree[SMHIP_MAX_MODELS + 1];   /* elements with exactly c masks set; they sum to n */
    uint64_t selected;                      /* elements with c >= min(consensus_k, k) */
} smhip_consensus_report;
/* out: device, base_out_dtype, [n].  delta_out (optional): device float [n], fl32(lambda * M).  report (optional): HOST. */
int smhip_consensus_merge(smhip_ctx* ctx, const smhip_consensus_desc* desc, void* out, float* delta_out,
                          smhip_consensus_report* report, void* stream);

/* ---- Pairwise fusion: ONE finetune grafted onto a base, element by element (the operators arcee_fusion and nearswap;
 *      both after mergekit's methods of those names, as recalled - PAPERS.md).  ARCEE takes only the updates an importance
 *      score marks as outliers, NEARSWAP limits how far any weight may move.  The reference has no such operator; this
 *      section IS their definition.  One tensor of n elements viewed as R x C: R = rows, C = n / rows (the caller passes
 *      the last dimension as C; a 1-D tensor is one row).  k must be 1 and alpha[0] is not read: the operators take no
 *      weight.  Both modes: d = fp32(finetune) - fp32(base).
 *      NEARSWAP.  t32 = fp32(t), t > 0 and finite, else SMHIP_ERR_ARG.  M = min(max(d, -t32), t32) (d where
 *      |d| <= t32, +-t32 beyond).  out = round_to(base_out_dtype, fp32(base_out) + M), delta_out = M.  clipped counts
 *      |d| > t32.  A NaN or Inf in d fails the call with SMHIP_ERR_NONFINITE.  One kernel, one pass: 4 tensor passes.
 *      mergekit writes lweight = clamp(t / |v0 - v1|, 0, 1) and interpolates; in exact arithmetic that is this clamp.
 *      ARCEE.  A NaN or Inf in the finetune or the base fails the call (the weights themselves enter the softmax), as
 *      does one in d.
 *        1. Row KL, in fp64: every operation below is ONE rounded IEEE operation, never an fma.  For row r, with
 *           x = fp32(finetune), y = fp32(base): mx = max_j x_j, my = max_j y_j, a_j = fp64(x_j) - fp64(mx),
 *           b_j = fp64(y_j) - fp64(my), ea_j = sm_exp(a_j), eb_j = sm_exp(b_j), S_a = sum ea_j, S_b = sum eb_j,
 *           U = sum ea_j * (a_j - b_j).  The three sums run in the row order of smhip_geo_merge step 2: octet o of the
 *           row (elements 8 o .. 8 o + 7 from the row's start) goes to lane o % 256, each lane adds in ascending index
 *           from +0, the 256 lanes are reduced by the binary tree p[t] += p[t + s], s = 128 .. 1.
 *           kl = U / S_a - (sm_log(S_a) - sm_log(S_b)); kappa_r = fp32(kl) where kl > 0, +0 elsewhere.
 *           This is KL(softmax(finetune row) || softmax(base row)) written through log-softmax: nothing takes the log of
 *           a probability, so the +1e-8 guard of mergekit's formula is not needed (and not part of this definition).
 *           A row equal in finetune and base gives kappa = 0 EXACTLY: every a_j - b_j is +0, so U = +0 and U / S_a = +0;
 *           S_a and S_b are the same bits, so the difference of their logarithms is +0.
 *        2. Score: s_e = fl32(|d_e| * kappa_row(e)), one fp32 multiplication.
 *        3. Quartiles: rho_q = floor(q (n - 1)) for q = 1/4, 1/2, 3/4; Q1, Q2, Q3 are the rho_q-th smallest scores
 *           (0-based), exact: no interpolation, no subsampling.  thr = fl32(Q2 + fl32(fp32(iqr_mult) * fl32(Q3 - Q1))).
 *        4. Gate: an element is selected iff s_e > thr, an IEEE fp32 comparison - strict, so ties with the threshold all
 *           go the same way and the result does not depend on order.  M = d where selected, +0 elsewhere; out and
 *           delta_out as in NEARSWAP.
 *      sm_exp and sm_log (csrc/sm_fusion.hpp) are DEFINED there: sm_exp on (-inf, 0], +0 below -45 (e^-45 < 2^-64
 *      against sums that are at least 1); sm_log on [1, 2^40).  Both: an argument reduction with a two-part ln 2, a Horner
 *      evaluation of a truncated Taylor series, the scale by a power of two, one rounded operation at a time - the
 *      host, the device, the emulator and a numpy restatement give the same bits; smhip_fusion_fn exposes them.
 *      Every value is one correctly rounded operation, an exact order statistic or an integer count in a stated order:
 *      the result is defined bit for bit.  Identities: NEARSWAP with t >= max |d|, and ARCEE with thr < 0, equal
 *      smhip_dare_merge (sign_election 0, normalize 1) at density 1 with alpha 1 (a delta of -0, which that sum turns into +0,
 *      aside); ARCEE's selected sets are nested in
 *      iqr_mult when Q3 >= Q1.  Passes (ARCEE): "fusion_rowkl" once (a work-group per row; 2 tensor passes, the second
 *      read of a row from L2), "fusion_hist" / "fusion_select" three times (all three ranks in the same 11 + 10 + 10 bit
 *      levels, the scores formed on the fly: 3 x 2), "fusion_merge" once (4): 12 tensor passes.  Counters are integers
 *      (LDS, then one global atomic per work-group), no floating-point atomics; the stream is synchronised once, at
 *      the end.  Aliasing, alignment, n == 0 (a no-op, the report all zeros), dtypes and the size limit: the rules of
 *      smhip_ties_merge.  SMHIP_ERR_ARG: k != 1, a bad mode, rows < 1 or not dividing n, t <= 0 or not finite
 *      (NEARSWAP), iqr_mult not finite (ARCEE), a null pointer, kl_out misaligned or overlapping an output. ---- */
enum { SMHIP_FUSION_ARCEE = 0, SMHIP_FUSION_NEARSWAP = 1 };
typedef struct {
    int k;                                  /* must be 1 */
    const void* finetune[SMHIP_MAX_MODELS]; /* [0]: device, in_dtype, [n] */
    const void* base[SMHIP_MAX_MODELS];     /* [0]: device, in_dtype */
    double alpha[SMHIP_MAX_MODELS];         /* not read */
    int in_dtype;                           /* SMHIP_BF16 / F16 / F32, the finetune and the base */
    const void* base_out; int base_out_dtype;
    size_t n;
    int mode;                               /* SMHIP_FUSION_ARCEE / SMHIP_FUSION_NEARSWAP */
    size_t rows;                            /* R: C = n / rows is the row of step 1 */
    double iqr_mult;                        /* ARCEE */
    double t;                               /* NEARSWAP */
    float* kl_out;                          /* ARCEE, optional: device float [rows], kappa_r */
} smhip_fusion_desc;
typedef struct {
    float q1, q2, q3, threshold;            /* ARCEE */
    uint64_t selected;                      /* ARCEE: elements with s_e > thr */
    uint64_t clipped;                       /* NEARSWAP: elements with |d| > t32 */
    float kl_min, kl_max;                   /* ARCEE: over the rows */
} smhip_fusion_report;
/* out: device, base_out_dtype, [n].  delta_out (optional): device float [n], M.  report (optional): HOST. */
int smhip_fusion_merge(smhip_ctx* ctx, const smhip_fusion_desc* desc, void* out, float* delta_out,
                       smhip_fusion_report* report, void* stream);
/* y[i] = sm_exp(x[i]) (op SMHIP_FUSION_EXP) or sm_log(x[i]) (SMHIP_FUSION_LOG) for n doubles.  on_device = 0: x and y
 * are HOST arrays, evaluated on the host; 1: DEVICE arrays, evaluated by a kernel ("fusion_fn") on the stream. */
enum { SMHIP_FUSION_EXP = 0, SMHIP_FUSION_LOG = 1 };
int smhip_fusion_fn(smhip_ctx* ctx, int op, const double* x, double* y, size_t n, int on_device, void* stream);

/* ---- PCB merge (Du et al., "Parameter Competition Balancing for Model Merging", NeurIPS 2024): every entry of every
 *      task vector gets a continuous weight of its own - how large it is within its own task (intra-balancing) times how
 *      well it agrees with what all tasks together do to that weight (inter-balancing); the low scores are dropped, the
 *      rest are averaged with their scores as weights.  The reference has no such operator; this section IS its
 *      definition.  For one tensor of n elements (any shape, flat), finetunes i = 0..k-1 in order (1 <= k <= 16), and
 *      the parameters ratio in (0, 1], clip in [0, 0.5) and lambda:
 *        1. d_i = fp32(finetune_i) - fp32(base_i), tv_i = fl32(d_i * fp32(alpha_i)): one fp32 subtraction, one fp32
 *           multiplication, as smhip_consensus_merge forms them; alpha_i of any sign, or zero.  A NaN or Inf in any d_i
 *           fails the call with SMHIP_ERR_NONFINITE (the message lists the finetunes); out is then unspecified.
 *        2. Clip.  r = (uint64) floor(clip * n) in fp64.  Per finetune, with the n values |tv_i| in ascending order
 *           (0-based): lo_i is the one at index r, hi_i the one at index n - 1 - r - exact order statistics, whatever the
 *           traversal order; r < n / 2, so lo_i <= hi_i.  fl32(|d| * |alpha|) is monotone in |d|, so they are computed as
 *           lo_i = |fl32(q * fp32(alpha_i))| for the same order statistics q of |d_i|.  c_i = min(max(|tv_i|, lo_i), hi_i);
 *           tvc_i = copysign(c_i, tv_i), and +0 where tv_i == 0.
 *        3. Intra-balancing, in fp64, every operation ONE rounded IEEE operation, never an fma:
 *           s_i = (fp64(c_i) - fp64(lo_i)) / (fp64(hi_i) - fp64(lo_i)), and 0 where hi_i == lo_i; 0 <= s_i <= 1.
 *           intra_i = sm_exp(fp64(k) * (s_i * s_i - 1)): the argument lies in [-16, 0].  The paper's exp(k s^2) is this
 *           times the constant e^k, which cancels in step 7.
 *        4. Inter-balancing.  U = ((0 + tv_0) + tv_1) + ... in fp32, in order, over the UNCLIPPED entries.
 *           x_i = fp64(tv_i) * fp64(U) (exact), inter_i = sm_tanh(x_i).
 *        5. Score.  p_i = intra_i * inter_i in fp64; S_i = fp32(p_i) (one rounding to nearest even) where
 *           p_i >= 2^-126, compared in fp64, and +0 elsewhere - so a score is +0 or a NORMAL positive fp32 number and
 *           the result depends on no denormal mode.  An entry that opposes the sum of its element, or is zero, scores 0
 *           and is never selected.  DEVIATION: the paper's code applies tanh unclamped, so a negative score can receive a
 *           positive weight there once ratio exceeds the share of agreeing entries; here it cannot.
 *        6. Select and weigh.  q = max(1, (uint64) floor(ratio * n)) (n when ratio == 1).  Per finetune t_i is the q-th
 *           largest of its n scores (+0 when fewer than q are positive) and M_i the largest, both exact.
 *           scale_i = 0 where S_i < t_i or S_i == 0; else 1 where M_i == t_i; else fl32(fl32(S_i - t_i) / fl32(M_i - t_i)).
 *           The weight is continuous at the threshold - an entry equal to t_i < M_i weighs 0 - so the tie rule changes
 *           the counts only.
 *        7. merged = fl32(num / max(den, fp32(1e-12))), num = ((0 + fl32(scale_0 * tvc_0)) + ...), den = ((0 + scale_0) +
 *           ...), fp32, in order; out = round_to(base_out_dtype, fl32(fp32(base_out) + fl32(fp32(lambda) * merged)));
 *           delta_out = merged (NOT times lambda).
 *      sm_tanh (csrc/sm_pcb.hpp) is DEFINED there, next to sm_exp and in its manner.  |x| < 2^-4: x * P(x * x), P the
 *      series 1, -1/3, 2/15, -17/315, 62/2835, -1382/155925, 21844/6081075, -929569/638512875, 6404582/10854718875 (each
 *      rounded to fp64) in Horner form.  2^-4 <= |x| <= 22.5: (1 - e) / (1 + e) with e = sm_exp(-2 |x|), the sign of x.
 *      Beyond: +-1.  sm_tanh(+-0) = +-0.  One rounded operation at a time: the host, the device, the emulator and a numpy
 *      restatement give the same bits; smhip_pcb_fn exposes it.
 *      Report: lo, hi, t, M per finetune; positive[i] = #{S_i > 0}; selected[i] = #{S_i >= t_i and S_i > 0};
 *      covered = #{den > 0}; contested = #{at least two finetunes with scale > 0}.
 *      Every value is one correctly rounded operation, an exact order statistic or an integer count in a stated order:
 *      the result is defined bit for bit.  Passes: "stats_hist" / "stats_select" three times (the two ranks of step 2 in
 *      the same 11 + 10 + 10 bit levels over the magnitude bits), "pcb_hist" / "stats_select" three times (the two ranks of
 *      step 6 over the score stream, recomputed from the inputs, lo, hi and U in every pass: no score is cached),
 *      "pcb_merge" once: 3 (k + 1) + 3 (k + 1) + (k + 2) = 7 k + 8 tensor passes with a shared base and k <= 4 (beyond,
 *      pcb_hist runs once per group of four finetunes and reads all k each time).  Counters are integers (LDS, then one
 *      global atomic per counter and work-group), no floating-point atomics; the stream is synchronised once, at the
 *      end.  Aliasing, alignment, n == 0 (a no-op, the report all zeros), dtypes and the size limit: the rules of
 *      smhip_ties_merge.  SMHIP_ERR_ARG: k outside 1..16, ratio outside (0, 1], clip outside [0, 0.5), lambda or an
 *      alpha not finite, out overlapping an input, a bad dtype, a null pointer. ---- */
typedef struct {
    int k;
    const void* finetune[SMHIP_MAX_MODELS]; /* device, in_dtype, [n] */
    const void* base[SMHIP_MAX_MODELS];     /* device, in_dtype: each finetune's own base */
    double alpha[SMHIP_MAX_MODELS];
    int in_dtype;                           /* SMHIP_BF16 / F16 / F32, finetunes and their bases */
    const void* base_out; int base_out_dtype;
    size_t n;
    double ratio;                           /* 0 < ratio <= 1: the share of each finetune's scores that is kept */
    double clip;                            /* 0 <= clip < 0.5: the share of magnitudes clamped at either end */
    double lambda;
} smhip_pcb_desc;
typedef struct {
    uint64_t clip_rank;                     /* r */
    uint64_t q;                             /* scores asked for per finetune */
    float lo[SMHIP_MAX_MODELS], hi[SMHIP_MAX_MODELS];     /* the clip bounds of |tv_i| */
    float t[SMHIP_MAX_MODELS], M[SMHIP_MAX_MODELS];       /* the q-th largest and the largest score */
    uint64_t positive[SMHIP_MAX_MODELS];    /* entries with S_i > 0 */
    uint64_t selected[SMHIP_MAX_MODELS];    /* entries with S_i >= t_i and S_i > 0 */
    uint64_t covered;                       /* elements with den > 0 */
    uint64_t contested;                     /* elements where at least two finetunes have scale > 0 */
} smhip_pcb_report;
/* out: device, base_out_dtype, [n].  delta_out (optional): device float [n], merged.  report (optional): HOST. */
int smhip_pcb_merge(smhip_ctx* ctx, const smhip_pcb_desc* desc, void* out, float* delta_out,
                    smhip_pcb_report* report, void* stream);
/* y[i] = sm_tanh(x[i]) (op SMHIP_PCB_TANH) for n doubles.  on_device = 0: x and y are HOST arrays, evaluated on the
 * host; 1: DEVICE arrays, evaluated by a kernel ("pcb_fn") on the stream. */
enum { SMHIP_PCB_TANH = 0 };
int smhip_pcb_fn(smhip_ctx* ctx, int op, const double* x, double* y, size_t n, int on_device, void* stream);

/* ---- Task-vector statistics: what the knobs of the delta merges (density above all) would do to THESE finetunes,
 *      before a merge has run.  No output tensor: for one tensor of n elements (any shape, flat), finetunes i = 0..k-1
 *      (1 <= k <= 16) and candidate densities rho_q, q = 0..m-1 (1 <= m <= SMHIP_STATS_MAX_DENSITIES, each in (0, 1],
 *      any order, duplicates allowed), the report holds:
 *        1. d_i = fp32(finetune_i) - fp32(base_i).  A NaN or Inf in any d_i fails the call with SMHIP_ERR_NONFINITE
 *           (the message lists the finetunes, as smhip_ties_merge does).  nonzero[i] = #{d_i != 0}.
 *        2. G[i][j] (symmetric): step 2 of smhip_geo_merge in delta space over the whole tensor - segments of 32768
 *           elements, octet o to lane o % 256, the binary tree over the lanes, the segments added in index order.
 *        3. k_keep[q] = n if rho_q == 1, else (uint64) floor(rho_q * n) in fp64.  tau[q][i] = the k_keep[q]-th largest
 *           |d_i|, exact; +inf when k_keep[q] == 0.  Entry (q, i) of an element is KEPT iff |d_i| >= tau[q][i] and
 *           d_i != 0: step 2 of smhip_ties_merge with its tie rule.  kept[q][i] counts the kept entries.
 *        4. energy[q][i] = sum over the elements of (double) x * (double) x, x = d_i where kept and +0 elsewhere, summed
 *           in the order of 2 (how smhip_sce_merge step 3 sums, with this step's mask).
 *        5. For every q, each operation one rounded fp32 operation: tv_i = fl32(d_i * fp32(alpha_i)) where kept, +0
 *           elsewhere; S = ((0 + tv_0) + tv_1) + ...; the elected sign is + when S >= 0; m_i = [sign(tv_i) == elected
 *           sign], a zero agrees with nothing (steps 3-5 of smhip_ties_merge; Yadav et al. 2023).  Then, all uint64:
 *             opposed[q][i]  #{kept and m_i == 0}: what TIES at this density discards of finetune i
 *             alone[q][i]    #{kept by i and by no other finetune}
 *             cover[q][c]    c = 0..k: elements that exactly c finetunes keep
 *             conflict[q]    elements with a kept tv > 0 and a kept tv < 0
 *      Every value is an integer, an exact order statistic or an fp64 sum in a stated order: the report is defined bit
 *      for bit, the same on any grid.  Identities: tau[q][i] and kept[q][i] equal smhip_ties_merge's report at density
 *      rho_q; energy[q][i] at rho_q == 1 equals G[i][i] bit for bit (a zero adds +0); G equals the Gram that
 *      smhip_geo_merge (MODEL_STOCK) reports on the same inputs; sum_c cover[q][c] == n;
 *      sum_c c * cover[q][c] == sum_i kept[q][i]; sum_i alone[q][i] == cover[q][1].
 *      Passes: the radix select finds all m thresholds of a finetune in the same three levels (a 2048-bin histogram per
 *      finetune at level 1, a 1024-bin histogram per distinct prefix at levels 2 and 3), then the Gram pass, then ONE
 *      fused pass for everything else: with a shared base and k <= 4 the call reads 5 (k + 1) tensors, whatever m
 *      (k > 4: the Gram pass re-reads per tile of pairs, as in smhip_geo_merge).  Counters are integers (LDS, then one
 *      global atomic per counter and work-group), no floating-point atomics; the stream is synchronised once, at the
 *      end.  Aliasing, alignment, dtypes and the size limit: the rules of smhip_ties_merge's inputs.  n == 0: the report
 *      is all zeros and tau is +inf.  SMHIP_ERR_ARG: k outside 1..16, m outside 1..4, a density outside (0, 1], an alpha
 *      not finite, a bad dtype, a null descriptor, report or tensor.
 *      Profile names: "stats_hist", "stats_select", "geo_gram", "geo_gram_fold", "stats_pass", "stats_fold". ---- */
#define SMHIP_STATS_MAX_DENSITIES 4
typedef struct {
    int k;
    const void* finetune[SMHIP_MAX_MODELS]; /* device, in_dtype, [n] */
    const void* base[SMHIP_MAX_MODELS];     /* device, in_dtype: each finetune's own base */
    double alpha[SMHIP_MAX_MODELS];         /* the election's weights (step 5 only) */
    int in_dtype;                           /* SMHIP_BF16 / F16 / F32, finetunes and their bases */
    size_t n;
    int m;                                  /* densities, 1..SMHIP_STATS_MAX_DENSITIES */
    double density[SMHIP_STATS_MAX_DENSITIES];
} smhip_stats_desc;
typedef struct {
    uint64_t nonzero[SMHIP_MAX_MODELS];
    double G[SMHIP_MAX_MODELS][SMHIP_MAX_MODELS];
    uint64_t k_keep[SMHIP_STATS_MAX_DENSITIES];
    float tau[SMHIP_STATS_MAX_DENSITIES][SMHIP_MAX_MODELS];
    uint64_t kept[SMHIP_STATS_MAX_DENSITIES][SMHIP_MAX_MODELS];
    double energy[SMHIP_STATS_MAX_DENSITIES][SMHIP_MAX_MODELS];
    uint64_t opposed[SMHIP_STATS_MAX_DENSITIES][SMHIP_MAX_MODELS];
    uint64_t alone[SMHIP_STATS_MAX_DENSITIES][SMHIP_MAX_MODELS];
    uint64_t cover[SMHIP_STATS_MAX_DENSITIES][SMHIP_MAX_MODELS + 1];
    uint64_t conflict[SMHIP_STATS_MAX_DENSITIES];
} smhip_stats_report;
/* report: HOST, required. */
int smhip_delta_stats(smhip_ctx* ctx, const smhip_stats_desc* desc, smhip_stats_report* report, void* stream);

/* ---- slerp (reference shard/tensor/functions.py:24-43) on fp32 device tensors of rows x cols elements (1-D:
 *      rows = 1): the cosine is taken between the UN-normalised vectors over the whole tensor, the relative vector
 *      v1 - v0 dot is normalised along the LAST dimension (F.normalize(dim=-1), eps 1e-12), out = v0 cos + rel sin.
 *      rows * cols = 0: nothing to do.  A zero vector gives NaN, as in the reference. ---- */
int smhip_slerp(smhip_ctx* ctx, const float* v0, const float* v1, size_t rows, size_t cols, float t, float* out, void* stream);

/* ---- the two halves of normalize_tensor (functions.py:75-88: norm = tensor.norm().item(); tensor / norm):
 *      smhip_exact_norm - ||x||_2 accumulated in fp64 (the norm as torch.norm computes it on CPU, rounding bias
 *      included, is smhip_reference_cpu_norm); norm_out: HOST double.
 *      smhip_div_scalar - out = x / s in x's dtype (a 16-bit tensor over a Python float: an fp32 division rounded
 *      to the dtype, as torch does it); out may be x. ---- */
int smhip_exact_norm(smhip_ctx* ctx, const void* x, int dtype, size_t n, double* norm_out, void* stream);
int smhip_div_scalar(smhip_ctx* ctx, const void* x, int dtype, size_t n, float s, void* out, void* stream);

/* ---- LoRA: the finetune weight a LoRA adapter defines, W = base + scale * (lora_b @ lora_a).
 *      out = round_dtype(base + scale * (lora_b @ lora_a)), all row-major: base/out [rows x cols] of `dtype`,
 *      lora_a [rank x cols], lora_b [rows x rank] of `factor_dtype` (SMHIP_BF16/F16/F32); 1 <= rank <= 512;
 *      out must not overlap an input.  Any rows, cols >= 1 (no transform plan involved).  The product is
 *      accumulated in fp32 (16-bit factors on MFMA, products exact) and added as fma(scale, sum, base), rounded
 *      once into `dtype`.  Pointers need only the alignment of their element type.  Profile names:
 *      "lora_pack" (the factors copied k-contiguous into the workspace) and "lora_apply". ---- */
int smhip_lora_apply(smhip_ctx* ctx, const void* base, int dtype, int rows, int cols,
                     const void* lora_a, const void* lora_b, int factor_dtype, int rank, float scale,
                     void* out, void* stream);

/* ---- adapters: the finetune weight of a PEFT LoRA / DoRA / embedding-LoRA module, one descriptor.
 *      LINEAR:    lora_a [rank x cols], lora_b [rows x rank]; out = round(base + scale * (lora_b @ lora_a)), exactly
 *                 smhip_lora_apply's result when magnitude is NULL.
 *      EMBEDDING: lora_a = lora_embedding_A [rank x rows], lora_b = lora_embedding_B [cols x rank];
 *                 out = round(base + scale * (lora_a^T @ lora_b^T)), the same one-rounding contract.
 *      magnitude (LINEAR only, NULL for plain LoRA): DoRA, [rows] of magnitude_dtype (SMHIP_BF16/F16/F32).  With
 *                 v = base + scale * (lora_b @ lora_a) as the LoRA path forms it before rounding,
 *                 out[i][:] = round(v[i][:] * f[i]), f[i] = magnitude[i] / ||v[i][:]||_2 in fp64 (row norm over cols).
 *                 A row whose f is not finite (zero or non-finite norm, non-finite magnitude) fails the call with
 *                 SMHIP_ERR_ROW_NORM naming the row; out is then unspecified.  The call synchronises the stream.
 *      Same argument, alignment and overlap rules as smhip_lora_apply, the magnitude included; DoRA with EMBEDDING is
 *      SMHIP_ERR_ARG.  Profile names: "lora_pack", "lora_apply"; DoRA: "dora_norm", "dora_scale", "dora_apply". ---- */
enum { SMHIP_ADAPTER_LINEAR = 0, SMHIP_ADAPTER_EMBEDDING = 1 };
typedef struct {
    const void* base; int dtype; int rows, cols;
    const void* lora_a; const void* lora_b; int factor_dtype; int rank; float scale;
    int layout;                    /* SMHIP_ADAPTER_LINEAR / SMHIP_ADAPTER_EMBEDDING */
    const void* magnitude;         /* NULL: plain LoRA; else DoRA (LINEAR only), [rows] of magnitude_dtype */
    int magnitude_dtype;
    void* out;
} smhip_adapter_desc;
int smhip_adapter_apply(smhip_ctx* ctx, const smhip_adapter_desc* d, void* stream);

/* ---- extract-lora: the other direction - a rank-r adapter (A [r x cols], B [rows x r], lora_alpha = r, scale 1) from one
 *      2-D finetune and its base, D = fp32(finetune) - fp32(base) (one fp32 subtraction), B A ~ D.  A randomized subspace
 *      iteration (Halko, Martinsson, Tropp 2011) with a Gram-space orthonormalisation: the small algebra runs on L x L
 *      matrices, no tensor-sized matrix is factorised, and every value is defined step by step (csrc/sm_extract.hpp).
 *      1 <= r <= 256, power iterations 0 <= q <= 4, L = min(ceil16(r + 8), ceil16(min(rows, cols))) <= 272.
 *        1. Sketch.  Omega [cols x L] fp32: entry e = i * L + j is +1 when bit (e & 31) of word ((e >> 5) & 3) of the
 *           Philox4x32-10 block with counter (lo32(e >> 7), hi32(e >> 7), 0, 0) under `key` is 0, else -1.
 *        2. Y = D Omega [rows x L].
 *        3. q times: Q = orth(Y); Z = D^T Q [cols x L]; Q' = orth(Z); Y = D Q'.
 *        4. Q = orth(Y); C = D^T Q [cols x L].
 *        5. G_C = gram(C) = V diag(lambda) V^T (eig below), sigma_i = sqrt(max(lambda_i, 0)).  With n = min(r, L):
 *           rho = #{i < n : lambda_i > 1e-12 * lambda_0}.  s_i = sqrt(sigma_i);  Tb[k][i] = fp32(V[k][i] * s_i),
 *           Ta[k][i] = fp32(V[k][i] / s_i) for i < rho, zero columns for rho <= i < r;  B = round(pmm(Q, Tb)),
 *           A = round(pmm(C, Ta))^T, each rounded once into factor_dtype; rows / columns i >= rho are exact zeros.
 *        6. orth(Y): G = gram(Y) = V diag(lambda) V^T; T[:, i] = fp32(V[:, i] / sqrt(lambda_i)) where
 *           lambda_i > 1e-12 * lambda_0, else a zero column; Q = pmm(Y, T).  The kept rank of every call is reported.
 *           (Symmetric orthonormalisation with truncation: a finetune that is a merged low-rank adapter has a singular Gram.)
 *        7. delta_sq = ||D||_F^2: step 2 of smhip_geo_merge in delta space with k = 1.  share = (((0 + sigma_0^2) + ...
 *           + sigma_{n-1}^2) / delta_sq with sigma_i^2 = max(lambda_i, 0), 0 when delta_sq == 0.
 *      The products.  D X and D^T X run on v_mfma_f32_16x16x4_f32, bit for bit a k-ordered fp32 fma chain.  The reduction
 *      index is cut into segments of 512; within a segment every output element is ONE fma chain from +0, the segments'
 *      results are added in index order in fp32 (((0 + p_0) + p_1) + ...).  D^T X: the chain runs k = 512 s, 512 s + 1,
 *      ..., padded with products of two +0 to a multiple of 4.  D X: inside every block of 32 consecutive k the chain
 *      visits k0 + 8 g + j in the order j = 0..7 (outer), g = 0..3 (inner) - a lane's 16-byte load feeds one k of eight
 *      instructions - and the segment is padded with products of two +0 to a multiple of 32.
 *      gram(P) [L x L], fp64 (products of fp32 values are exact): rows in segments of 256; within a segment
 *      s_c = the sum over rows c, c + 4, ... in order (c = 0..3), the segment's value (s_0 + s_2) + (s_1 + s_3); segments
 *      added in index order.  pmm(P, T)[m][j] = the fp32 fma chain over k = 0..L-1 of P[m][k] * T[k][j] from +0.
 *      eig: cyclic Jacobi in fp64, one rounded operation at a time, fixed sweep order, stopping rule, descending order and
 *      sign convention as stated at xl_sym_eig in csrc/sm_extract.hpp.
 *      A NaN or Inf in D reaches the first panel and fails the call with SMHIP_ERR_NONFINITE.  The workspace is the
 *      caller's: DEVICE memory, 256-byte aligned, at least smhip_lora_extract_workspace(rows, cols, rank) bytes, else
 *      SMHIP_ERR_ARG; as are a null pointer, r outside 1..256, q outside 0..4, a bad dtype, rows or cols < 1, a pointer
 *      not aligned to its element.  Passes: 2 q + 2 delta products, each reading finetune and base once (L <= 80; one more
 *      read per further 80 columns).  The stream is synchronised once per orth and once at the end.
 *      Profile names and launches per call: "xl_fill" 1, "xl_delta_mm" and "xl_fold" 2 q + 2 each, "xl_gram" and
 *      "xl_gram_fold" 2 q + 2 each, "xl_panel_mm" 2 q + 3, "geo_gram" and "geo_gram_fold" 1 each. ---- */
#define SMHIP_EXTRACT_MAX_L 272
#define SMHIP_EXTRACT_MAX_ORTH 9
typedef struct {
    const void* finetune; const void* base; /* device, in_dtype, [rows x cols] */
    int in_dtype;
    int rows, cols;
    int rank;                               /* r, 1..256 */
    int power_iters;                        /* q, 0..4 */
    uint64_t key;
    int factor_dtype;                       /* of A and B */
    void* workspace; size_t workspace_bytes;
} smhip_extract_desc;
typedef struct {
    int L;                                  /* the panel width */
    int rho;                                /* the effective rank, <= min(r, L) */
    int n_orth;                             /* orth calls: 2 q + 1 */
    int orth_rank[SMHIP_EXTRACT_MAX_ORTH];  /* the rank each kept */
    double sigma[SMHIP_EXTRACT_MAX_L];      /* sigma[0 .. L) */
    double delta_sq;                        /* ||D||_F^2 */
    double share;                           /* the captured energy share */
} smhip_extract_report;
size_t smhip_lora_extract_workspace(int rows, int cols, int rank);
/* a_out [rank x cols], b_out [rows x rank]: device, factor_dtype.  report: HOST, required. */
int smhip_lora_extract(smhip_ctx* ctx, const smhip_extract_desc* desc, void* a_out, void* b_out,
                       smhip_extract_report* report, void* stream);
/* TEST ABI, not part of the stable surface and free to change with the kernels: the probe of the primitives, one per
 * call.  FILL y = the Rademacher panel [rows x L] under key; DELTA_MM
 * y [M x L] = D X or D^T X (trans) with its fold, x [K x L]; GRAM y = gram(x), x [rows x L] fp32, y fp64 [L x L];
 * PANEL_MM y = pmm(x [rows x L], t [L x L2]) in out_dtype, stored transposed when trans; x, t, y DEVICE.
 * SYM_EIG: x HOST fp64 [L x L], y HOST fp64 [L + L * L]: lambda, then V row-major.  The workspace as above (for L). */
enum { SMHIP_XL_FILL = 0, SMHIP_XL_DELTA_MM = 1, SMHIP_XL_GRAM = 2, SMHIP_XL_PANEL_MM = 3, SMHIP_XL_SYM_EIG = 4 };
typedef struct {
    int op;
    const void* finetune; const void* base; int in_dtype;
    int rows, cols, L, L2, trans;
    uint64_t key;
    const void* x; const float* t; void* y; int out_dtype;
    void* workspace; size_t workspace_bytes;
} smhip_xl_probe_desc;
size_t smhip_xl_probe_workspace(int rows, int cols, int L);    /* DELTA_MM: (rows, cols, L); GRAM: (rows, 1, L) */
int smhip_xl_probe(smhip_ctx* ctx, const smhip_xl_probe_desc* desc, void* stream);

/* ---- TSV merge (Gargiulo et al. 2025, "Task Singular Vectors"): the one operator that treats a task vector as a matrix.
 *      One 2-D tensor [rows x cols], finetunes i = 0..k-1 in order, each with its own base and a weight alpha_i >= 0.
 *      An entry with alpha_i == 0 is inactive: it is not read and its report fields are zero; k_a counts the others.
 *      rank 1..256, power iterations q 0..4, r = min(rank, rows, cols), L = xl_panel_width(rows, cols, r) =
 *      min(ceil16(r + 8), ceil16(min(rows, cols))), and k_a * r <= 256.  Every primitive (the sketch, the delta products,
 *      orth, gram, pmm, eig) is the one stated at smhip_lora_extract.
 *        1. Per active finetune, steps 1 - 4 of smhip_lora_extract on D_i = fp32(finetune_i) - fp32(base_i) with ONE
 *           sketch Omega [cols x L] under `key` for the whole call: Q_i [rows x L], C_i = D_i^T Q_i [cols x L], the orth
 *           ranks, and delta_sq_i as its step 7.  A NaN or Inf fails the call with SMHIP_ERR_NONFINITE (the message
 *           names the finetune); out is then unspecified.
 *        2. Singular triplets.  gram(C_i) = V_i diag(lambda_i) V_i^T (eig), sigma_ij = sqrt(max(lambda_ij, 0)),
 *           rho_i = #{j < r : lambda_ij > 1e-12 * lambda_i0} (these j are a prefix: lambda descends), share_i =
 *           (((0 + sigma_i0^2) + ...) + sigma_i,r-1^2) / delta_sq_i with sigma^2 = max(lambda, 0), 0 when delta_sq_i == 0.
 *           U_i = pmm(Q_i, fp32(V_i[:, :rho_i])) [rows x rho_i], W_i = pmm(C_i, T_i), T_i[:, j] = fp32(V_i[:, j] / sigma_ij)
 *           [cols x rho_i].  R = sum rho_i, Rp = ceil16(R).  U [rows x Rp] and W [cols x Rp] hold the blocks side by side
 *           in finetune order; columns R .. Rp are exact zeros.  s = concat_i(alpha_i * sigma_ij, j < rho_i), fp64, one
 *           multiplication each.  R == 0: merged = +0 everywhere and steps 3 - 4 do not run.
 *        3. Whitening (Loewdin).  G_U = the leading R x R block of gram(U) = E diag(mu) E^T (eig).  In fp64, ONE rounded
 *           operation at a time, j in index order over the kept j = {mu_j > 1e-6 * mu_0}:
 *           S_U[a][b] = S_U[a][b] + (E[a][j] * E[b][j]) / sqrt(mu_j), from 0.  kept_U = their number.  S_W, mu_W, kept_W
 *           from W alike.  (1e-6 is a constant of the definition: the panels are fp32, a Gram eigenvalue far below
 *           R * 2^-23 of the largest is rounding, and two identical finetunes produce exact duplicates that fall under it.)
 *        4. Core.  M[a][b] = ((0 + t_0) + t_1) + ... over c = 0..R-1 with t_c = (S_U[a][c] * s_c) * S_W[c][b], fp64, one
 *           rounded operation at a time; M32 [Rp x Rp] = fp32(M), zero beyond R.  B = pmm(U, M32) [rows x Rp].
 *        5. Apply ("tsv_apply", v_mfma_f32_16x16x4_f32).  merged[m][n] is ONE fp32 fma chain from +0 over the products
 *           B[m][k] * W[n][k]; inside every block of 16 consecutive k the chain visits k0 + 4 g + j in the order
 *           j = 0..3 (outer), g = 0..3 (inner) - a lane's 16-byte load feeds one k of four instructions.
 *           out = round_to(base_out_dtype, fma(fp32(lambda), merged, fp32(base_out))) (one rounding, then the dtype's);
 *           delta_out = merged (NOT times lambda).
 *      At k_a = 1 the result is the rank-r truncation of D_0 times alpha_0 (whitening an orthonormal block changes it
 *      by rounding only).  Every value is defined bit for bit.  Passes: k_a (2 q + 2) delta products of two tensor
 *      reads each, k_a reads of both for delta_sq, base_out read and out written once.  Profile names: those of
 *      smhip_lora_extract ("xl_fill" once per call) and "tsv_apply" once.  The stream is synchronised at every orth and
 *      eig.  The workspace is the caller's: DEVICE memory, 256-byte aligned, at least
 *      smhip_tsv_workspace(rows, cols, k, rank) bytes.  SMHIP_ERR_ARG: k outside 1..16, a negative or non-finite alpha,
 *      lambda not finite, rank outside 1..256, q outside 0..4, k_a * r > 256, n != rows * cols, rows or cols < 1 (n > 0),
 *      a bad workspace, and the aliasing, alignment, dtype and null-pointer rules of smhip_ties_merge.  n == 0: a no-op,
 *      the report all zeros. ---- */
#define SMHIP_TSV_MAX_R 256
typedef struct {
    int k;
    const void* finetune[SMHIP_MAX_MODELS]; /* device, in_dtype, [rows x cols] */
    const void* base[SMHIP_MAX_MODELS];     /* device, in_dtype: each finetune's own base */
    double alpha[SMHIP_MAX_MODELS];         /* >= 0; 0: the entry is skipped */
    int in_dtype;
    const void* base_out; int base_out_dtype;
    size_t n;                               /* rows * cols */
    int rows, cols;
    int rank;                               /* 1..256 */
    int power_iters;                        /* q, 0..4 */
    double lambda;
    uint64_t key;
    void* workspace; size_t workspace_bytes;
} smhip_tsv_desc;
typedef struct {
    int L, r, R, Rp;
    int rho[SMHIP_MAX_MODELS];
    int n_orth[SMHIP_MAX_MODELS];           /* 2 q + 1 per active finetune */
    int orth_rank[SMHIP_MAX_MODELS][SMHIP_EXTRACT_MAX_ORTH];
    double sigma[SMHIP_MAX_MODELS][SMHIP_TSV_MAX_R];      /* sigma_i[0 .. r) */
    double delta_sq[SMHIP_MAX_MODELS], share[SMHIP_MAX_MODELS];
    double mu_U[SMHIP_TSV_MAX_R], mu_W[SMHIP_TSV_MAX_R];  /* [0 .. R) */
    int kept_U, kept_W;
} smhip_tsv_report;
size_t smhip_tsv_workspace(int rows, int cols, int k, int rank);   /* 0: a bad argument */
/* out: device, base_out_dtype, [rows x cols].  delta_out (optional): device float, merged.  report (optional): HOST. */
int smhip_tsv_merge(smhip_ctx* ctx, const smhip_tsv_desc* desc, void* out, float* delta_out,
                    smhip_tsv_report* report, void* stream);
/* TEST ABI, as smhip_xl_probe: "tsv_apply" alone.  b [rows x Rp], w [cols x Rp]: DEVICE fp32 panels, contiguous rows,
 * element-aligned; Rp a multiple of 16, 0..256. */
int smhip_tsv_probe(smhip_ctx* ctx, const float* b, const float* w, int rows, int cols, int Rp, const void* base_out,
                    int base_out_dtype, double lambda, void* out, float* delta_out, void* stream);

/* ---- Iso-C merge (Marczak et al. 2025, "No Task Left Behind: Isotropic Model Merging with Common and Task-Specific
 *      Subspaces"): the task-arithmetic sum T = sum_i alpha_i (finetune_i - base_i) of one 2-D tensor [rows x cols], with
 *      SVD T = U S V^T, has its spectrum replaced by its mean: merged = mean(S) U V^T.  U V^T is the orthogonal polar
 *      factor of T and mean(S) = <U V^T, T> / min(rows, cols), so no SVD is taken: a Newton-Schulz iteration finds the
 *      polar factor with matrix products alone.  s = min(rows, cols) <= 16384, L = max(rows, cols).
 *      gemm(A, B) below is "iso_gemm": every element is ONE fp32 fmaf chain from +0 over the products in ASCENDING k,
 *      followed, when the number of products is odd, by one step fmaf(+0, +0, acc) (which changes -0 to +0 and nothing
 *      else); a symmetric product is computed for m >= n (by whole 128 x 128 tiles; inside a diagonal tile both halves,
 *      which are equal bit for bit because fp32 products commute) and mirrored.  An ordered sum is fp64 in the order of
 *      smhip_geo_merge's Gram: segments of 32768 elements of the row-major matrix, inside a segment lane t of 256 adds the
 *      elements of the octets t, t + 256, ... one after another from 0, the 256 lane sums go through the binary tree
 *      p[t] += p[t + h], h = 128 .. 1, and the segments are added in index order from 0.
 *        1. The sum.  T[e] = ((0 + d_0 * a_0) + d_1 * a_1) + ..., d_i = fp32(finetune_i) - fp32(base_i), a_i = fp32(alpha_i):
 *           one rounded fp32 operation at a time - dare_linear at density 1 without normalisation.  Alphas of any sign.
 *           A NaN or Inf in a d_i fails the call with SMHIP_ERR_NONFINITE (the message names the finetunes).
 *        2. Orientation.  X = T when rows <= cols, else T^T (a copy): [s x L], row-major.  Everything below runs on the
 *           oriented matrix, so transposed inputs give the transposed output bit for bit.
 *        3. Scale.  nu = sqrt(ordered sum of X_ij^2) (a product of two fp32 values is exact in fp64).  nu not finite:
 *           SMHIP_ERR_NONFINITE.  nu == 0: zero = 1, merged = +0 and step 6 runs with it; no iteration.
 *           X_0 = X * fp32(1 / nu), 1 / nu one fp64 division.
 *        4. Iteration, t = 0, 1, ...:  G = gemm(X_t, X_t^T) [s x s], symmetric.
 *           e_t = sqrt((ordered sum of ((fp64(G_ij) - [i == j]) squared)) / s): the subtraction, the square, each addition,
 *           the division and the root are one rounded fp64 operation each.  e_t not finite: SMHIP_ERR_NONFINITE.
 *           e_t <= tol: converged, Q = X_t.  Else t == max_iter: not converged, Q = X_t, and no error.
 *           The quintic phase lasts while e_t > 0.35 AND (t == 0 or e_t < e_{t-1}); it ends for good at the first t where
 *           either fails.  (The quintic does not converge: it throws the spectrum into a band around 1, about
 *           [0.68, 1.13], where e settles between 0.35 and 0.40 - above the threshold on many inputs, a 128 x 128 Gaussian
 *           among them.  A residual that stops falling is that band; from it, and from any spectrum below sqrt(3), the
 *           cubic converges monotonically.)
 *           The quintic step: P = fmaf(c5, gemm(G, G), b5 * G) (symmetric), X_{t+1} = fmaf(a5, X_t, gemm(P, X_t)),
 *           (a5, b5, c5) = (0x1.b8e56p+1, -0x1.31999ap+2, 0x1.040832p+1) = fp32(3.4445, -4.7750, 2.0315).
 *           The cubic step: X_{t+1} = fmaf(1.5, X_t, -0.5 * gemm(G, X_t)).
 *           steps[t] is 'q' or 'c'; iterations = the number of steps taken.
 *        5. N = ordered sum of Q_ij * X_ij over the UNSCALED oriented X of step 2; sigma_bar = N / s (fp64).  Not finite:
 *           SMHIP_ERR_NONFINITE.
 *        6. merged = fp32(sigma_bar) * Q, oriented back; out = round_to(base_out_dtype, fma(fp32(lambda), merged,
 *           fp32(base_out))); delta_out = merged (NOT times lambda).
 *      A T without full rank (merged LoRA adapters) has directions in its null space that are whatever rounding puts
 *      there, amplified to singular value 1 - as arbitrary as the SVD's basis of the null space in the paper's form, and
 *      the same bits everywhere.  It is not guarded against.  Passes: the k finetunes and their bases read once;
 *      3 gemm per quintic step, 2 per cubic step and one more for the last G.  Profile names: "iso_sum",
 *      "iso_transpose" (rows > cols only: 2, or 1 when T is zero), "iso_norm", "iso_scale", "iso_gemm_nt", "iso_gemm_nn", "iso_resid", "iso_dot",
 *      "iso_apply", "geo_gram_fold".  The stream is synchronised once per e_t, once for nu and once for N.  The
 *      workspace is the caller's: DEVICE memory, 256-byte aligned, at least smhip_iso_workspace(rows, cols) bytes -
 *      three [rows x cols] and two [s x s] fp32 buffers and the sums' partials.  SMHIP_ERR_ARG: k outside 1..16, a
 *      non-finite alpha or lambda, tol outside (0, 1], max_iter outside 0..200, n != rows * cols, rows or cols < 1
 *      (n > 0), s > 16384, a bad workspace, and the aliasing, alignment, dtype and null-pointer rules of
 *      smhip_ties_merge.  n == 0: a no-op, the report all zeros. ---- */
#define SMHIP_ISO_MAX_S 16384
#define SMHIP_ISO_MAX_ITER 200
typedef struct {
    int k;
    const void* finetune[SMHIP_MAX_MODELS]; /* device, in_dtype, [rows x cols] */
    const void* base[SMHIP_MAX_MODELS];     /* device, in_dtype: each finetune's own base */
    double alpha[SMHIP_MAX_MODELS];
    int in_dtype;
    const void* base_out; int base_out_dtype;
    size_t n;                               /* rows * cols */
    int rows, cols;
    double lambda;
    double tol;                             /* (0, 1] */
    int max_iter;                           /* 0..200 */
    void* workspace; size_t workspace_bytes;
} smhip_iso_desc;
typedef struct {
    int s, L, transposed;
    int iterations, converged, zero;
    double nu, N, sigma_bar;
    double e[SMHIP_ISO_MAX_ITER + 1];       /* e_0 .. e_iterations */
    char steps[SMHIP_ISO_MAX_ITER + 4];     /* 'q' / 'c' per step, NUL-terminated */
} smhip_iso_report;
size_t smhip_iso_workspace(int rows, int cols);   /* 0: a bad argument */
/* out: device, base_out_dtype, [rows x cols].  delta_out (optional): device float, merged.  report (optional): HOST. */
int smhip_iso_merge(smhip_ctx* ctx, const smhip_iso_desc* desc, void* out, float* delta_out,
                    smhip_iso_report* report, void* stream);
/* TEST ABI, as smhip_tsv_probe: "iso_gemm" alone on DEVICE fp32 matrices with element-aligned pointers and pitches.
 * form 0 (NT): c = ep(a b^T), a [M x K] pitch lda, b [N x K] pitch ldb; form 1 (NN): c = ep(a b), b [K x N].  sym (NT,
 * M == N, b^T the transpose of a's partner bit for bit - a == b, or a == b symmetric): m >= n computed and mirrored.
 * epilogue 0: acc; 1: fmaf(ca, acc, cb * e[m][n]); 2: fmaf(ca, e[m][n], acc); 3: fmaf(ca, e[m][n], cb * acc); e [M x N]
 * pitch lde.  c [M x N] pitch ldc may not overlap an input.  M, N, K >= 1. */
typedef struct {
    int form, sym, epilogue;
    int M, N, K;
    const float* a; int lda;
    const float* b; int ldb;
    const float* e; int lde;
    float ca, cb;
    float* c; int ldc;
} smhip_iso_gemm_desc;
int smhip_iso_gemm(smhip_ctx* ctx, const smhip_iso_gemm_desc* desc, void* stream);

/* ---- WIDEN merge (Yu, Yu, Yu, Huang, Li, "Extend Model Merging from Fine-Tuned to Pre-Trained Large Language Models via
 *      Weight Disentanglement", 2024): every weight matrix is disentangled into a magnitude and a direction per column,
 *      the divergences of each finetune from its base in both are RANKED within the finetune - which makes the measure
 *      scale-free: a delta a hundred times larger ranks the same - and the ranks become per-column, per-finetune weights
 *      through a softmax across the finetunes, with the above-average columns calibrated.  The reference has no such
 *      operator; this section IS its definition (what the paper's code does was recalled, not checked: PAPERS.md).
 *      One tensor of n elements is viewed as R x C, R = rows (the first dimension; a tensor of rank > 2 is
 *      [shape[0] x the rest]), C = n / R.  Finetunes i = 0..k-1 in order, 1 <= k <= 16; f_i = fp32(finetune_i),
 *      b_i = fp32(base_i), x_i = fl32(f_i - b_i).
 *        1. Column sums (matrix mode, R >= 2).  Per finetune i and column j, in fp64: P = sum_r f[r,j]^2,
 *           B = sum_r b[r,j]^2, X = sum_r f[r,j] b[r,j].  A product of two fp32 values is exact in fp64, so every addition
 *           is ONE correctly rounded fp64 addition of an exact product, in this order: the rows are cut into segments
 *           of 512, segment g = rows [512 g, min(R, 512 (g + 1))); inside a segment the row with local index rho belongs
 *           to sub-lane u = rho % 8; a sub-lane starts from +0 and adds its rows in ascending rho; the 8 sub-lanes are
 *           reduced by a binary tree, p_u = p_u + p_(u+s) for u < s, s = 4, 2, 1, the segment's value is p_0; the
 *           segments' values are added from +0 in ascending g.  The order is a function of R alone - not of the grid,
 *           the device or the number of processes - and no floating-point atomic takes part.  A NaN or Inf in
 *           finetune_i or base_i shows as a non-finite P or B and fails the call with SMHIP_ERR_NONFINITE (the message
 *           lists the finetunes); out is then unspecified.
 *        2. Divergences (matrix mode), every operation ONE rounded fp64 operation, never an fma:
 *           m_i[j] = |sqrt(P) - sqrt(B)|;  d_i[j] = 1 - c, den = sqrt(P * B), c = min(1, max(-1, X / den)); where den is
 *           0 or not finite, d = 0 if P == B, else 1.  A column the finetune did not touch has P == B == X and
 *           sqrt(P * P) == P, so c = 1 and d = +0 exactly (hence not X / (sqrt(P) * sqrt(B))).  Both are finite and >= +0:
 *           their bit patterns order as unsigned integers.
 *           Vector mode (R == 1: norm weights, any tensor whose first dimension is 1): ONE statistic, a_i[j] =
 *           (double) |x_i[j]| (the paper's rule for 1-D parameters); a non-finite a_i fails the call as above.
 *        3. Ranks.  rank_i^s[j] = #{j' : statistic s of finetune i at j' is strictly smaller than at j}: equal values
 *           share a rank, so the result depends on no sort order (DEVIATION: the paper's stable argsort breaks ties by
 *           index).  sigma = (double) rank / (double) C, one division; with S the sum of the ranks as a 64-bit integer,
 *           mu_i^s = ((double) S / (double) C) / (double) C.
 *        4. Scores, per column and statistic: sigma_max = max_i sigma_i, e_i = sm_exp(sigma_i - sigma_max) (sm_exp of
 *           csrc/sm_fusion.hpp; the argument is <= 0), Z = ((0 + e_0) + e_1) + ..., p_i = e_i / Z;
 *           score_i = calibration where sigma_i > ratio * mu_i^s (one multiplication, a strict comparison), else p_i.
 *        5. Weights.  Matrix mode: h = 0.5 * (score^m + score^d), w_i[j] = fp32(alpha_i * h); vector mode:
 *           w_i[j] = fp32(alpha_i * score).  alpha_i in fp64, of any sign; their sum may be 0: nothing divides by it.
 *        6. Combine, for element [r, j]: M = ((0 + fl32(w_0[j] * x_0)) + fl32(w_1[j] * x_1)) + ... in fp32, product and
 *           sum rounded separately; out = round_to(base_out_dtype, fp32(base_out) + fl32(fp32(lambda) * M));
 *           delta_out (optional) = fl32(fp32(lambda) * M): steps 6 and 7 of smhip_dare_merge, so a call whose weights
 *           all equal fp32(alpha_i) is dare_linear at density 1 without normalize, bit for bit.
 *      Limits: C <= 65536 (SMHIP_ERR_ARG beyond); n > 0 needs rows >= 1 that divides n; ratio finite, calibration
 *      finite and >= 0, lambda finite.  Aliasing, alignment, n == 0 (a no-op, the report all zeros), dtypes and the size
 *      limit: the rules of smhip_ties_merge.
 *      Passes: "widen_colstats" (matrix mode only: the finetune and its base once each, 2 k tensor passes - a shared
 *      base is re-read per finetune), "widen_colfold", "widen_rank" (all pairs, O(C^2) integer comparisons per finetune
 *      and statistic), "widen_coef", "widen_combine" (k + 2 tensor passes with a shared base): 3 k + 2.  Counters are
 *      integers; the stream is synchronised once, at the end. ---- */
typedef struct {
    int k;
    const void* finetune[SMHIP_MAX_MODELS]; /* device, in_dtype, [n] */
    const void* base[SMHIP_MAX_MODELS];     /* device, in_dtype: each finetune's own base */
    double alpha[SMHIP_MAX_MODELS];
    int in_dtype;                           /* SMHIP_BF16 / F16 / F32, finetunes and their bases */
    const void* base_out; int base_out_dtype;
    size_t n;
    size_t rows;                            /* R; C = n / rows */
    double ratio;                           /* the cut: a column is calibrated where sigma > ratio * mu */
    double calibration;                     /* >= 0: the score of a calibrated column */
    double lambda;
} smhip_widen_desc;
typedef struct {
    uint64_t rows, cols;                    /* R, C */
    int vector_mode;                        /* 1: R == 1, the one statistic a at index 0 */
    double mu[SMHIP_MAX_MODELS][2];         /* [i][s]: s = 0 magnitude (or a), 1 direction */
    uint64_t calibrated[SMHIP_MAX_MODELS][2];   /* columns with sigma > ratio * mu */
} smhip_widen_report;
/* out: device, base_out_dtype, [n].  delta_out (optional): device float [n], lambda * M.  For the tests (optional,
 * device, element-aligned): stat_out double [k][2][C] (m, d; vector mode a, then zeros), rank_out uint32 [k][2][C],
 * weight_out float [k][C].  report (optional): HOST. */
int smhip_widen_merge(smhip_ctx* ctx, const smhip_widen_desc* desc, void* out, float* delta_out, double* stat_out,
                      uint32_t* rank_out, float* weight_out, smhip_widen_report* report, void* stream);

/* ---- CABS merge (Yang et al., "CABS: Conflict-Aware and Balanced Sparsification for Enhancing Model Merging", ICML 2025,
 *      as recalled: PAPERS.md): n:m sparsification of every task vector - each group of M consecutive weights of a row
 *      keeps its N largest magnitudes, so the budget is spent evenly over the tensor (BS) - applied to the finetunes one
 *      after another, each allowed only the positions that no earlier one kept (CA), so the kept sets are disjoint; the
 *      sparse task vectors are then added with their weights.  The reference has no such operator; this section IS its
 *      definition.  The tensor of n elements is seen as R = rows rows of C = n / rows elements (the caller passes the
 *      length of the last dimension; a 0-D or 1-D tensor is one row: DELLA's view), finetunes i = 0..k-1 IN THE ORDER
 *      GIVEN (1 <= k <= 16); n_keep = N, group = M, conflict_aware are integers:
 *        1. d_i = fp32(finetune_i) - fp32(base_i).  A NaN or Inf in any d_i fails the call with SMHIP_ERR_NONFINITE
 *           (the message lists the finetunes), detected as smhip_dare_merge detects it; out is then unspecified.
 *        2. Groups.  Row r is cut into G = ceil(C / M) groups; group g covers the columns [g M, min(C, (g + 1) M)) and has
 *           m' of them.  Its quota is q = ceil(N m' / M) in integers, (N * m' + M - 1) / M: N for a full group, at least
 *           1 for a tail.
 *        3. Selection, for i = 0, 1, ..., k - 1 in this order.  The CANDIDATES of finetune i in a group are its elements
 *           with d_i != 0 and, when conflict_aware == 1, kept by no j < i.  With c candidates: c <= q keeps them all (the
 *           group is SHORT for i if c < q); otherwise tau is the q-th largest |d_i| among the candidates, exact on the
 *           31 magnitude bits as unsigned integers, and a candidate is KEPT iff |d_i| >= tau.  TIE RULE: a candidate that
 *           ties with tau is kept (the rule of smhip_ties_merge), so the result depends on no traversal order and a
 *           group may keep more than q; the excess is its SURPLUS.
 *        4. tv_i = fl32(d_i * fp32(alpha_i)) where kept, +0 elsewhere; M = ((0 + tv_0) + tv_1) + ... in fp32, in order.
 *           There is NO normalisation: under CA at most one term of an element is non-zero, and a division by the sum
 *           of the weights would shrink it.  The alphas may have any sign and any sum.
 *        5. out = round_to(base_out_dtype, fp32(base_out) + fl32(fp32(lambda) * M)), delta_out = fl32(lambda * M):
 *           step 7 of smhip_ties_merge.
 *        6. mask_out (optional): device uint16 [n], bit i set iff finetune i kept the element.
 *        7. The report, all integers: groups = R G; kept[i]; short_groups[i]; surplus[i], the elements kept beyond the
 *           quota summed over the groups; covered, the elements kept by at least one finetune; overlap, those kept by at
 *           least two (0 whenever conflict_aware == 1).
 *      Every step is an integer function, an exact order statistic or one correctly rounded fp32 operation: the result is
 *      defined bit for bit.  conflict_aware == 0 with N == M keeps every non-zero entry: smhip_dare_merge (sign_election 0,
 *      normalize 0) at density 1.  SMHIP_ERR_ARG: group not a power of two in 4..512, n_keep outside 1..group,
 *      conflict_aware not 0 or 1, k outside 1..16, rows that do not divide n, lambda or an alpha not finite, a mask_out
 *      that is misaligned or overlaps another tensor.  Aliasing, alignment, n == 0 (a no-op, the report all zeros),
 *      dtypes and the size limit: the rules of smhip_ties_merge.
 *      ONE kernel, one pass over the inputs (k + 2 tensor passes with a shared base): a lane holds the k deltas of 8
 *      columns of a row in registers, the max(M, 8) / 8 lanes of a group select together - in the lane for M <= 8, else by a
 *      digit descent over the 31 key bits through a 16-bin histogram in LDS, one barrier per digit, 8 per finetune.  No
 *      histogram launch, no second read.  C % 8 == 0 with 16-byte aligned pointers takes 16-byte accesses, anything else
 *      goes element by element and is as exact.  Counters are integers (LDS, then one global atomic per counter and
 *      work-group), no floating-point atomics; the call synchronises the stream once, at its end.  Profile name:
 *      "cabs_merge" (k <= 4) or "cabs_merge_any". ---- */
typedef struct {
    int k;
    const void* finetune[SMHIP_MAX_MODELS]; /* device, in_dtype, [n] */
    const void* base[SMHIP_MAX_MODELS];     /* device, in_dtype: each finetune's own base */
    double alpha[SMHIP_MAX_MODELS];
    int in_dtype;                           /* SMHIP_BF16 / F16 / F32, finetunes and their bases */
    const void* base_out; int base_out_dtype;
    size_t n;
    size_t rows;                            /* R; C = n / rows */
    int n_keep, group;                      /* N : M */
    int conflict_aware;                     /* 1: a finetune may keep only what no earlier one kept */
    double lambda;
} smhip_cabs_desc;
typedef struct {
    uint64_t groups;                        /* R * ceil(C / M) */
    uint64_t kept[SMHIP_MAX_MODELS];
    uint64_t short_groups[SMHIP_MAX_MODELS];/* groups with fewer candidates than their quota */
    uint64_t surplus[SMHIP_MAX_MODELS];     /* elements kept beyond the quota (ties with tau) */
    uint64_t covered, overlap;              /* elements kept by >= 1 and by >= 2 finetunes */
} smhip_cabs_report;
/* out: device, base_out_dtype, [n].  delta_out (optional): device float [n], lambda * M.  mask_out (optional): device
 * uint16 [n].  report (optional): HOST. */
int smhip_cabs_merge(smhip_ctx* ctx, const smhip_cabs_desc* desc, void* out, float* delta_out, uint16_t* mask_out,
                     smhip_cabs_report* report, void* stream);

/* ---- Delta pack: a finetune stored as one or two bits per weight and a scale, on top of its base.  bits == 1 keeps the
 *      sign of every delta and one scale (BitDelta, Liu et al. 2024); bits == 2 keeps a mask of the `density` largest
 *      magnitudes and their signs, a sparse ternary delta (ComPEFT, Yadav et al. 2023; both as recalled: PAPERS.md).  It
 *      is no merge operator: smhip_dpack_apply rebuilds a finetune tensor that every operator then takes.  The reference
 *      has no such format; this section IS its definition.  The tensor is seen as R = rows rows of C = cols elements
 *      (the caller passes shape[0] and the product of the rest; a 0-D or 1-D tensor is one row), n = R C.
 *      PACK, smhip_dpack_pack:
 *        1. d_e = fl32(fp32(finetune_e) - fp32(base_e)).  A NaN or Inf in d fails the call with SMHIP_ERR_NONFINITE; the
 *           outputs are then unspecified.
 *        2. bits == 2, density in (0, 1]: k_keep and tau are those of smhip_ties_merge (step 2) with this one finetune at
 *           this density, found by its selection kernels; an element is KEPT iff |d| >= tau and d != 0, every tie is kept.
 *           bits == 1 (density must be 1): nothing is selected, EVERY element is kept, a zero delta included.
 *        3. Planes, uint8 [R][ceil(C / 8)]: bit c % 8 of byte c / 8 of row r is element (r, c).  mask (bits == 2 only): set
 *           iff kept.  sign: set iff kept and d < 0.  The padding bits of a row's last byte are 0.
 *        4. Sums per row, fp64, in the row-wise order of step 2 of smhip_geo_merge: octet o of the row (columns 8 o ..
 *           8 o + 7) goes to lane o % 256, a lane adds its elements in ascending order from +0, the 256 lanes are added by
 *           the binary tree v[t] += v[t + s], s = 128, 64, ..., 1.  (double) of an fp32 value and the product of two are
 *           exact.  A_r = sum over kept of |d|, Q_r = sum over kept of d^2, Z_r = sum over the others of d^2; c_r the
 *           kept count and nz_r the count of d != 0, integers.  The totals A, Q, Z, c, nz are the rows' values added in
 *           ascending row order from +0.
 *        5. Scale.  scale_mode ROW: s_r = fp32(A_r / (double) c_r), +0 when c_r == 0; scale is float [R].  TENSOR:
 *           s = fp32(A / (double) c) of the totals, +0 when c == 0; scale is float [1].  The mean of the kept magnitudes is
 *           the scale that minimises sum over kept of (d - s sgn d)^2.
 *        6. Residual, fp64, one IEEE operation at a time, no fused multiply-add:
 *             e(A, Q, c, s) = max((Q - 2 (s A)) + c (s s), 0)
 *           ROW: resid_sq = sum_r (Z_r + e(A_r, Q_r, c_r, s_r)) and delta_sq = sum_r (Q_r + Z_r), rows added in ascending
 *           order from +0.  TENSOR: the same with the totals as the one row: resid_sq = Z + e(A, Q, c, s), delta_sq = Q + Z.
 *        7. The report: rows, cols, bits, k_keep (n for bits == 1), threshold (tau; +inf when k_keep == 0, 0 for
 *           bits == 1), kept = c, nonzero = nz, delta_sq, resid_sq.
 *      APPLY, smhip_dpack_apply: a kept element gives round_to(dtype, fp32(base_e) + (sign ? -s_r : s_r)), one fp32 addition
 *      and one round-to-nearest-even cast; an element that is not kept gives base_e bit for bit, a -0 included.  mask ==
 *      NULL (a 1-bit pack): every element is kept.  Padding bits are not read as elements.
 *      Every step is an exact order statistic, an integer function or one correctly rounded operation, there is no
 *      floating-point atomic, and nothing depends on the grid or the device: both results are defined bit for bit.
 *      n == 0: no plane has a byte, the scales are +0, the report is zero but for the threshold, apply is a no-op.
 *      SMHIP_ERR_ARG: bits not 1 or 2, a density outside (0, 1], bits == 1 with density != 1, a bad scale_mode or dtype, a
 *      null or misaligned pointer (mask is needed iff bits == 2), an output that overlaps an input, a tensor too large.
 *      C % 8 == 0 with 16-byte aligned tensors moves them in 16-byte accesses; anything else goes element by element and is
 *      as exact.  Pack synchronises the stream once, at its end; apply does not.  Profile names: "ties_hist",
 *      "ties_select" (bits == 2), "dpack_pack", "geo_gram_fold", "dpack_scale"; "dpack_apply". ---- */
enum { SMHIP_DPACK_ROW = 0, SMHIP_DPACK_TENSOR = 1 };
typedef struct {
    const void* finetune; const void* base; /* device, dtype, [rows][cols] */
    int dtype;                              /* SMHIP_BF16 / F16 / F32 */
    size_t rows, cols;
    int bits;                               /* 1 or 2 */
    double density;                         /* bits == 2: in (0, 1]; bits == 1: 1 */
    int scale_mode;                         /* SMHIP_DPACK_ROW / SMHIP_DPACK_TENSOR */
} smhip_dpack_desc;
typedef struct {
    uint64_t rows, cols;
    int bits;
    uint64_t k_keep;
    float threshold;
    uint64_t kept, nonzero;
    double delta_sq, resid_sq;
} smhip_dpack_report;
/* sign, mask (bits == 2, else NULL): device uint8 [rows][ceil(cols / 8)].  scale: device float [rows] or [1].
 * report (optional): HOST. */
int smhip_dpack_pack(smhip_ctx* ctx, const smhip_dpack_desc* desc, uint8_t* sign, uint8_t* mask, float* scale,
                     smhip_dpack_report* report, void* stream);
typedef struct {
    const void* base; int dtype;            /* device, [rows][cols] */
    size_t rows, cols;
    const uint8_t* sign; const uint8_t* mask; /* device; mask NULL: a 1-bit pack */
    const float* scale; int scale_mode;
} smhip_dpack_apply_desc;
/* out: device, dtype, [rows][cols]; it must not overlap an input */
int smhip_dpack_apply(smhip_ctx* ctx, const smhip_dpack_apply_desc* desc, void* out, void* stream);

/* ---- EMR-Merging (Huang et al., "EMR-Merging: Tuning-Free High-Performance Model Merging", NeurIPS 2024; as recalled:
 *      PAPERS.md): ONE unified task vector is ELECTED from the finetunes' deltas - per element the sign of their sum and
 *      the largest magnitude among the entries of that sign - and every task gets a 1-bit MASK (where its own delta
 *      agrees in sign with the unified one) and ONE RESCALER on top of it, which recover a model for that task.  The
 *      reference has no such operator; this section IS its definition.  Three functions: the unified model
 *      (smhip_emr_merge), a task's modulator from (finetune, base, unified model) (smhip_emr_mask), and the task's
 *      tensor from (base, unified model, mask, rescaler) (smhip_emr_apply).
 *      MERGE, smhip_emr_merge.  One tensor of n elements (any shape, flat), finetunes i = 0..k-1 in order (1 <= k <= 16):
 *        1. d_i = fl32(fp32(finetune_i) - fp32(base_i)), each entry against its own base.  A NaN or Inf in any d_i fails
 *           the call with SMHIP_ERR_NONFINITE (the message lists the finetunes); out is then unspecified.
 *        2. S = ((+0 + d_0) + d_1) + ... in fp32, in order.  A NaN or Inf in S fails the call the same way.
 *           pos = S >= 0: the rule of smhip_ties_merge, an exact zero sum elects plus (the authors' code, as recalled,
 *           takes sum > 0; the deviation is stated in PAPERS.md).
 *        3. eps = the largest |d_i| over the entries with d_i > 0 (pos) or d_i < 0 (not pos), +0 when there is none;
 *           w = the smallest such i that attains it.
 *        4. tau = pos ? eps : -eps, and +0 when eps == 0: tau is +0 or exactly one of the d_i.
 *        5. out = round_to(base_out_dtype, fp32(base_out) + fl32(fp32(lambda) * tau)), delta_out = fl32(lambda * tau):
 *           step 7 of smhip_ties_merge.  The method has no weights: alpha is not read.
 *      Nothing rounds between 1 and 4 but the subtraction and the sum: the result is defined bit for bit.  k == 1 is
 *      smhip_dare_merge (sign_election 0) at density 1 with alpha 1 and the same lambda.  The report: n; elected_pos,
 *      elected_neg (eps > 0 and pos / not pos) and zero (eps == 0), which sum to n; contested (elements with non-zero
 *      entries of both signs); winner[i] (elements with w == i; with zero they sum to n); agree[i] (elements where
 *      d_i != 0 has the sign of tau).  ONE kernel, one pass over the inputs (k + 2 tensor passes): the k deltas of an
 *      element stay in registers between the sum and the maximum, no finetune is read twice.  Counters are integers
 *      (LDS, then one global atomic per counter and work-group), no floating-point atomics; the call synchronises the
 *      stream once, at its end.  Aliasing, alignment, n == 0, dtypes and the size limit: the rules of smhip_ties_merge.
 *      SMHIP_ERR_ARG: k outside 1..16, lambda not finite, out overlapping an input, a bad dtype, a null descriptor.
 *      MASK, smhip_emr_mask.  The tensor is seen as R = rows rows of C = cols elements as smhip_dpack_pack sees it:
 *        1. d = fl32(fp32(finetune) - fp32(base)), u = fl32(fp32(unified) - fp32(base)).  A NaN or Inf in d or u fails
 *           the call with SMHIP_ERR_NONFINITE (the message says which); the outputs are then unspecified.
 *        2. m = (d > 0 and u > 0) or (d < 0 and u < 0): the signs are compared, no product is formed (it underflows).
 *           mask, uint8 [R][ceil(C / 8)]: bit c % 8 of byte c / 8 of row r is m of element (r, c); padding bits are 0.
 *        3. Seven sums per row, fp64, in exactly the order of step 4 of smhip_dpack_pack (lane o % 256, ascending, the
 *           binary tree, rows added in ascending order from +0); the product of two fp32 values is exact in fp64:
 *           A = sum |d|, B = sum over m of |u|, D2 = sum d d, X = sum over m of d u, U2 = sum over m of u u, and the
 *           integer counts c = sum m, nz = sum [d != 0].
 *        4. lambda = fp32(A / B), +0 when B == 0: the paper's rescaler sum |tau_t| / sum |M_t . tau_uni| of this tensor
 *           (a caller that wants one rescaler for a whole model adds A and B over its tensors).  scale: float [1].
 *        5. resid_sq = max((D2 - 2 (lambda X)) + (lambda lambda) U2, 0), one IEEE fp64 operation at a time, no fused
 *           multiply-add: sum (d - lambda m u)^2.  delta_sq = D2.
 *      n == 0: the plane has no byte, lambda is +0, the report is zero.  SMHIP_ERR_ARG: a bad dtype, a null or
 *      misaligned pointer, an output that overlaps an input, a tensor too large.  One synchronisation, at the end.
 *      APPLY, smhip_emr_apply.  Per element: mask bit clear: base bit for bit, a -0 included.  Set: u = fl32(fp32(unified)
 *      - fp32(base)), t = fl32(lambda * u), out = round_to(dtype, fp32(base) + t), one rounding each; lambda = scale[0].
 *      Padding bits are not read as elements.  It does not synchronise.  C % 8 == 0 with 16-byte aligned tensors moves
 *      them in 16-byte accesses; anything else goes element by element and is as exact.
 *      Profile names: "emr_merge"; "emr_mask", "geo_gram_fold"; "emr_apply". ---- */
typedef struct {
    int k;
    const void* finetune[SMHIP_MAX_MODELS]; /* device, in_dtype, [n] */
    const void* base[SMHIP_MAX_MODELS];     /* device, in_dtype: each finetune's own base */
    double alpha[SMHIP_MAX_MODELS];         /* not read (the layout of the other merge descriptors) */
    int in_dtype;                           /* SMHIP_BF16 / F16 / F32, finetunes and their bases */
    const void* base_out; int base_out_dtype;
    size_t n;
    double lambda;
} smhip_emr_desc;
typedef struct {
    uint64_t n;
    uint64_t elected_pos, elected_neg, zero, contested;
    uint64_t winner[SMHIP_MAX_MODELS];
    uint64_t agree[SMHIP_MAX_MODELS];
} smhip_emr_report;
/* out: device, base_out_dtype, [n].  delta_out (optional): device float [n], fl32(lambda * tau).  report (optional): HOST. */
int smhip_emr_merge(smhip_ctx* ctx, const smhip_emr_desc* desc, void* out, float* delta_out, smhip_emr_report* report,
                    void* stream);
typedef struct {
    const void* finetune; const void* base; const void* unified; /* device, dtype, [rows][cols] */
    int dtype;                              /* SMHIP_BF16 / F16 / F32 */
    size_t rows, cols;
} smhip_emr_mask_desc;
typedef struct {
    uint64_t rows, cols;
    double A, B, D2, X, U2;
    uint64_t c, nonzero;
    float lambda;
    double delta_sq, resid_sq;
} smhip_emr_mask_report;
/* mask: device uint8 [rows][ceil(cols / 8)].  scale: device float [1].  report (optional): HOST. */
int smhip_emr_mask(smhip_ctx* ctx, const smhip_emr_mask_desc* desc, uint8_t* mask, float* scale,
                   smhip_emr_mask_report* report, void* stream);
typedef struct {
    const void* base; const void* unified; int dtype; /* device, [rows][cols] */
    size_t rows, cols;
    const uint8_t* mask;                    /* device uint8 [rows][ceil(cols / 8)] */
    const float* scale;                     /* device float [1] */
} smhip_emr_apply_desc;
/* out: device, dtype, [rows][cols]; it must not overlap an input */
int smhip_emr_apply(smhip_ctx* ctx, const smhip_emr_apply_desc* desc, void* out, void* stream);
/* ---- MERGE AND MASKS, smhip_emr_merge_masks: the unified tensor and every entry's modulator from ONE pass.  It is the
 *      composition of the two functions above, and that composition is its whole specification.  The tensor of
 *      desc->n = rows * cols elements is seen as R = rows rows of C = cols elements (a 0-D or 1-D tensor: one row), k
 *      entries, 1 <= k <= 16:
 *        1. out, delta_out and report are those of smhip_emr_merge(desc), bit for bit.
 *        2. g = the fp32 value of the element of out AS STORED, after its one rounding into base_out_dtype.  Per entry i
 *           and element: d = fl32(fp32(finetune_i) - fp32(base_i)), u = fl32(g - fp32(base_i)), each entry against its
 *           own base.
 *        3. m = (d > 0 and u > 0) or (d < 0 and u < 0); masks[i], uint8 [R][ceil(C / 8)]: bit c % 8 of byte c / 8 of row
 *           r is m of element (r, c) of entry i, padding bits 0.
 *        4. Per entry and row the seven values A, B, D2, X, U2, c, nz of step 3 of smhip_emr_mask in exactly its order:
 *           lane t of 256 takes octets t, t + 256, ... of the row in ascending order, each value one rounded fp64
 *           addition; then the fixed binary tree v[t] = v[t] + v[t + s], s = 128 .. 1; then the rows added in index
 *           order from 0.0.
 *        5. scales[i][0] = fp32(A_i / B_i), +0 when B_i == 0; resid_sq_i as step 5 of smhip_emr_mask forms it.
 *      So (masks[i], scales[i], mask_reports[i]) equals smhip_emr_mask(finetune_i, base_i, out) for every i, bit for
 *      bit (with in_dtype != base_out_dtype: of the three tensors converted to fp32, which changes no value).
 *      SMHIP_ERR_NONFINITE, in this order of precedence: a NaN or Inf in a d_i (the message names the lowest such
 *      finetune), in the sum of the deltas, in a u (the message names the lowest such entry); the outputs are then
 *      unspecified.  n == 0: the planes have no byte, every scale is +0, the reports are zero.  SMHIP_ERR_ARG, before
 *      any launch: what smhip_emr_merge rejects; rows * cols != n; cols >= 2^31; null masks, scales or one of their
 *      first k entries; a plane or a scale that is misaligned or overlaps another tensor of the call.
 *      Two launches: "emr_merge_mask" (a work-group of 256 per row; k <= 4: one sweep, k + 2 tensor passes plus k / 8
 *      of a byte per element of planes; k > 4: the row is swept again once per group of four entries, which reads the
 *      finetunes twice, the bases once per group (own bases: twice) and out once per group) and "emr_fold" (the ordered
 *      fold of the rows' 7k partials, staged through LDS).  No floating-point atomics; one synchronisation, at the
 *      end, which fetches the counters, the flags and the 7k totals at once. ---- */
/* out, delta_out, report: as smhip_emr_merge.  masks: HOST array of k device pointers, uint8 [rows][ceil(cols / 8)] each.
 * scales: HOST array of k device pointers, float [1] each.  mask_reports (optional): HOST array of k reports. */
int smhip_emr_merge_masks(smhip_ctx* ctx, const smhip_emr_desc* desc, size_t rows, size_t cols, void* out, float* delta_out,
                          uint8_t* const* masks, float* const* scales, smhip_emr_report* report,
                          smhip_emr_mask_report* mask_reports, void* stream);

/* ---- correlate_pairs (reference shard/tensor/functions.py:304-314, the legacy fourier.py operator's
 *      pairing matrix): matrix[i][j] = mean over the trailing positions of
 *      cosine_similarity(t_i, t_j, dim=0).nan_to_num(0); zero diagonal.  tensors: k (2..8) device
 *      tensors of `dtype`, viewed as [rows = shape[0]] x [cols = the rest] (1-D: cols = 1).
 *      matrix_out: HOST float[k*k].  (The legacy operator's task_add_models post-pass,
 *      fourier.py:191-196, is smhip_task_arithmetic_fft2(result, delta, t = 1, agreement = 0).) ---- */
int smhip_correlate_pairs(smhip_ctx* ctx, int k, const void* const* tensors, int dtype, size_t rows, size_t cols,
                          float* matrix_out, void* stream);

/* ---- torch.norm(x - base) as ATen's CPU kernel returns it for a contiguous fp32 tensor (the reference's
 *      device="cpu" norms: shard/tensor/functions.py:36,40,85, shard/merge/fast_fourier.py:152,209-210):
 *      acc = fma(x, x, acc) - one rounding per element - serially in 8 fp32 lanes, lanes added in order, the n % 8 tail,
 *      sqrt - reproduced bit for bit by a parallel algorithm (csrc/sm_aten_norm.hpp).  x, base (may be
 *      NULL): device, `dtype`, n elements, 16-byte aligned.  norm_out: HOST float.  This is what
 *      smhip_layer_desc::norm_mode = 1 uses for every spatial norm. -------------------------------- */
int smhip_reference_cpu_norm(smhip_ctx* ctx, const void* x, const void* base, int dtype, size_t n, float* norm_out,
                             void* stream);

/* ---- test hooks: "cand_cap" clamps the capacity of the selection passes' candidate
 *      lists (0 = default) so that the overflow fallback can be exercised;
 *      "sel_chunks" sets the steps per thread of the level-2 selection pass,
 *      "force_split" = p splits the column length of smhip_merge_layer into p row blocks (the path of
 *      lengths without a plan, smhip_shape_supported) although it has one, 0 = off;
 *      "force_bluestein" = 1 sends every row transform through the chirp-z row passes (the path of ROW lengths
 *      without a plan);
 *      "pair1d" = 0 sends 1-D tensors through the multi-kernel pipeline instead of the one-launch pair merge;
 *      "spec_cull" = 0 keeps the SLERP blend and the cull's selection pass apart (no speculation on the
 *      threshold's level-1 bin); "spec_min_bins" = the smallest spectrum (bins) that speculates (default 2^20);
 *      "dftp_pairs" = 0 runs the generic p-point DFT kernel also for p <= 126;
 *      "sel_wgs_per_cu" the resident work-groups per CU its grid is sized for (0 = default 5), and
 *      "sel_flush_always" flushes its staged candidates after every round (the
 *      mid-stream flush that only very large tensors reach otherwise);
 *      "noise_seed" = s offsets the seed of the rounding-noise model that a spectral intermediate's culled bins
 *      receive (another realisation of the same statistics; default 0);
 *      "spectral_intermediates" = 0 makes a K >= 3 tournament materialise every intermediate
 *      (inverse transform to fp32, forward again) as round 1 of this library did, instead of
 *      keeping it in the spectral domain (default 1);
 *      "della_slab_rows" = r makes smhip_della_merge rank and merge r rows at a time (0, the default: as many whole
 *      rows as hold at most 2^26 elements per finetune); the result does not depend on it;
 *      "emr_fused_geo_fold" = 1 makes smhip_emr_merge_masks fold its rows' partials with "geo_gram_fold" instead of
 *      "emr_fold" (default 0; the same bits, for A/B timing). ------- */
int smhip_debug_option(smhip_ctx* ctx, const char* key, long value);
/* test hook, read side: "spec_hit" = 1 if the last speculative blend's guess was confirmed, 0 if it was voided;
 * "spec_checked" / "spec_hits": how many speculations this context has checked / confirmed since it was created;
 * "aten_fast" / "aten_group" / "aten_slow": chunks the last smhip_reference_cpu_norm composed from their summaries /
 * crossed with the group summaries / walked cooperatively
 * ("aten_serial" = 1 as an option selects the old serial single-work-group chain instead);
 * "eig_host_us": microseconds this context has spent on the host in the Jacobi eigensolver of smhip_lora_extract and
 * smhip_tsv_merge since it was created */
int smhip_debug_query(smhip_ctx* ctx, const char* key, long* value);

/* ---- profiling: per-kernel device time measured with HIP events on the
 *      caller's stream (bench.py's roofline leg) ---------------------------- */
int smhip_profile_enable(smhip_ctx* ctx, int on);
int smhip_profile_reset(smhip_ctx* ctx);
int smhip_profile_count(smhip_ctx* ctx);
/* i-th kernel: name, number of launches, total milliseconds */
int smhip_profile_get(smhip_ctx* ctx, int i, const char** name, uint64_t* launches, double* total_ms);

#ifdef __cplusplus
}
#endif
#endif /* SHARDMERGE_HIP_H */
