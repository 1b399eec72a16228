// sm_capi.inc - the extern "C" surface of include/shardmerge_hip.h, written once
// and included by the HIP build (smhip_hip.hip) and by the CPU work-group
// emulator (tests/emul/smhip_emul.cpp) after they define SM_BACKEND.
//
// struct smhip_ctx wraps Pipeline<SM_BACKEND>; the delta operators are its member `delta` (sm_delta_host.hpp).

struct smhip_ctx {
    smhip::Pipeline<SM_BACKEND> pipe;
    explicit smhip_ctx(int device) : pipe(device) {}
};

#define SM_GUARD(ctx)                      \
    if (!(ctx)) return SMHIP_ERR_ARG;      \
    (ctx)->pipe.err.clear();
#define SM_FINISH(ctx, rc)                                                        \
    do {                                                                          \
        int rc__ = (rc);                                                          \
        if (rc__ == SMHIP_OK && !(ctx)->pipe.be.ok()) {                           \
            (ctx)->pipe.err = (ctx)->pipe.be.error();                             \
            rc__ = SMHIP_ERR_HIP;                                                 \
        }                                                                         \
        return rc__;                                                              \
    } while (0)

// The argument checks that smhip_ties_merge, smhip_dare_merge and smhip_breadcrumbs_merge share: their descriptors have
// the same leading fields (k .. normalize), hence the template.  `op` names the entry point in the messages.
// smhip_geo_merge shares all of it but the scalars (`scalars`: the operator's own checks, after k and the dtypes) and,
// in weight space, the bases (`need_base` = false: they are not read and may be NULL); smhip_sce_merge, smhip_della_merge and
// smhip_consensus_merge all but the scalars; smhip_fusion_merge too (k == 1).
template <class Desc, class Scalars>
static int delta_tensor_check(smhip_ctx* ctx, const char* op, const Desc* d, const void* out, const float* delta_out,
                              bool need_base, Scalars scalars) {
    auto bad = [&](const char* what) { return ctx->pipe.fail(SMHIP_ERR_ARG, std::string(op) + ": " + what); };
    if (!d) return bad("null descriptor");
    if (d->k < 1 || d->k > SMHIP_MAX_MODELS) return bad("k out of range (1..16)");
    if (d->in_dtype < SMHIP_BF16 || d->in_dtype > SMHIP_F32 || d->base_out_dtype < SMHIP_BF16 || d->base_out_dtype > SMHIP_F32)
        return bad("bad dtype");
    if (const char* what = scalars()) return bad(what);
    for (int i = 0; i < d->k; ++i)
        if (!std::isfinite(d->alpha[i])) return bad("an alpha is not finite");
    if (d->n == 0) return SMHIP_OK;
    if (!out || (need_base && !d->base_out)) return bad("null out or base_out");
    const size_t ies = d->in_dtype == SMHIP_F32 ? 4 : 2, oes = d->base_out_dtype == SMHIP_F32 ? 4 : 2;
    if ((uintptr_t)out % oes || (uintptr_t)d->base_out % oes || (uintptr_t)delta_out % 4)
        return bad("a pointer is not aligned to its element size");
    auto overlaps = [&](const void* o, size_t obytes, const void* p, size_t bytes) {
        return o && (uintptr_t)p < (uintptr_t)o + obytes && (uintptr_t)o < (uintptr_t)p + bytes;
    };
    auto hits_output = [&](const void* p, size_t bytes) {
        return overlaps(out, d->n * oes, p, bytes) || overlaps(delta_out, d->n * 4, p, bytes);
    };
    bool hit = (need_base && hits_output(d->base_out, d->n * oes)) || overlaps(out, d->n * oes, delta_out, d->n * 4);
    for (int i = 0; i < d->k; ++i) {
        if (!d->finetune[i] || (need_base && !d->base[i])) return bad("null model tensor");
        if ((uintptr_t)d->finetune[i] % ies || (need_base && (uintptr_t)d->base[i] % ies))
            return bad("a pointer is not aligned to its element size");
        hit = hit || hits_output(d->finetune[i], d->n * ies) || (need_base && hits_output(d->base[i], d->n * ies));
    }
    if (hit) return bad("out overlaps an input");
    if ((d->n + 7) / 8 / 256 > (size_t)1 << 30) return bad("tensor too large");
    return SMHIP_OK;
}
template <class Desc>
static int delta_merge_check(smhip_ctx* ctx, const char* op, const Desc* d, const void* out, const float* delta_out) {
    return delta_tensor_check(ctx, op, d, out, delta_out, true, [&]() -> const char* {
        if (!(d->density > 0.0 && d->density <= 1.0)) return "density must be in (0, 1]";
        if (!std::isfinite(d->lambda)) return "lambda is not finite";
        return nullptr;
    });
}

extern "C" {

const char* smhip_version(void) { return SM_VERSION_STRING; }

int smhip_create(int device, smhip_ctx** out) {
    if (!out) return SMHIP_ERR_ARG;
    *out = nullptr;
    smhip_ctx* c = new smhip_ctx(device);
    if (!c->pipe.be.ok()) {
        fprintf(stderr, "smhip_create: %s\n", c->pipe.be.error().c_str());
        delete c;
        return SMHIP_ERR_HIP;
    }
    *out = c;
    return SMHIP_OK;
}

void smhip_destroy(smhip_ctx* ctx) { delete ctx; }

const char* smhip_last_error(smhip_ctx* ctx) { return ctx ? ctx->pipe.err.c_str() : "null context"; }

int smhip_reserve(smhip_ctx* ctx, int rows, int cols) {
    SM_GUARD(ctx);
    if (rows < 1 || cols < 1) return ctx->pipe.fail(SMHIP_ERR_ARG, "bad shape");
    SM_FINISH(ctx, ctx->pipe.reserve(rows, cols));
}

size_t smhip_workspace_bytes(smhip_ctx* ctx) { return ctx ? ctx->pipe.workspace_bytes() : 0; }

int smhip_length_supported(int n) {
    int T;
    std::vector<int> rad;
    return smhip::plan_shape(n, T, rad) ? SMHIP_OK : SMHIP_ERR_SHAPE;
}

int smhip_shape_supported(int rows, int cols) {
    return smhip::shape_support(rows, cols) ? SMHIP_OK : SMHIP_ERR_SHAPE;
}

int smhip_fft_transform(smhip_ctx* ctx, const float* x, int rows, int cols, float* spectrum, void* stream) {
    SM_GUARD(ctx);
    if (!x || !spectrum || rows < 1 || cols < 1) return ctx->pipe.fail(SMHIP_ERR_ARG, "bad argument");
    ctx->pipe.stream = stream;
    SM_FINISH(ctx, ctx->pipe.fft_transform(x, rows, cols, spectrum));
}

int smhip_ifft_transform(smhip_ctx* ctx, const float* spectrum, int rows, int cols, float* real_out, void* stream) {
    SM_GUARD(ctx);
    if (!real_out || !spectrum || rows < 1 || cols < 1) return ctx->pipe.fail(SMHIP_ERR_ARG, "bad argument");
    ctx->pipe.stream = stream;
    SM_FINISH(ctx, ctx->pipe.ifft_transform(spectrum, rows, cols, real_out));
}

int smhip_interpolate_fft_components(smhip_ctx* ctx, const float* f0, const float* f1, int rows, int cols, double t,
                                     double t_sum, double cutoff_pct, double cull_pct, int interp_imag,
                                     float* out_spectrum, smhip_blend_info* info, void* stream) {
    SM_GUARD(ctx);
    if (!f0 || !f1 || !out_spectrum || rows < 1 || cols < 1) return ctx->pipe.fail(SMHIP_ERR_ARG, "bad argument");
    ctx->pipe.stream = stream;
    SM_FINISH(ctx, ctx->pipe.blend_full(f0, f1, rows, cols, smhip::BLEND_SLERP, t, t_sum, cutoff_pct, cull_pct, 1,
                                        interp_imag, out_spectrum, info));
}

int smhip_arithmetic_fft_components(smhip_ctx* ctx, const float* f0, const float* f1, int rows, int cols, double t,
                                    int agreement, int do_imag, float* out_spectrum, void* stream) {
    SM_GUARD(ctx);
    if (!f0 || !f1 || !out_spectrum || rows < 1 || cols < 1) return ctx->pipe.fail(SMHIP_ERR_ARG, "bad argument");
    ctx->pipe.stream = stream;
    SM_FINISH(ctx, ctx->pipe.blend_full(f0, f1, rows, cols, smhip::BLEND_ARITH, t, 1.0, 0, 0, agreement, do_imag,
                                        out_spectrum, nullptr));
}

int smhip_merge_tensors_fft2_slerp(smhip_ctx* ctx, const float* v0, const float* v1, int rows, int cols, double t,
                                   double b, double t_sum, double cutoff_pct, double cull_pct, float* out,
                                   double* norm0, double* norm1, int* branch, smhip_blend_info* info, void* stream) {
    SM_GUARD(ctx);
    if (!v0 || !v1 || !out || rows < 1 || cols < 1) return ctx->pipe.fail(SMHIP_ERR_ARG, "bad argument");
    ctx->pipe.stream = stream;
    SM_FINISH(ctx, ctx->pipe.merge_pair_slerp(v0, v1, rows, cols, t, b, t_sum, cutoff_pct, cull_pct, out, norm0, norm1,
                                              branch, info));
}

int smhip_task_arithmetic_fft2(smhip_ctx* ctx, const float* v0, const float* v1, int rows, int cols, double t,
                               int agreement, float* out, void* stream) {
    SM_GUARD(ctx);
    if (!v0 || !v1 || !out || rows < 1 || cols < 1) return ctx->pipe.fail(SMHIP_ERR_ARG, "bad argument");
    ctx->pipe.stream = stream;
    smhip::SigDesc a{v0, nullptr, smhip::DT_F32, 1.f}, bb{v1, nullptr, smhip::DT_F32, 1.f};
    smhip::PairOut po;
    po.out = out; po.out_mode = smhip::OUT_F32; po.post = 1.f;
    const int rc0 = ctx->pipe.reserve(rows, cols);
    if (rc0) SM_FINISH(ctx, rc0);
    ctx->pipe.clear_flags();
    po.ifft_policy = 0;      // the reference's task_arithmetic_fft2 has no NaN/Inf policy of its own
    SM_FINISH(ctx, ctx->pipe.pair_arith(a, bb, rows, cols, 1.f, 1.f, t, agreement, po, -1, -1));
}

int smhip_merge_layer(smhip_ctx* ctx, const smhip_layer_desc* desc, void* out_bf16, float* delta_out,
                      smhip_layer_report* report, void* stream) {
    SM_GUARD(ctx);
    if (!desc || !out_bf16) return ctx->pipe.fail(SMHIP_ERR_ARG, "bad argument");
    for (int i = 0; i < desc->k && i < SMHIP_MAX_MODELS; ++i)
        if (!desc->finetune[i] || !desc->base[i]) return ctx->pipe.fail(SMHIP_ERR_ARG, "null model tensor");
    if (!desc->base_out) return ctx->pipe.fail(SMHIP_ERR_ARG, "null base_out");
    ctx->pipe.stream = stream;
    SM_FINISH(ctx, ctx->pipe.merge_layer(*desc, out_bf16, delta_out, report));
}

int smhip_addition_merge(smhip_ctx* ctx, int k, const void* const* finetunes, const void* base, int dtype, size_t n,
                         int sign_agreement, void* out, void* stream) {
    SM_GUARD(ctx);
    if (!finetunes || !base || !out || n < 1) return ctx->pipe.fail(SMHIP_ERR_ARG, "bad argument");
    if (dtype < SMHIP_BF16 || dtype > SMHIP_F32) return ctx->pipe.fail(SMHIP_ERR_ARG, "bad dtype");
    for (int i = 0; i < k && i < SMHIP_MAX_MODELS; ++i)
        if (!finetunes[i]) return ctx->pipe.fail(SMHIP_ERR_ARG, "null model tensor");
    ctx->pipe.stream = stream;
    SM_FINISH(ctx, ctx->pipe.addition_merge(k, finetunes, base, dtype, n, sign_agreement ? 1 : 0, out));
}

int smhip_ties_merge(smhip_ctx* ctx, const smhip_ties_desc* d, void* out, float* delta_out, smhip_ties_report* report,
                     void* stream) {
    SM_GUARD(ctx);
    if (int rc = delta_merge_check(ctx, "ties_merge", d, out, delta_out)) return rc;
    ctx->pipe.stream = stream;
    SM_FINISH(ctx, ctx->pipe.delta.ties_merge(*d, out, delta_out, report));
}

int smhip_dare_merge(smhip_ctx* ctx, const smhip_dare_desc* d, void* out, float* delta_out, smhip_dare_report* report,
                     void* stream) {
    SM_GUARD(ctx);
    if (int rc = delta_merge_check(ctx, "dare_merge", d, out, delta_out)) return rc;
    if (ctx->pipe.delta.dare_threshold(d->density) == 0)
        return ctx->pipe.fail(SMHIP_ERR_ARG, "dare_merge: density is below the smallest density, 2^-16 = 1.52587890625e-05 (the mask draws 16 bits per element)");
    ctx->pipe.stream = stream;
    SM_FINISH(ctx, ctx->pipe.delta.dare_merge(*d, out, delta_out, report));
}

int smhip_breadcrumbs_merge(smhip_ctx* ctx, const smhip_breadcrumbs_desc* d, void* out, float* delta_out,
                            smhip_breadcrumbs_report* report, void* stream) {
    SM_GUARD(ctx);
    if (int rc = delta_merge_check(ctx, "breadcrumbs_merge", d, out, delta_out)) return rc;
    if (!(d->gamma >= 0.0 && d->gamma < 1.0)) return ctx->pipe.fail(SMHIP_ERR_ARG, "breadcrumbs_merge: gamma must be in [0, 1)");
    if (!(d->density + d->gamma <= 1.0)) return ctx->pipe.fail(SMHIP_ERR_ARG, "breadcrumbs_merge: density + gamma must not exceed 1");
    ctx->pipe.stream = stream;
    SM_FINISH(ctx, ctx->pipe.delta.breadcrumbs_merge(*d, out, delta_out, report));
}

int smhip_geo_merge(smhip_ctx* ctx, const smhip_geo_desc* d, void* out, float* delta_out, smhip_geo_report* report,
                    void* stream) {
    SM_GUARD(ctx);
    const bool weight = d && d->mode == SMHIP_GEO_SLERP;
    if (int rc = delta_tensor_check(ctx, "geo_merge", d, out, delta_out, !weight, [&]() -> const char* {
            if (d->mode < SMHIP_GEO_MODEL_STOCK || d->mode > SMHIP_GEO_SLERP) return "bad mode";
            if (d->mode == SMHIP_GEO_MODEL_STOCK) return nullptr;
            if (d->rowwise) return "rowwise is an option of mode MODEL_STOCK";
            if (d->k > 2) return "modes NUSLERP and SLERP take k <= 2";
            if (d->k == 2 && !(d->alpha[0] >= 0.0 && d->alpha[1] >= 0.0 && d->alpha[0] + d->alpha[1] > 0.0 &&
                               std::isfinite(d->alpha[0] + d->alpha[1])))
                return "modes NUSLERP and SLERP need alphas >= 0 with a sum > 0";
            return nullptr;
        }))
        return rc;
    if (d->n > 0 && (d->rows < 1 || d->n % d->rows)) return ctx->pipe.fail(SMHIP_ERR_ARG, "geo_merge: rows must divide n");
    ctx->pipe.stream = stream;
    SM_FINISH(ctx, ctx->pipe.delta.geo_merge(*d, out, delta_out, report));
}

int smhip_sphere_merge(smhip_ctx* ctx, const smhip_sphere_desc* d, void* out, float* delta_out, smhip_sphere_report* report,
                       void* stream) {
    SM_GUARD(ctx);
    const bool weight = d && d->weight_space;
    if (int rc = delta_tensor_check(ctx, "sphere_merge", d, out, delta_out, !weight, [&]() -> const char* {
            double sum = 0.0;
            for (int i = 0; i < d->k; ++i) {
                if (!(d->alpha[i] >= 0.0) || !std::isfinite(d->alpha[i])) return "needs alphas >= 0 with a sum > 0";
                sum += d->alpha[i];
            }
            if (!(sum > 0.0) || !std::isfinite(sum)) return "needs alphas >= 0 with a sum > 0";
            if (d->max_iter < 1 || d->max_iter > 100) return "max_iter must be in 1..100";
            if (!(d->tol >= 0.0 && d->tol < 1.0)) return "tol must be in [0, 1)";
            return nullptr;
        }))
        return rc;
    if (d->n > 0 && (d->rows < 1 || d->n % d->rows)) return ctx->pipe.fail(SMHIP_ERR_ARG, "sphere_merge: rows must divide n");
    ctx->pipe.stream = stream;
    SM_FINISH(ctx, ctx->pipe.delta.sphere_merge(*d, out, delta_out, report));
}

int smhip_sphere_fn(smhip_ctx* ctx, int op, const double* x, double* y, size_t n, int on_device, void* stream) {
    SM_GUARD(ctx);
    if (op < SMHIP_SPHERE_ACOS || op > SMHIP_SPHERE_COS) return ctx->pipe.fail(SMHIP_ERR_ARG, "sphere_fn: bad op");
    if (n > 0 && (!x || !y)) return ctx->pipe.fail(SMHIP_ERR_ARG, "sphere_fn: null array");
    if ((uintptr_t)x % 8 || (uintptr_t)y % 8) return ctx->pipe.fail(SMHIP_ERR_ARG, "sphere_fn: a pointer is not aligned to 8 bytes");
    if (n > ((size_t)1 << 30)) return ctx->pipe.fail(SMHIP_ERR_ARG, "sphere_fn: array too large");
    ctx->pipe.stream = stream;
    SM_FINISH(ctx, ctx->pipe.delta.sphere_fn_array(op, x, y, n, on_device != 0));
}

int smhip_sce_merge(smhip_ctx* ctx, const smhip_sce_desc* d, void* out, float* delta_out, smhip_sce_report* report,
                    void* stream) {
    SM_GUARD(ctx);
    if (int rc = delta_tensor_check(ctx, "sce_merge", d, out, delta_out, true, [&]() -> const char* {
            if (!(d->select_topk > 0.0 && d->select_topk <= 1.0)) return "select_topk must be in (0, 1]";
            if (!std::isfinite(d->lambda)) return "lambda is not finite";
            double sum = 0.0;
            for (int i = 0; i < d->k; ++i) {
                if (!(d->alpha[i] >= 0.0) || !std::isfinite(d->alpha[i])) return "every alpha must be >= 0 and finite";
                sum += d->alpha[i];
            }
            if (!(sum > 0.0) || !std::isfinite(sum)) return "the alphas need a sum > 0";
            return nullptr;
        }))
        return rc;
    ctx->pipe.stream = stream;
    SM_FINISH(ctx, ctx->pipe.delta.sce_merge(*d, out, delta_out, report));
}

int smhip_della_merge(smhip_ctx* ctx, const smhip_della_desc* d, void* out, float* delta_out, uint16_t* threshold_out,
                      smhip_della_report* report, void* stream) {
    SM_GUARD(ctx);
    if (int rc = delta_tensor_check(ctx, "della_merge", d, out, delta_out, true, [&]() -> const char* {
            if (!(d->density > 0.0 && d->density <= 1.0)) return "density must be in (0, 1]";
            if (!std::isfinite(d->lambda)) return "lambda is not finite";
            if (!(d->epsilon >= 0.0)) return "epsilon must be >= 0";
            if (d->density == 1.0) return d->epsilon == 0.0 ? nullptr : "density 1 keeps everything: it requires epsilon 0";
            if (d->epsilon == 0.0)
                return ctx->pipe.delta.dare_threshold(d->density) >= 1 ? nullptr : "density is below the smallest density, 2^-16 = 1.52587890625e-05 (the mask draws 16 bits per element)";
            if (!(d->density + d->epsilon < 1.0)) return "density + epsilon must be below 1";
            if (!(std::floor((d->density - d->epsilon) * 65536.0) >= 1.0)) return "floor((density - epsilon) * 65536) must be at least 1 (the mask draws 16 bits per element)";
            return nullptr;
        }))
        return rc;
    if (d->n > 0) {
        if (d->rows < 1 || d->n % d->rows) return ctx->pipe.fail(SMHIP_ERR_ARG, "della_merge: rows must divide n");
        const size_t c = d->n / d->rows;
        if (d->epsilon > 0.0 && c > (size_t)smhip::DELLA_MAX_COLS)
            return ctx->pipe.fail(SMHIP_ERR_SHAPE, "della_merge: rows of c = " + std::to_string(c) + " elements exceed the limit of " +
                                                       std::to_string(smhip::DELLA_MAX_COLS) + " (a row is sorted in the LDS of one compute unit)");
        if (threshold_out) {
            const uintptr_t t0 = (uintptr_t)threshold_out, t1 = t0 + (size_t)d->k * d->n * 2;
            const size_t ies = d->in_dtype == SMHIP_F32 ? 4 : 2, oes = d->base_out_dtype == SMHIP_F32 ? 4 : 2;
            auto hits = [&](const void* p, size_t bytes) { return p && (uintptr_t)p < t1 && t0 < (uintptr_t)p + bytes; };
            bool hit = t0 % 2 != 0 || hits(out, d->n * oes) || hits(delta_out, d->n * 4) || hits(d->base_out, d->n * oes);
            for (int i = 0; i < d->k; ++i) hit = hit || hits(d->finetune[i], d->n * ies) || hits(d->base[i], d->n * ies);
            if (hit) return ctx->pipe.fail(SMHIP_ERR_ARG, "della_merge: threshold_out is misaligned or overlaps another tensor");
        }
    }
    ctx->pipe.stream = stream;
    SM_FINISH(ctx, ctx->pipe.delta.della_merge(*d, out, delta_out, threshold_out, report));
}

int smhip_consensus_merge(smhip_ctx* ctx, const smhip_consensus_desc* d, void* out, float* delta_out,
                          smhip_consensus_report* report, void* stream) {
    SM_GUARD(ctx);
    if (int rc = delta_tensor_check(ctx, "consensus_merge", d, out, delta_out, true, [&]() -> const char* {
            if (d->consensus_k < 1 || d->consensus_k > SMHIP_MAX_MODELS) return "consensus_k out of range (1..16)";
            if (!(d->mask_lambda >= 0.0 && d->mask_lambda <= 1e6)) return "mask_lambda must be in [0, 1e6]";
            if (d->ties && !(d->density > 0.0 && d->density <= 1.0)) return "density must be in (0, 1]";
            if (!std::isfinite(d->lambda)) return "lambda is not finite";
            return nullptr;
        }))
        return rc;
    ctx->pipe.stream = stream;
    SM_FINISH(ctx, ctx->pipe.delta.consensus_merge(*d, out, delta_out, report));
}

int smhip_fusion_merge(smhip_ctx* ctx, const smhip_fusion_desc* d, void* out, float* delta_out, smhip_fusion_report* report,
                       void* stream) {
    SM_GUARD(ctx);
    if (int rc = delta_tensor_check(ctx, "fusion_merge", d, out, delta_out, true, [&]() -> const char* {
            if (d->k != 1) return "k must be 1 (one finetune and its base)";
            if (d->mode != SMHIP_FUSION_ARCEE && d->mode != SMHIP_FUSION_NEARSWAP) return "bad mode";
            if (d->mode == SMHIP_FUSION_NEARSWAP && !(d->t > 0.0 && std::isfinite(d->t) && (float)d->t > 0.f && std::isfinite((float)d->t)))
                return "t must be > 0 and finite";
            if (d->mode == SMHIP_FUSION_ARCEE && !std::isfinite((float)d->iqr_mult)) return "iqr_mult is not finite";
            return nullptr;
        }))
        return rc;
    if (d->n > 0) {
        if (d->rows < 1 || d->n % d->rows) return ctx->pipe.fail(SMHIP_ERR_ARG, "fusion_merge: rows must divide n");
        if (d->mode == SMHIP_FUSION_ARCEE && d->kl_out) {
            const uintptr_t k0 = (uintptr_t)d->kl_out, k1 = k0 + d->rows * 4;
            const size_t ies = d->in_dtype == SMHIP_F32 ? 4 : 2, oes = d->base_out_dtype == SMHIP_F32 ? 4 : 2;
            auto hits = [&](const void* p, size_t bytes) { return p && (uintptr_t)p < k1 && k0 < (uintptr_t)p + bytes; };
            if (k0 % 4 || hits(out, d->n * oes) || hits(delta_out, d->n * 4) || hits(d->base_out, d->n * oes) ||
                hits(d->finetune[0], d->n * ies) || hits(d->base[0], d->n * ies))
                return ctx->pipe.fail(SMHIP_ERR_ARG, "fusion_merge: kl_out is misaligned or overlaps another tensor");
        }
    }
    ctx->pipe.stream = stream;
    SM_FINISH(ctx, ctx->pipe.delta.fusion_merge(*d, out, delta_out, report));
}

int smhip_fusion_fn(smhip_ctx* ctx, int op, const double* x, double* y, size_t n, int on_device, void* stream) {
    SM_GUARD(ctx);
    if (op != SMHIP_FUSION_EXP && op != SMHIP_FUSION_LOG) return ctx->pipe.fail(SMHIP_ERR_ARG, "fusion_fn: bad op");
    if (n > 0 && (!x || !y)) return ctx->pipe.fail(SMHIP_ERR_ARG, "fusion_fn: null array");
    if ((uintptr_t)x % 8 || (uintptr_t)y % 8) return ctx->pipe.fail(SMHIP_ERR_ARG, "fusion_fn: a pointer is not aligned to 8 bytes");
    if (n > ((size_t)1 << 30)) return ctx->pipe.fail(SMHIP_ERR_ARG, "fusion_fn: array too large");
    ctx->pipe.stream = stream;
    SM_FINISH(ctx, ctx->pipe.delta.fusion_fn_array(op, x, y, n, on_device != 0));
}

int smhip_pcb_merge(smhip_ctx* ctx, const smhip_pcb_desc* d, void* out, float* delta_out, smhip_pcb_report* report, void* stream) {
    SM_GUARD(ctx);
    if (int rc = delta_tensor_check(ctx, "pcb_merge", d, out, delta_out, true, [&]() -> const char* {
            if (!(d->ratio > 0.0 && d->ratio <= 1.0)) return "ratio must be in (0, 1]";
            if (!(d->clip >= 0.0 && d->clip < 0.5)) return "clip must be in [0, 0.5)";
            if (!std::isfinite(d->lambda)) return "lambda is not finite";
            return nullptr;
        }))
        return rc;
    ctx->pipe.stream = stream;
    SM_FINISH(ctx, ctx->pipe.delta.pcb_merge(*d, out, delta_out, report));
}

int smhip_pcb_fn(smhip_ctx* ctx, int op, const double* x, double* y, size_t n, int on_device, void* stream) {
    SM_GUARD(ctx);
    if (op != SMHIP_PCB_TANH) return ctx->pipe.fail(SMHIP_ERR_ARG, "pcb_fn: bad op");
    if (n > 0 && (!x || !y)) return ctx->pipe.fail(SMHIP_ERR_ARG, "pcb_fn: null array");
    if ((uintptr_t)x % 8 || (uintptr_t)y % 8) return ctx->pipe.fail(SMHIP_ERR_ARG, "pcb_fn: a pointer is not aligned to 8 bytes");
    if (n > ((size_t)1 << 30)) return ctx->pipe.fail(SMHIP_ERR_ARG, "pcb_fn: array too large");
    ctx->pipe.stream = stream;
    SM_FINISH(ctx, ctx->pipe.delta.pcb_fn_array(op, x, y, n, on_device != 0));
}

int smhip_delta_stats(smhip_ctx* ctx, const smhip_stats_desc* d, smhip_stats_report* report, void* stream) {
    SM_GUARD(ctx);
    auto bad = [&](const char* what) { return ctx->pipe.fail(SMHIP_ERR_ARG, std::string("delta_stats: ") + what); };
    if (!d) return bad("null descriptor");
    if (!report) return bad("null report");
    if (d->k < 1 || d->k > SMHIP_MAX_MODELS) return bad("k out of range (1..16)");
    if (d->in_dtype < SMHIP_BF16 || d->in_dtype > SMHIP_F32) return bad("bad dtype");
    if (d->m < 1 || d->m > SMHIP_STATS_MAX_DENSITIES) return bad("m out of range (1..4)");
    for (int q = 0; q < d->m; ++q)
        if (!(d->density[q] > 0.0 && d->density[q] <= 1.0)) return bad("density must be in (0, 1]");
    for (int i = 0; i < d->k; ++i)
        if (!std::isfinite(d->alpha[i])) return bad("an alpha is not finite");
    const size_t ies = d->in_dtype == SMHIP_F32 ? 4 : 2;
    for (int i = 0; i < d->k && d->n > 0; ++i) {
        if (!d->finetune[i] || !d->base[i]) return bad("null model tensor");
        if ((uintptr_t)d->finetune[i] % ies || (uintptr_t)d->base[i] % ies) return bad("a pointer is not aligned to its element size");
    }
    if ((d->n + 7) / 8 / 256 > (size_t)1 << 30) return bad("tensor too large");
    ctx->pipe.stream = stream;
    SM_FINISH(ctx, ctx->pipe.delta.delta_stats(*d, report));
}

int smhip_slerp(smhip_ctx* ctx, const float* v0, const float* v1, size_t rows, size_t cols, float t, float* out, void* stream) {
    SM_GUARD(ctx);
    if (rows * cols > 0 && (!v0 || !v1 || !out)) return ctx->pipe.fail(SMHIP_ERR_ARG, "bad argument");
    ctx->pipe.stream = stream;
    SM_FINISH(ctx, ctx->pipe.fn_slerp(v0, v1, rows, cols, t, out));
}

int smhip_div_scalar(smhip_ctx* ctx, const void* x, int dtype, size_t n, float s, void* out, void* stream) {
    SM_GUARD(ctx);
    if (n > 0 && (!x || !out)) return ctx->pipe.fail(SMHIP_ERR_ARG, "bad argument");
    if (dtype < SMHIP_BF16 || dtype > SMHIP_F32) return ctx->pipe.fail(SMHIP_ERR_ARG, "bad dtype");
    ctx->pipe.stream = stream;
    SM_FINISH(ctx, ctx->pipe.fn_div_scalar(x, dtype, n, s, out));
}

int smhip_lora_apply(smhip_ctx* ctx, const void* base, int dtype, int rows, int cols, const void* lora_a,
                     const void* lora_b, int factor_dtype, int rank, float scale, void* out, void* stream) {
    SM_GUARD(ctx);
    if (!base || !lora_a || !lora_b || !out || rows < 1 || cols < 1) return ctx->pipe.fail(SMHIP_ERR_ARG, "bad argument");
    if (dtype < SMHIP_BF16 || dtype > SMHIP_F32 || factor_dtype < SMHIP_BF16 || factor_dtype > SMHIP_F32)
        return ctx->pipe.fail(SMHIP_ERR_ARG, "bad dtype");
    if (rank < 1 || rank > smhip::LORA_MAX_RANK) return ctx->pipe.fail(SMHIP_ERR_ARG, "rank out of range (1..512)");
    const size_t bes = dtype == SMHIP_F32 ? 4 : 2, fes = factor_dtype == SMHIP_F32 ? 4 : 2;
    const uintptr_t o0 = (uintptr_t)out, o1 = o0 + (size_t)rows * cols * bes;
    auto overlaps = [&](const void* p, size_t bytes) { return (uintptr_t)p < o1 && o0 < (uintptr_t)p + bytes; };
    if (overlaps(base, (size_t)rows * cols * bes) || overlaps(lora_a, (size_t)rank * cols * fes) ||
        overlaps(lora_b, (size_t)rows * rank * fes))
        return ctx->pipe.fail(SMHIP_ERR_ARG, "lora_apply: out overlaps an input");
    ctx->pipe.stream = stream;
    SM_FINISH(ctx, ctx->pipe.lora_apply(base, dtype, rows, cols, lora_a, lora_b, factor_dtype, rank, scale, out));
}

int smhip_adapter_apply(smhip_ctx* ctx, const smhip_adapter_desc* d, void* stream) {
    SM_GUARD(ctx);
    if (!d || !d->base || !d->lora_a || !d->lora_b || !d->out || d->rows < 1 || d->cols < 1)
        return ctx->pipe.fail(SMHIP_ERR_ARG, "bad argument");
    if (d->dtype < SMHIP_BF16 || d->dtype > SMHIP_F32 || d->factor_dtype < SMHIP_BF16 || d->factor_dtype > SMHIP_F32 ||
        (d->magnitude && (d->magnitude_dtype < SMHIP_BF16 || d->magnitude_dtype > SMHIP_F32)))
        return ctx->pipe.fail(SMHIP_ERR_ARG, "bad dtype");
    if (d->layout != SMHIP_ADAPTER_LINEAR && d->layout != SMHIP_ADAPTER_EMBEDDING)
        return ctx->pipe.fail(SMHIP_ERR_ARG, "adapter_apply: bad layout");
    if (d->magnitude && d->layout != SMHIP_ADAPTER_LINEAR)
        return ctx->pipe.fail(SMHIP_ERR_ARG, "adapter_apply: DoRA (a magnitude) needs the LINEAR layout");
    if (d->rank < 1 || d->rank > smhip::LORA_MAX_RANK) return ctx->pipe.fail(SMHIP_ERR_ARG, "rank out of range (1..512)");
    const size_t bes = d->dtype == SMHIP_F32 ? 4 : 2, fes = d->factor_dtype == SMHIP_F32 ? 4 : 2;
    const size_t mes = d->magnitude_dtype == SMHIP_F32 ? 4 : 2;
    const bool emb = d->layout == SMHIP_ADAPTER_EMBEDDING;
    const uintptr_t o0 = (uintptr_t)d->out, o1 = o0 + (size_t)d->rows * d->cols * bes;
    auto overlaps = [&](const void* p, size_t bytes) { return (uintptr_t)p < o1 && o0 < (uintptr_t)p + bytes; };
    if (overlaps(d->base, (size_t)d->rows * d->cols * bes) ||
        overlaps(d->lora_a, (size_t)d->rank * (emb ? d->rows : d->cols) * fes) ||
        overlaps(d->lora_b, (size_t)(emb ? d->cols : d->rows) * d->rank * fes) ||
        (d->magnitude && overlaps(d->magnitude, (size_t)d->rows * mes)))
        return ctx->pipe.fail(SMHIP_ERR_ARG, "adapter_apply: out overlaps an input");
    ctx->pipe.stream = stream;
    SM_FINISH(ctx, ctx->pipe.adapter_apply(d->base, d->dtype, d->rows, d->cols, d->lora_a, d->lora_b, d->factor_dtype,
                                           d->rank, d->scale, emb ? 1 : 0, d->magnitude, d->magnitude_dtype, d->out));
}

size_t smhip_lora_extract_workspace(int rows, int cols, int rank) {
    if (rows < 1 || cols < 1 || rank < 1 || rank > smhip::XL_MAX_RANK) return 0;
    return smhip::DeltaHost<SM_BACKEND>::xl_layout(rows, cols, rank).total;
}
size_t smhip_xl_probe_workspace(int rows, int cols, int L) {
    if (rows < 1 || cols < 1 || L < 16 || L > smhip::XL_MAX_L || L % 16) return 0;
    return smhip::DeltaHost<SM_BACKEND>::xl_layout_L(rows, cols, L, L).total;
}

int smhip_lora_extract(smhip_ctx* ctx, const smhip_extract_desc* d, void* a_out, void* b_out,
                       smhip_extract_report* report, void* stream) {
    SM_GUARD(ctx);
    auto bad = [&](const char* what) { return ctx->pipe.fail(SMHIP_ERR_ARG, std::string("lora_extract: ") + what); };
    if (!d || !report || !a_out || !b_out) return bad("null descriptor, report or output");
    if (!d->finetune || !d->base) return bad("null model tensor");
    if (d->rows < 1 || d->cols < 1) return bad("rows and cols must be >= 1");
    if (d->in_dtype < SMHIP_BF16 || d->in_dtype > SMHIP_F32 || d->factor_dtype < SMHIP_BF16 || d->factor_dtype > SMHIP_F32)
        return bad("bad dtype");
    if (d->rank < 1 || d->rank > smhip::XL_MAX_RANK) return bad("rank out of range (1..256)");
    if (d->power_iters < 0 || d->power_iters > smhip::XL_MAX_POWER) return bad("power_iters out of range (0..4)");
    const size_t ies = d->in_dtype == SMHIP_F32 ? 4 : 2, fes = d->factor_dtype == SMHIP_F32 ? 4 : 2;
    if ((uintptr_t)d->finetune % ies || (uintptr_t)d->base % ies || (uintptr_t)a_out % fes || (uintptr_t)b_out % fes)
        return bad("a pointer is not aligned to its element size");
    if ((size_t)d->rows * d->cols / smhip::GEO_SEG_ELEMS > (size_t)1 << 30) return bad("tensor too large");
    if (!d->workspace || (uintptr_t)d->workspace % 256 || d->workspace_bytes < smhip_lora_extract_workspace(d->rows, d->cols, d->rank))
        return bad("the workspace is null, not 256-byte aligned or too small (smhip_lora_extract_workspace)");
    ctx->pipe.stream = stream;
    SM_FINISH(ctx, ctx->pipe.delta.lora_extract(*d, a_out, b_out, report));
}

int smhip_xl_probe(smhip_ctx* ctx, const smhip_xl_probe_desc* d, void* stream) {
    SM_GUARD(ctx);
    auto bad = [&](const char* what) { return ctx->pipe.fail(SMHIP_ERR_ARG, std::string("xl_probe: ") + what); };
    if (!d || !d->y) return bad("null descriptor or output");
    if (d->op < SMHIP_XL_FILL || d->op > SMHIP_XL_SYM_EIG) return bad("bad op");
    if (d->op == SMHIP_XL_SYM_EIG) {
        if (!d->x || d->L < 1 || d->L > smhip::XL_MAX_L) return bad("bad argument");
    } else {
        if (d->L < 16 || d->L > smhip::XL_MAX_L || d->L % 16 || d->rows < 1) return bad("bad shape");
        if (d->op != SMHIP_XL_FILL && !d->x) return bad("null panel");
        if (d->op == SMHIP_XL_DELTA_MM && (!d->finetune || !d->base || d->cols < 1 || d->in_dtype < SMHIP_BF16 || d->in_dtype > SMHIP_F32))
            return bad("bad delta");
        if (d->op == SMHIP_XL_GRAM && d->cols != 1) return bad("gram: cols must be 1");
        if (d->op == SMHIP_XL_PANEL_MM && (!d->t || d->L2 < 1 || d->out_dtype < SMHIP_BF16 || d->out_dtype > SMHIP_F32))
            return bad("bad panel product");
        if ((d->op == SMHIP_XL_DELTA_MM || d->op == SMHIP_XL_GRAM) && (uintptr_t)d->workspace % 256) return bad("the workspace is not 256-byte aligned");
    }
    ctx->pipe.stream = stream;
    SM_FINISH(ctx, ctx->pipe.delta.xl_probe(*d));
}

size_t smhip_tsv_workspace(int rows, int cols, int k, int rank) {
    if (rows < 1 || cols < 1 || k < 1 || k > SMHIP_MAX_MODELS || rank < 1 || rank > smhip::XL_MAX_RANK) return 0;
    return smhip::DeltaHost<SM_BACKEND>::tsv_layout(rows, cols, k, rank).total;
}

int smhip_tsv_merge(smhip_ctx* ctx, const smhip_tsv_desc* d, void* out, float* delta_out, smhip_tsv_report* report, void* stream) {
    SM_GUARD(ctx);
    if (int rc = delta_tensor_check(ctx, "tsv_merge", d, out, delta_out, true, [&]() -> const char* {
            if (!std::isfinite(d->lambda)) return "lambda is not finite";
            if (d->rank < 1 || d->rank > smhip::XL_MAX_RANK) return "rank out of range (1..256)";
            if (d->power_iters < 0 || d->power_iters > smhip::XL_MAX_POWER) return "power_iters out of range (0..4)";
            for (int i = 0; i < d->k; ++i)
                if (d->alpha[i] < 0.0) return "an alpha is negative";
            return nullptr;
        }))
        return rc;
    auto bad = [&](const char* what) { return ctx->pipe.fail(SMHIP_ERR_ARG, std::string("tsv_merge: ") + what); };
    if (d->n > 0) {
        if (d->rows < 1 || d->cols < 1 || (size_t)d->rows * (size_t)d->cols != d->n) return bad("rows and cols must be >= 1 and rows * cols == n");
        int active = 0;
        for (int i = 0; i < d->k; ++i) active += d->alpha[i] != 0.0;
        const int r = std::min(d->rank, std::min(d->rows, d->cols));
        if (active * r > SMHIP_TSV_MAX_R) return bad("active finetunes * min(rank, rows, cols) exceeds 256");
        if (d->n / smhip::GEO_SEG_ELEMS > (size_t)1 << 30) return bad("tensor too large");
        if (!d->workspace || (uintptr_t)d->workspace % 256 || d->workspace_bytes < smhip_tsv_workspace(d->rows, d->cols, d->k, d->rank))
            return bad("the workspace is null, not 256-byte aligned or too small (smhip_tsv_workspace)");
    }
    ctx->pipe.stream = stream;
    SM_FINISH(ctx, ctx->pipe.delta.tsv_merge(*d, out, delta_out, report));
}

int smhip_widen_merge(smhip_ctx* ctx, const smhip_widen_desc* d, void* out, float* delta_out, double* stat_out,
                      uint32_t* rank_out, float* weight_out, smhip_widen_report* report, void* stream) {
    SM_GUARD(ctx);
    if (int rc = delta_tensor_check(ctx, "widen_merge", d, out, delta_out, true, [&]() -> const char* {
            if (!std::isfinite(d->ratio)) return "ratio is not finite";
            if (!(d->calibration >= 0.0) || !std::isfinite(d->calibration)) return "calibration must be finite and >= 0";
            if (!std::isfinite(d->lambda)) return "lambda is not finite";
            return nullptr;
        }))
        return rc;
    auto bad = [&](const char* what) { return ctx->pipe.fail(SMHIP_ERR_ARG, std::string("widen_merge: ") + what); };
    if (d->n > 0) {
        if (d->rows < 1 || d->n % d->rows) return bad("rows must divide n");
        const size_t C = d->n / d->rows;
        if (C > smhip::WIDEN_MAX_COLS) return bad("more than 65536 columns");
        if ((uintptr_t)stat_out % 8 || (uintptr_t)rank_out % 4 || (uintptr_t)weight_out % 4)
            return bad("a pointer is not aligned to its element size");
    }
    ctx->pipe.stream = stream;
    SM_FINISH(ctx, ctx->pipe.delta.widen_merge(*d, out, delta_out, stat_out, rank_out, weight_out, report));
}

int smhip_cabs_merge(smhip_ctx* ctx, const smhip_cabs_desc* d, void* out, float* delta_out, uint16_t* mask_out,
                     smhip_cabs_report* report, void* stream) {
    SM_GUARD(ctx);
    if (int rc = delta_tensor_check(ctx, "cabs_merge", d, out, delta_out, true, [&]() -> const char* {
            const int M = d->group;
            if (M < smhip::CABS_MIN_GROUP || M > smhip::CABS_MAX_GROUP || (M & (M - 1))) return "group must be a power of two in 4..512";
            if (d->n_keep < 1 || d->n_keep > M) return "n_keep must be in 1..group";
            if (d->conflict_aware != 0 && d->conflict_aware != 1) return "conflict_aware must be 0 or 1";
            if (!std::isfinite(d->lambda)) return "lambda is not finite";
            return nullptr;
        }))
        return rc;
    if (d->n > 0) {
        if (d->rows < 1 || d->n % d->rows) return ctx->pipe.fail(SMHIP_ERR_ARG, "cabs_merge: rows must divide n");
        if (mask_out) {
            const uintptr_t t0 = (uintptr_t)mask_out, t1 = t0 + d->n * 2;
            const size_t ies = d->in_dtype == SMHIP_F32 ? 4 : 2, oes = d->base_out_dtype == SMHIP_F32 ? 4 : 2;
            auto hits = [&](const void* p, size_t bytes) { return p && (uintptr_t)p < t1 && t0 < (uintptr_t)p + bytes; };
            bool hit = t0 % 2 != 0 || hits(out, d->n * oes) || hits(delta_out, d->n * 4) || hits(d->base_out, d->n * oes);
            for (int i = 0; i < d->k; ++i) hit = hit || hits(d->finetune[i], d->n * ies) || hits(d->base[i], d->n * ies);
            if (hit) return ctx->pipe.fail(SMHIP_ERR_ARG, "cabs_merge: mask_out is misaligned or overlaps another tensor");
        }
    }
    ctx->pipe.stream = stream;
    SM_FINISH(ctx, ctx->pipe.delta.cabs_merge(*d, out, delta_out, mask_out, report));
}

}  // extern "C"

// what smhip_dpack_pack and smhip_dpack_apply share: the shape, the dtype and the tensors' spans ({pointer, bytes,
// alignment}; ins are read, outs written).  n == 0: only the shape and the dtype are checked
struct dpack_span { const void* p; size_t bytes, align; };
static int dpack_check(smhip_ctx* ctx, const char* op, int dtype, size_t rows, size_t cols, int scale_mode,
                       std::initializer_list<dpack_span> ins, std::initializer_list<dpack_span> outs) {
    auto bad = [&](const char* what) { return ctx->pipe.fail(SMHIP_ERR_ARG, std::string(op) + ": " + what); };
    if (dtype < SMHIP_BF16 || dtype > SMHIP_F32) return bad("bad dtype");
    if (scale_mode != SMHIP_DPACK_ROW && scale_mode != SMHIP_DPACK_TENSOR) return bad("bad scale_mode");
    if (rows && cols > ((size_t)1 << 40) / rows) return bad("tensor too large");
    for (const dpack_span& o : outs) {
        if (!o.bytes) continue;
        if (!o.p) return bad("null pointer");
        if ((uintptr_t)o.p % o.align) return bad("a pointer is not aligned to its element size");
        for (const dpack_span& i : ins)
            if (i.p && i.bytes && (uintptr_t)i.p < (uintptr_t)o.p + o.bytes && (uintptr_t)o.p < (uintptr_t)i.p + i.bytes)
                return bad("an output overlaps an input");
        for (const dpack_span& q : outs)
            if (q.p != o.p && q.bytes && (uintptr_t)q.p < (uintptr_t)o.p + o.bytes && (uintptr_t)o.p < (uintptr_t)q.p + q.bytes)
                return bad("two outputs overlap");
    }
    for (const dpack_span& i : ins) {
        if (!i.bytes) continue;
        if (!i.p) return bad("null pointer");
        if ((uintptr_t)i.p % i.align) return bad("a pointer is not aligned to its element size");
    }
    return SMHIP_OK;
}

extern "C" {

int smhip_dpack_pack(smhip_ctx* ctx, const smhip_dpack_desc* d, uint8_t* sign, uint8_t* mask, float* scale,
                     smhip_dpack_report* report, void* stream) {
    SM_GUARD(ctx);
    auto bad = [&](const char* what) { return ctx->pipe.fail(SMHIP_ERR_ARG, std::string("dpack_pack: ") + what); };
    if (!d) return bad("null descriptor");
    if (d->bits != 1 && d->bits != 2) return bad("bits must be 1 or 2");
    if (!(d->density > 0.0 && d->density <= 1.0)) return bad("density must be in (0, 1]");
    if (d->bits == 1 && d->density != 1.0) return bad("bits == 1 needs density == 1");
    const size_t es = d->dtype == SMHIP_F32 ? 4 : 2, n = d->rows * d->cols, plane = d->rows * ((d->cols + 7) / 8);
    const size_t ns = d->scale_mode == SMHIP_DPACK_TENSOR ? 1 : d->rows;
    if (d->bits == 1 && mask) return bad("a mask with bits == 1");
    if (int rc = dpack_check(ctx, "dpack_pack", d->dtype, d->rows, d->cols, d->scale_mode,
                             {{d->finetune, n * es, es}, {d->base, n * es, es}},
                             {{sign, plane, 1}, {mask, d->bits == 2 ? plane : 0, 1}, {scale, ns * 4, 4}}))
        return rc;
    ctx->pipe.stream = stream;
    SM_FINISH(ctx, ctx->pipe.delta.dpack_pack(*d, sign, mask, scale, report));
}

int smhip_dpack_apply(smhip_ctx* ctx, const smhip_dpack_apply_desc* d, void* out, void* stream) {
    SM_GUARD(ctx);
    if (!d) return ctx->pipe.fail(SMHIP_ERR_ARG, "dpack_apply: null descriptor");
    const size_t es = d->dtype == SMHIP_F32 ? 4 : 2, n = d->rows * d->cols, plane = n ? d->rows * ((d->cols + 7) / 8) : 0;
    const size_t ns = !n ? 0 : (d->scale_mode == SMHIP_DPACK_TENSOR ? 1 : d->rows);
    if (int rc = dpack_check(ctx, "dpack_apply", d->dtype, d->rows, d->cols, d->scale_mode,
                             {{d->base, n * es, es}, {d->sign, plane, 1}, {d->mask, d->mask ? plane : 0, 1}, {d->scale, ns * 4, 4}},
                             {{out, n * es, es}}))
        return rc;
    ctx->pipe.stream = stream;
    SM_FINISH(ctx, ctx->pipe.delta.dpack_apply(*d, out));
}

int smhip_emr_merge(smhip_ctx* ctx, const smhip_emr_desc* d, void* out, float* delta_out, smhip_emr_report* report,
                    void* stream) {
    SM_GUARD(ctx);
    if (int rc = delta_tensor_check(ctx, "emr_merge", d, out, delta_out, true, [&]() -> const char* {
            if (!std::isfinite(d->lambda)) return "lambda is not finite";
            return nullptr;
        }))
        return rc;
    ctx->pipe.stream = stream;
    SM_FINISH(ctx, ctx->pipe.delta.emr_merge(*d, out, delta_out, report));
}

int smhip_emr_mask(smhip_ctx* ctx, const smhip_emr_mask_desc* d, uint8_t* mask, float* scale, smhip_emr_mask_report* report,
                   void* stream) {
    SM_GUARD(ctx);
    if (!d) return ctx->pipe.fail(SMHIP_ERR_ARG, "emr_mask: null descriptor");
    const size_t es = d->dtype == SMHIP_F32 ? 4 : 2, n = d->rows * d->cols, plane = d->rows * ((d->cols + 7) / 8);
    if (int rc = dpack_check(ctx, "emr_mask", d->dtype, d->rows, d->cols, SMHIP_DPACK_TENSOR,
                             {{d->finetune, n * es, es}, {d->base, n * es, es}, {d->unified, n * es, es}},
                             {{mask, plane, 1}, {scale, 4, 4}}))
        return rc;
    ctx->pipe.stream = stream;
    SM_FINISH(ctx, ctx->pipe.delta.emr_mask(*d, mask, scale, report));
}

int smhip_emr_merge_masks(smhip_ctx* ctx, const smhip_emr_desc* d, size_t rows, size_t cols, void* out, float* delta_out,
                          uint8_t* const* masks, float* const* scales, smhip_emr_report* report,
                          smhip_emr_mask_report* mask_reports, void* stream) {
    SM_GUARD(ctx);
    if (int rc = delta_tensor_check(ctx, "emr_merge_masks", d, out, delta_out, true, [&]() -> const char* {
            if (!std::isfinite(d->lambda)) return "lambda is not finite";
            return nullptr;
        }))
        return rc;
    auto bad = [&](const char* what) { return ctx->pipe.fail(SMHIP_ERR_ARG, std::string("emr_merge_masks: ") + what); };
    if (rows && cols > ((size_t)1 << 40) / rows) return bad("tensor too large");
    if (rows * cols != d->n) return bad("rows * cols is not n");
    if (cols >= (size_t)1 << 31) return bad("a row of 2^31 elements or more");
    if (!masks || !scales) return bad("null masks or scales");
    const size_t ies = d->in_dtype == SMHIP_F32 ? 4 : 2, oes = d->base_out_dtype == SMHIP_F32 ? 4 : 2, plane = rows * ((cols + 7) / 8);
    auto overlaps = [&](const void* o, size_t obytes, const void* q, size_t bytes) {
        return o && q && obytes && bytes && (uintptr_t)q < (uintptr_t)o + obytes && (uintptr_t)o < (uintptr_t)q + bytes;
    };
    for (int i = 0; i < d->k; ++i) {
        if (!scales[i] || (plane && !masks[i])) return bad("null mask or scale");
        if ((uintptr_t)scales[i] % 4) return bad("a pointer is not aligned to its element size");
        // a plane or a rescaler is written while every input is still read, and after out
        const void* outs[2] = {masks[i], scales[i]};
        const size_t obytes[2] = {plane, 4};
        for (int o = 0; o < 2; ++o) {
            bool hit = overlaps(outs[o], obytes[o], out, d->n * oes) || overlaps(outs[o], obytes[o], delta_out, d->n * 4) ||
                       overlaps(outs[o], obytes[o], d->base_out, d->n * oes);
            for (int j = 0; j < d->k; ++j) {
                hit = hit || overlaps(outs[o], obytes[o], d->finetune[j], d->n * ies) || overlaps(outs[o], obytes[o], d->base[j], d->n * ies);
                if (j != i) hit = hit || overlaps(outs[o], obytes[o], masks[j], plane) || overlaps(outs[o], obytes[o], scales[j], 4);
            }
            hit = hit || (o == 0 && overlaps(masks[i], plane, scales[i], 4));
            if (hit) return bad("a mask or a scale overlaps another tensor");
        }
    }
    ctx->pipe.stream = stream;
    SM_FINISH(ctx, ctx->pipe.delta.emr_merge_masks(*d, rows, cols, out, delta_out, masks, scales, report, mask_reports));
}

int smhip_emr_apply(smhip_ctx* ctx, const smhip_emr_apply_desc* d, void* out, void* stream) {
    SM_GUARD(ctx);
    if (!d) return ctx->pipe.fail(SMHIP_ERR_ARG, "emr_apply: null descriptor");
    const size_t es = d->dtype == SMHIP_F32 ? 4 : 2, n = d->rows * d->cols, plane = n ? d->rows * ((d->cols + 7) / 8) : 0;
    if (int rc = dpack_check(ctx, "emr_apply", d->dtype, d->rows, d->cols, SMHIP_DPACK_TENSOR,
                             {{d->base, n * es, es}, {d->unified, n * es, es}, {d->mask, plane, 1}, {d->scale, n ? (size_t)4 : (size_t)0, 4}},
                             {{out, n * es, es}}))
        return rc;
    ctx->pipe.stream = stream;
    SM_FINISH(ctx, ctx->pipe.delta.emr_apply(*d, out));
}

int smhip_tsv_probe(smhip_ctx* ctx, const float* b, const float* w, int rows, int cols, int Rp, const void* base_out,
                    int base_out_dtype, double lambda, void* out, float* delta_out, void* stream) {
    SM_GUARD(ctx);
    auto bad = [&](const char* what) { return ctx->pipe.fail(SMHIP_ERR_ARG, std::string("tsv_probe: ") + what); };
    if (rows < 1 || cols < 1 || Rp < 0 || Rp > SMHIP_TSV_MAX_R || Rp % 16) return bad("bad shape");
    if (!base_out || !out || (Rp > 0 && (!b || !w))) return bad("null pointer");
    if (base_out_dtype < SMHIP_BF16 || base_out_dtype > SMHIP_F32) return bad("bad dtype");
    const size_t oes = base_out_dtype == SMHIP_F32 ? 4 : 2;
    if ((uintptr_t)b % 4 || (uintptr_t)w % 4 || (uintptr_t)delta_out % 4 || (uintptr_t)base_out % oes || (uintptr_t)out % oes)
        return bad("a pointer is not aligned to its element size");
    ctx->pipe.stream = stream;
    SM_FINISH(ctx, ctx->pipe.delta.tsv_probe(b, w, rows, cols, Rp, base_out, base_out_dtype, lambda, out, delta_out));
}

size_t smhip_iso_workspace(int rows, int cols) {
    if (rows < 1 || cols < 1 || std::min(rows, cols) > SMHIP_ISO_MAX_S) return 0;
    return smhip::DeltaHost<SM_BACKEND>::iso_layout(rows, cols).total;
}

int smhip_iso_merge(smhip_ctx* ctx, const smhip_iso_desc* d, void* out, float* delta_out, smhip_iso_report* report, void* stream) {
    SM_GUARD(ctx);
    if (int rc = delta_tensor_check(ctx, "iso_merge", d, out, delta_out, true, [&]() -> const char* {
            if (!std::isfinite(d->lambda)) return "lambda is not finite";
            if (!(d->tol > 0.0 && d->tol <= 1.0)) return "tol must be in (0, 1]";
            if (d->max_iter < 0 || d->max_iter > SMHIP_ISO_MAX_ITER) return "max_iter out of range (0..200)";
            return nullptr;
        }))
        return rc;
    auto bad = [&](const char* what) { return ctx->pipe.fail(SMHIP_ERR_ARG, std::string("iso_merge: ") + what); };
    if (d->n > 0) {
        if (d->rows < 1 || d->cols < 1 || (size_t)d->rows * (size_t)d->cols != d->n) return bad("rows and cols must be >= 1 and rows * cols == n");
        if (std::min(d->rows, d->cols) > SMHIP_ISO_MAX_S) return bad("min(rows, cols) exceeds 16384");
        if (d->n / smhip::GEO_SEG_ELEMS > (size_t)1 << 30) return bad("tensor too large");
        if (!d->workspace || (uintptr_t)d->workspace % 256 || d->workspace_bytes < smhip_iso_workspace(d->rows, d->cols))
            return bad("the workspace is null, not 256-byte aligned or too small (smhip_iso_workspace)");
    }
    ctx->pipe.stream = stream;
    SM_FINISH(ctx, ctx->pipe.delta.iso_merge(*d, out, delta_out, report));
}

int smhip_iso_gemm(smhip_ctx* ctx, const smhip_iso_gemm_desc* d, void* stream) {
    SM_GUARD(ctx);
    auto bad = [&](const char* what) { return ctx->pipe.fail(SMHIP_ERR_ARG, std::string("iso_gemm: ") + what); };
    if (!d) return bad("null descriptor");
    if (d->form != 0 && d->form != 1) return bad("bad form");
    if (d->epilogue < 0 || d->epilogue > 3) return bad("bad epilogue");
    if (d->M < 1 || d->N < 1 || d->K < 1 || d->M > (1 << 24) || d->N > (1 << 24)) return bad("bad shape");
    if (d->sym != 0 && d->sym != 1) return bad("sym must be 0 or 1");
    if (d->sym && (d->form != 0 || d->M != d->N)) return bad("sym needs the NT form and M == N");
    if (!d->a || !d->b || !d->c || (d->epilogue && !d->e)) return bad("null pointer");
    if ((uintptr_t)d->a % 4 || (uintptr_t)d->b % 4 || (uintptr_t)d->c % 4 || (uintptr_t)d->e % 4)
        return bad("a pointer is not aligned to its element size");
    if (d->lda < d->K || d->ldb < (d->form == 0 ? d->K : d->N) || d->ldc < d->N || (d->epilogue && d->lde < d->N))
        return bad("a pitch is shorter than its row");
    const int gm = (d->M + 127) / 128, gn = (d->N + 127) / 128;
    if ((long long)gm * gn > 0x7fffffffLL) return bad("bad shape");
    auto span = [](const float* p, int rows, int ld, int cols) { return std::make_pair((uintptr_t)p, (uintptr_t)(p + (size_t)(rows - 1) * ld + cols)); };
    const auto sc = span(d->c, d->M, d->ldc, d->N);
    auto hits = [&](std::pair<uintptr_t, uintptr_t> x) { return x.first < sc.second && sc.first < x.second; };
    if (hits(span(d->a, d->M, d->lda, d->K)) || hits(d->form == 0 ? span(d->b, d->N, d->ldb, d->K) : span(d->b, d->K, d->ldb, d->N)) ||
        (d->epilogue && hits(span(d->e, d->M, d->lde, d->N))))
        return bad("c overlaps an input");
    ctx->pipe.stream = stream;
    SM_FINISH(ctx, ctx->pipe.delta.iso_gemm_probe(*d));
}

int smhip_exact_norm(smhip_ctx* ctx, const void* x, int dtype, size_t n, double* norm_out, void* stream) {
    SM_GUARD(ctx);
    if (!norm_out || (n > 0 && !x)) return ctx->pipe.fail(SMHIP_ERR_ARG, "bad argument");
    if (dtype < SMHIP_BF16 || dtype > SMHIP_F32) return ctx->pipe.fail(SMHIP_ERR_ARG, "bad dtype");
    ctx->pipe.stream = stream;
    SM_FINISH(ctx, ctx->pipe.fn_exact_norm(x, dtype, n, norm_out));
}

int smhip_correlate_pairs(smhip_ctx* ctx, int k, const void* const* tensors, int dtype, size_t rows, size_t cols,
                          float* matrix_out, void* stream) {
    SM_GUARD(ctx);
    if (!tensors || !matrix_out || rows < 1 || cols < 1) return ctx->pipe.fail(SMHIP_ERR_ARG, "bad argument");
    if (dtype < SMHIP_BF16 || dtype > SMHIP_F32) return ctx->pipe.fail(SMHIP_ERR_ARG, "bad dtype");
    for (int i = 0; i < k && i < 8; ++i)
        if (!tensors[i]) return ctx->pipe.fail(SMHIP_ERR_ARG, "null tensor");
    ctx->pipe.stream = stream;
    SM_FINISH(ctx, ctx->pipe.correlate_pairs(k, tensors, dtype, rows, cols, matrix_out));
}

int smhip_reference_cpu_norm(smhip_ctx* ctx, const void* x, const void* base, int dtype, size_t n, float* norm_out,
                             void* stream) {
    SM_GUARD(ctx);
    if (!x || !norm_out) return ctx->pipe.fail(SMHIP_ERR_ARG, "bad argument");
    if (dtype < SMHIP_BF16 || dtype > SMHIP_F32) return ctx->pipe.fail(SMHIP_ERR_ARG, "bad dtype");
    ctx->pipe.stream = stream;
    const int rc0 = ctx->pipe.reserve(1, 1);
    if (rc0) SM_FINISH(ctx, rc0);
    smhip::SigDesc sg{x, base, dtype, 1.f};
    double out = 0;
    if (!ctx->pipe.run_serial_norms(&sg, 1, n, &out))
        return ctx->pipe.fail(SMHIP_ERR_ARG, "reference_cpu norm: inputs must be 16-byte aligned");
    *norm_out = (float)out;
    SM_FINISH(ctx, SMHIP_OK);
}

int smhip_debug_option(smhip_ctx* ctx, const char* key, long value) {
    SM_GUARD(ctx);
    if (key && std::string(key) == "aten_overlap") { ctx->pipe.aten_overlap = value != 0; return SMHIP_OK; }
    if (key && std::string(key) == "emf_max_sample") { ctx->pipe.emf_max_sample = value >= 1 && value <= 4096 ? (int)value : smhip::EMF_MAX_SAMPLE; return SMHIP_OK; }
    if (key && std::string(key) == "aten_serial") { ctx->pipe.aten_serial = value != 0; return SMHIP_OK; }
    if (key && std::string(key) == "class_norms") { ctx->pipe.class_norms_mode = value >= 0 && value <= 2 ? (int)value : 1; return SMHIP_OK; }
    if (key && std::string(key) == "cand_cap") { ctx->pipe.debug_cand_cap = value > 0 ? (uint32_t)value : 0u; return SMHIP_OK; }
    if (key && std::string(key) == "sel_chunks") { ctx->pipe.debug_sel_chunks = value > 0 ? (uint32_t)value : 0u; return SMHIP_OK; }
    if (key && std::string(key) == "sel_flush_always") { ctx->pipe.debug_flush_always = value != 0; return SMHIP_OK; }
    if (key && std::string(key) == "fuse_norms") { ctx->pipe.fuse_norms = value != 0; return SMHIP_OK; }
    if (key && std::string(key) == "noise_seed") { ctx->pipe.noise_seed_base = (uint32_t)value; return SMHIP_OK; }
    if (key && std::string(key) == "spectral_intermediates") { ctx->pipe.spectral_inter = value != 0; return SMHIP_OK; }
    if (key && std::string(key) == "fuse_spec_norm") { ctx->pipe.fuse_spec_norm = value != 0; return SMHIP_OK; }
    if (key && std::string(key) == "sel_wgs_per_cu") { ctx->pipe.sel_wgs_per_cu = value > 0 ? (int)value : 5; return SMHIP_OK; }
    if (key && std::string(key) == "pair1d") { ctx->pipe.pair1d_enabled = value != 0; return SMHIP_OK; }
    if (key && std::string(key) == "spec_cull") { ctx->pipe.spec_cull = value != 0; return SMHIP_OK; }
    if (key && std::string(key) == "spec_min_bins") { ctx->pipe.spec_min_bins = value >= 0 ? (size_t)value : (size_t)1 << 20; return SMHIP_OK; }
    if (key && std::string(key) == "dftp_pairs") { ctx->pipe.dftp_pairs_enabled = value != 0; return SMHIP_OK; }
    if (key && std::string(key) == "f2s_pair") { ctx->pipe.f2s_pair = value != 0; return SMHIP_OK; }
    if (key && std::string(key) == "f1_multi") { ctx->pipe.f1_multi = value != 0; return SMHIP_OK; }
    if (key && std::string(key) == "force_bluestein") { ctx->pipe.debug_force_bluestein = value != 0; return SMHIP_OK; }
    if (key && std::string(key) == "force_split") { ctx->pipe.debug_force_split = value > 1 && value <= smhip::DFTP_MAX_P ? (int)value : 0; return SMHIP_OK; }
    if (key && std::string(key) == "fold_columns") { ctx->pipe.fold_enabled = value != 0; return SMHIP_OK; }
    if (key && std::string(key) == "della_slab_rows") { ctx->pipe.delta.della_slab_rows = value > 0 ? (size_t)value : 0; return SMHIP_OK; }
    if (key && std::string(key) == "emr_fused_geo_fold") { ctx->pipe.delta.emr_fused_geo_fold = value != 0; return SMHIP_OK; }
    if (key && std::string(key) == "fold_min_rows") { ctx->pipe.fold_min_rows = value > 0 ? (int)value : SM_FOLD_MIN_ROWS; return SMHIP_OK; }
    return ctx->pipe.fail(SMHIP_ERR_ARG, "unknown debug option");
}

int smhip_debug_query(smhip_ctx* ctx, const char* key, long* value) {
    SM_GUARD(ctx);
    if (!key || !value) return SMHIP_ERR_ARG;
    if (std::string(key) == "spec_hit") { *value = ctx->pipe.last_spec_verdict(); SM_FINISH(ctx, SMHIP_OK); }
    if (std::string(key) == "spec_checked" || std::string(key) == "spec_hits") {
        unsigned long long c = 0, h = 0;
        ctx->pipe.spec_totals(&c, &h);
        *value = (long)(std::string(key) == "spec_hits" ? h : c);
        SM_FINISH(ctx, SMHIP_OK);
    }
    if (std::string(key) == "aten_fast" || std::string(key) == "aten_group" || std::string(key) == "aten_slow") {
        unsigned long long v3[3];
        ctx->pipe.aten_stats(1, v3);
        *value = (long)v3[std::string(key) == "aten_fast" ? 0 : std::string(key) == "aten_group" ? 1 : 2];
        SM_FINISH(ctx, SMHIP_OK);
    }
    if (std::string(key) == "eig_host_us") { *value = (long)ctx->pipe.delta.eig_host_us; SM_FINISH(ctx, SMHIP_OK); }
    return ctx->pipe.fail(SMHIP_ERR_ARG, "unknown debug query");
}

int smhip_profile_enable(smhip_ctx* ctx, int on) { SM_GUARD(ctx); ctx->pipe.be.profile_enable(on != 0); return SMHIP_OK; }
int smhip_profile_reset(smhip_ctx* ctx) { SM_GUARD(ctx); ctx->pipe.be.profile_reset(); return SMHIP_OK; }
int smhip_profile_count(smhip_ctx* ctx) { return ctx ? ctx->pipe.be.profile_count() : 0; }
int smhip_profile_get(smhip_ctx* ctx, int i, const char** name, uint64_t* launches, double* total_ms) {
    SM_GUARD(ctx);
    return ctx->pipe.be.profile_get(i, name, launches, total_ms) ? SMHIP_OK : SMHIP_ERR_ARG;
}

}  // extern "C"
