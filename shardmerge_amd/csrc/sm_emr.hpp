// sm_emr.hpp - EMR-Merging (Huang et al., NeurIPS 2024, "EMR-Merging: Tuning-Free High-Performance Model Merging"; as
// recalled: PAPERS.md), an operator the reference does not have: ONE elected task vector for all tasks, and per task a
// 1-bit mask and one rescaler that recover a model for that task.  The functions are stated in include/shardmerge_hip.h
// (smhip_emr_merge, smhip_emr_mask, smhip_emr_apply); every step of them is one correctly rounded operation, a
// comparison or an integer count, so the kernels equal a plain restatement of them bit for bit.
//
//   emr_merge   the one fused streaming pass of the unified model.  "Elect" is the sign election of the other delta
//               merges with max in place of the sum: the k deltas of an octet stay in registers between the sum that
//               elects the sign and the sweep that takes the largest agreeing magnitude - the finetunes are read once.
//               KR = 4 serves k <= 4 (32 registers of deltas), KR = 16 any k (128), the same source.  Counters:
//               agree[i] and winner[i] a slot per (finetune, thread) in LDS folded by kept_fold; the four element
//               classes in per-thread registers, added to a work-group's LDS totals; one 64-bit global atomic per
//               counter and work-group.
//   emr_mask    a task's modulator from (finetune, base, unified): dpack_pack's walk over whole rows - lane tid takes
//               octets tid, tid + 256, ..., one plane byte per octet, seven fp64 partials per row through the fixed
//               binary tree - with the agreement of two deltas' signs as the keep test.  The rows are folded by
//               geo_gram_fold; the rescaler and the residual are a handful of fp64 operations on the host.
//   emr_apply   the streaming pass: a 16-byte run of base and of unified, one plane byte, a 16-byte store.
#pragma once
#include "sm_geo.hpp"

namespace smhip {

constexpr int EMR_REG_SMALL = 4;                  // k <= 4: the instantiation with four deltas per element in registers
enum { EMR_POS = 0, EMR_NEG = 1, EMR_ZERO = 2, EMR_CONTESTED = 3, EMR_COUNTS = 4 };
constexpr int EMR_THREADS = 256;                  // work-group of emr_mask: the tree needs a power of two
constexpr int EMR_NP = 7;                         // a row's partial: A, B, D2, X, U2, c, nonzero

struct EmrMergeParams {
    TiesInputs in;
    const void* base_out; int base_out_dtype;
    int out_is_base0;           // base_out is base[0] in the same dtype and the bases are shared: loaded once
    float lambda;
    void* out;                  // base_out_dtype, [n]
    float* delta_out;           // optional fp32 [n]: lambda * tau
    unsigned long long* agree;  // [k], device: elements where d_i != 0 has the elected sign
    unsigned long long* winner; // [k], device: elements whose tau is d_i (the first i that attains the maximum)
    unsigned long long* counts; // [EMR_COUNTS], device: elected plus / minus, zero, contested
    uint32_t* flags;            // [0]: bit i = finetune i has a non-finite delta; [1]: bit 0 = a non-finite sum
    int chunks;                 // octets per thread
};
// dynamic LDS beyond the scratch: dare_lds_words of agree counters, as many of winner counters, the EMR_COUNTS totals
SM_HD size_t emr_lds_words(int k, int nthreads) { return 2 * dare_lds_words(k, nthreads) + EMR_COUNTS; }

template <int KR, class Ex>
SM_HD void k_emr_merge(Ex& ex, const EmrMergeParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const int nt = ex.nthreads();
    const int k = p.in.k;
    uint32_t* la = (uint32_t*)(ex.lds() + LDS_SCRATCH_FLOATS);     // agree: [k][nt], then the totals (dare_lds_words)
    uint32_t* lw = la + dare_lds_words(k, nt);                     // winner: the same
    uint32_t* tc = lw + dare_lds_words(k, nt);                     // [EMR_COUNTS]
    ex.each(st, [&](int tid, EmptyState&) { if (tid < EMR_COUNTS) tc[tid] = 0; });
    kept_zero(ex, st, la, k);
    kept_zero(ex, st, lw, k);                                      // (ends with the barrier)
    ex.each(st, [&](int tid, EmptyState&) {
        uint32_t bad = 0, bad_sum = 0, cls[EMR_COUNTS] = {0u, 0u, 0u, 0u};
        for (int q = 0; q < p.chunks; ++q) {
            Octet o;
            if (!octet_at(p.in, ex.bid(), nt, p.chunks, tid, q, o)) break;
            float d[KR][8], b[8], bo[8], S[8];
            delta_base8(p.in, o, b);
            delta_base_out8(p, o, b, bo);
#pragma unroll
            for (int e = 0; e < 8; ++e) S[e] = 0.f;
            // sweep one: the deltas (kept in d) and their sum
#pragma unroll
            for (int i = 0; i < KR; ++i) {
                if (i < k) {
                    float f[8];
                    delta_load8(p.in, i, o, b, f);
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float de = f[e] - b[e];
                        if (delta_key(de) >= TIES_KEY_INF) bad |= 1u << i;
                        S[e] = aten_fadd_(S[e], de);
                        d[i][e] = de;
                    }
                }
            }
            // sweep two, out of registers: the largest magnitude among the entries of the elected sign, its first owner
            float eps[8];
            int w[8];
            uint32_t seen[8];                                      // bit 0: an entry > 0, bit 1: an entry < 0
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                eps[e] = 0.f; w[e] = -1; seen[e] = 0u;
                if (delta_key(S[e]) >= TIES_KEY_INF) bad_sum = 1u;
            }
#pragma unroll
            for (int i = 0; i < KR; ++i) {
                if (i < k) {
                    uint32_t na = 0;
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float de = d[i][e];
                        const bool pos = S[e] >= 0.f;
                        const bool cand = pos ? de > 0.f : de < 0.f;
                        const float mag = fabsf(de);
                        if (cand && mag > eps[e]) { eps[e] = mag; w[e] = i; }
                        seen[e] |= (de > 0.f ? 1u : 0u) | (de < 0.f ? 2u : 0u);
                        na += (cand && e >= o.lo && e < o.cnt) ? 1u : 0u;
                    }
                    la[i * nt + tid] += na;                        // this thread's own slot
                }
            }
#pragma unroll
            for (int i = 0; i < KR; ++i) {
                if (i < k) {
                    uint32_t nw = 0;
#pragma unroll
                    for (int e = 0; e < 8; ++e) nw += (w[e] == i && e >= o.lo && e < o.cnt) ? 1u : 0u;
                    lw[i * nt + tid] += nw;
                }
            }
            float r[8], dl[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const bool pos = S[e] >= 0.f, zero = eps[e] == 0.f;
                const float tau = zero ? 0.f : (pos ? eps[e] : -eps[e]);
                dl[e] = aten_fmul_(p.lambda, tau);
                r[e] = aten_fadd_(bo[e], dl[e]);
                if (e >= o.lo && e < o.cnt) {
                    cls[zero ? EMR_ZERO : (pos ? EMR_POS : EMR_NEG)] += 1u;
                    cls[EMR_CONTESTED] += seen[e] == 3u ? 1u : 0u;
                }
            }
            delta_store8(p, o, r, dl);
        }
#pragma unroll
        for (int c = 0; c < EMR_COUNTS; ++c)
            if (cls[c]) ex.lds_atomic_add(&tc[c], cls[c]);
        if (bad) ex.global_atomic_or_u32(p.flags, bad);
        if (bad_sum) ex.global_atomic_or_u32(p.flags + 1, bad_sum);
    });
    kept_fold(ex, st, la, k, p.agree);                             // (starts with the barrier the totals in tc need too)
    kept_fold(ex, st, lw, k, p.winner);
    ex.each(st, [&](int tid, EmptyState&) {
        if (tid < EMR_COUNTS && tc[tid]) ex.global_atomic_add(&p.counts[tid], (unsigned long long)tc[tid]);
    });
}

struct EmrMaskParams {
    const void* ft; const void* base; const void* uni; int dtype;
    size_t R, C, PB;            // rows, columns, bytes per row of the plane: ceil(C / 8)
    uint8_t* mask;              // [R][PB]
    int row_vec;                // C % 8 == 0 and ft, base, uni are 16-byte aligned: every octet is a 16-byte access
    double* part;               // [R][EMR_NP]
    uint32_t* flags;            // [0]: bit 0 = finetune - base holds a NaN or an Inf, bit 1 = unified - base does
};
SM_HD size_t emr_mask_lds_floats() { return LDS_SCRATCH_FLOATS + (size_t)2 * EMR_NP * EMR_THREADS; }

template <class Ex>
SM_HD void k_emr_mask(Ex& ex, const EmrMaskParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const int nt = ex.nthreads();                                  // EMR_THREADS
    double* red = (double*)(ex.lds() + LDS_SCRATCH_FLOATS);        // [EMR_NP][nt]
    for (size_t r = (size_t)ex.bid(); r < p.R; r += (size_t)ex.nblocks()) {
        const size_t start = r * p.C;
        ex.each(st, [&](int tid, EmptyState&) {
            double A = 0.0, B = 0.0, D2 = 0.0, X = 0.0, U2 = 0.0;
            unsigned long long c = 0, nz = 0;
            uint32_t bad = 0;
            for (size_t q = tid; q < p.PB; q += nt) {
                const Octet o = segment_octet(start, p.C, p.row_vec, q);
                float b[8], f[8], g[8];
                ties_load8(p.base, p.dtype, o.i0, o.cnt, o.vec, b);
                ties_load8(p.ft, p.dtype, o.i0, o.cnt, o.vec, f);
                ties_load8(p.uni, p.dtype, o.i0, o.cnt, o.vec, g);
                uint32_t mb = 0;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float d = f[e] - b[e], u = g[e] - b[e];  // (an element past the row's end: +0 - +0)
                    if (delta_key(d) >= TIES_KEY_INF) bad |= 1u;
                    if (delta_key(u) >= TIES_KEY_INF) bad |= 2u;
                    const bool m = (d > 0.f && u > 0.f) || (d < 0.f && u < 0.f);
                    // (the product of two fp32 values is exact in fp64: fused or not, ONE rounded addition each)
                    const double dd = (double)d, du = (double)u;
                    A = A + (double)fabsf(d);
                    B = B + (m ? (double)fabsf(u) : 0.0);
                    D2 = D2 + dd * dd;
                    X = X + (m ? dd * du : 0.0);
                    U2 = U2 + (m ? du * du : 0.0);
                    c += m ? 1u : 0u;
                    nz += (e < o.cnt && delta_key(d) != 0u) ? 1u : 0u;
                    mb |= m ? 1u << e : 0u;
                }
                p.mask[r * p.PB + q] = (uint8_t)mb;
            }
            red[0 * nt + tid] = A; red[1 * nt + tid] = B; red[2 * nt + tid] = D2; red[3 * nt + tid] = X;
            red[4 * nt + tid] = U2; red[5 * nt + tid] = (double)c; red[6 * nt + tid] = (double)nz;
            if (bad) ex.global_atomic_or_u32(p.flags, bad);
        });
        ex.sync();
        // the fixed binary tree of geo_gram: v[t] = v[t] + v[t + s] for t < s, s = nt / 2, nt / 4, ..., 1
        for (int s = nt >> 1; s > 0; s >>= 1) {
            ex.each(st, [&](int tid, EmptyState&) {
                if (tid >= s) return;
#pragma unroll
                for (int j = 0; j < EMR_NP; ++j) {
                    double* v = red + j * nt;
                    v[tid] = v[tid] + v[tid + s];
                }
            });
            ex.sync();
        }
        ex.each(st, [&](int tid, EmptyState&) {
            if (tid < EMR_NP) p.part[r * EMR_NP + tid] = red[tid * nt];
        });
        ex.sync();                                                  // (the next row's lanes write red)
    }
}

// the rescaler and the residual of the totals: lambda = fp32(A / B), +0 when B == 0;
// resid_sq = max((D2 - 2 (lambda X)) + (lambda lambda) U2, 0), one rounded fp64 operation at a time
SM_HD float emr_scale_of(double A, double B) { return B == 0.0 ? 0.f : (float)geo_ddiv(A, B); }
SM_HD double emr_resid_of(double D2, double X, double U2, float l32) {
    const double l = (double)l32;
    const double e = geo_dadd(geo_dadd(D2, -geo_dmul(2.0, geo_dmul(l, X))), geo_dmul(geo_dmul(l, l), U2));
    return e > 0.0 ? e : 0.0;
}

struct EmrApplyParams {
    const void* base; const void* uni; int dtype;
    size_t R, C, PB;
    size_t units;               // R * PB row octets
    const uint8_t* mask;        // [R][PB]
    const float* scale;         // [1]
    void* out;                  // dtype, [R][C]
    int row_vec;                // C % 8 == 0 and base, uni, out are 16-byte aligned
    int chunks;                 // row octets per thread
};
// element e of an octet: the base's raw bits w (a 16-bit type in the low half) pass through unless the mask bit is set;
// then u = U - b, t = lambda * u, b + t rounded once to the dtype (g: the unified model's raw bits)
SM_HD uint32_t emr_apply_elem(uint32_t w, uint32_t g, int dtype, bool set, float l) {
    if (!set) return w;
    const float b = dtype == DT_F32 ? u2f(w) : (dtype == DT_BF16 ? bf16_to_f(w) : f16_to_f(w));
    const float U = dtype == DT_F32 ? u2f(g) : (dtype == DT_BF16 ? bf16_to_f(g) : f16_to_f(g));
    const float r = aten_fadd_(b, aten_fmul_(l, aten_fadd_(U, -b)));
    return dtype == DT_F32 ? f2u(r) : (uint32_t)(dtype == DT_BF16 ? f_to_bf16_any(r) : f_to_f16_any(r));
}
template <class Ex>
SM_HD void k_emr_apply(Ex& ex, const EmrApplyParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const int nt = ex.nthreads();
    ex.each(st, [&](int tid, EmptyState&) {
        const float l = p.scale[0];
        for (int q = 0; q < p.chunks; ++q) {
            const size_t u = ((size_t)ex.bid() * p.chunks + q) * nt + tid;
            if (u >= p.units) break;
            const size_t r = p.units <= 0xffffffffull ? (size_t)((uint32_t)u / (uint32_t)p.PB) : u / p.PB, o = u - r * p.PB;
            const size_t c0 = 8 * o, i0 = r * p.C + c0;
            const int cnt = (int)((p.C - c0) < 8 ? (p.C - c0) : 8);
            const uint32_t mb = p.mask[u];
            if (p.row_vec) {
                if (p.dtype == DT_F32) {
                    const u32x4 a0 = ((const u32x4*)p.base)[i0 / 4], a1 = ((const u32x4*)p.base)[i0 / 4 + 1];
                    const u32x4 g0 = ((const u32x4*)p.uni)[i0 / 4], g1 = ((const u32x4*)p.uni)[i0 / 4 + 1];
                    uint32_t w[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
                    const uint32_t g[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
#pragma unroll
                    for (int e = 0; e < 8; ++e) w[e] = emr_apply_elem(w[e], g[e], DT_F32, (mb >> e) & 1u, l);
                    ((u32x4*)p.out)[i0 / 4] = u32x4{w[0], w[1], w[2], w[3]};
                    ((u32x4*)p.out)[i0 / 4 + 1] = u32x4{w[4], w[5], w[6], w[7]};
                } else {
                    const u32x4 a = ((const u32x4*)p.base)[i0 / 8], gg = ((const u32x4*)p.uni)[i0 / 8];
                    const uint32_t h[4] = {a.x, a.y, a.z, a.w}, g[4] = {gg.x, gg.y, gg.z, gg.w};
                    uint32_t w[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e)
                        w[e] = emr_apply_elem((h[e >> 1] >> (16 * (e & 1))) & 0xffffu, (g[e >> 1] >> (16 * (e & 1))) & 0xffffu,
                                              p.dtype, (mb >> e) & 1u, l);
                    ((u32x4*)p.out)[i0 / 8] = u32x4{w[0] | (w[1] << 16), w[2] | (w[3] << 16), w[4] | (w[5] << 16), w[6] | (w[7] << 16)};
                }
            } else {                                                // a row octet that starts anywhere: element by element
                for (int e = 0; e < cnt; ++e) {
                    const bool set = (mb >> e) & 1u;
                    if (p.dtype == DT_F32)
                        ((uint32_t*)p.out)[i0 + e] = emr_apply_elem(((const uint32_t*)p.base)[i0 + e], ((const uint32_t*)p.uni)[i0 + e], DT_F32, set, l);
                    else
                        ((uint16_t*)p.out)[i0 + e] = (uint16_t)emr_apply_elem(((const uint16_t*)p.base)[i0 + e], ((const uint16_t*)p.uni)[i0 + e], p.dtype, set, l);
                }
            }
        }
    });
}

// ---- kernel tags (sm_tag.hpp) and group 21 of smhip_side.hip (smhip_device.hpp) ----
// the one fused pass with the k deltas of an octet in registers across the sum and the max; k <= 4 at dare_merge's
// residency, or up to 16.  The modulator's pass over whole rows (its folds are geo_gram_fold) and the streaming apply
SM_KERNEL_TAG_LB(KEmrMerge, EmrMergeParams, "emr_merge", k_emr_merge<EMR_REG_SMALL>(ex, p), 256, 4)
SM_KERNEL_TAG_LB(KEmrMergeAny, EmrMergeParams, "emr_merge", k_emr_merge<TIES_MAX_MODELS>(ex, p), 256, 2)
SM_KERNEL_TAG_LB(KEmrMask, EmrMaskParams, "emr_mask", k_emr_mask(ex, p), EMR_THREADS, 4)
SM_KERNEL_TAG_LB(KEmrApply, EmrApplyParams, "emr_apply", k_emr_apply(ex, p), 256, 4)
#define SM_SIDE_KERNELS_21(X) X(KEmrMerge) X(KEmrMergeAny) X(KEmrMask) X(KEmrApply)

}  // namespace smhip
