// sm_dpack.hpp - the delta pack: a finetune as one or two bit planes and a scale per row (or per tensor) on top of its
// base - 1 bit: the sign of every delta (BitDelta, Liu et al. 2024); 2 bits: a mask of the largest magnitudes and their
// signs (ComPEFT, Yadav et al. 2023; both as recalled: PAPERS.md).  Not a merge operator: a second REPRESENTATION of a
// finetune next to the LoRA adapter, which every operator takes through dpack_apply.  The functions are stated in
// include/shardmerge_hip.h (smhip_dpack_pack, smhip_dpack_apply); every step of them is an exact order statistic, an
// integer function or one correctly rounded operation, so the kernels equal a plain restatement bit for bit.
//
//   dpack_pack    the fused pass.  A work-group works on whole rows; a lane takes the row's octets tid, tid + 256, ...
//                 (the order of geo_gram's row-wise sums), forms the 8 deltas in registers, applies the keep test (the
//                 threshold is ties_select's, on the device) and writes one byte per octet and plane: a wave writes 64
//                 contiguous bytes.  Three fp64 accumulators and two integer counters per lane, reduced by the fixed
//                 binary tree in LDS (the counters as fp64 too: integers below 2^53 add exactly in any order), one
//                 partial [A, Q, Z, c, nonzero] per row.
//   dpack_scale   a thread per row: the scale, the row's residual and energy terms.
//   the folds     geo_gram_fold over the rows' partials and terms: rows added in index order.
//   dpack_apply   the streaming pass: a 16-byte run of base, one byte of each plane, the row's scale, a 16-byte store.
#pragma once
#include "sm_geo.hpp"

namespace smhip {

constexpr int DPACK_THREADS = 256;                // work-group of dpack_pack: the tree needs a power of two
constexpr int DPACK_NP = 5;                       // a row's partial: A, Q, Z, c, nonzero
constexpr int DPACK_NT = 2;                       // a row's terms: Z + e, Q + Z
enum { DPACK_ROW = 0, DPACK_TENSOR = 1 };

struct DpackPackParams {
    const void* ft; const void* base; int dtype;
    size_t R, C, PB;            // rows, columns, bytes per row of a plane: ceil(C / 8)
    int bits;                   // 1: every element is kept; 2: kept iff |d| >= tau and d != 0
    const float* threshold;     // bits == 2: [1], device (ties_select's)
    uint8_t* sign;              // [R][PB]
    uint8_t* mask;              // [R][PB], bits == 2
    int row_vec;                // C % 8 == 0 and ft, base are 16-byte aligned: every octet is a 16-byte access
    double* part;               // [R][DPACK_NP]
    uint32_t* flags;            // [0]: bit 0 = the delta holds a NaN or an Inf
};
SM_HD size_t dpack_pack_lds_floats() { return LDS_SCRATCH_FLOATS + (size_t)2 * DPACK_NP * DPACK_THREADS; }

template <class Ex>
SM_HD void k_dpack_pack(Ex& ex, const DpackPackParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const int nt = ex.nthreads();                                  // DPACK_THREADS
    double* red = (double*)(ex.lds() + LDS_SCRATCH_FLOATS);        // [DPACK_NP][nt]
    const uint32_t tau = p.bits == 2 ? f2u(*p.threshold) : 0u;
    for (size_t r = (size_t)ex.bid(); r < p.R; r += (size_t)ex.nblocks()) {
        const size_t start = r * p.C;
        ex.each(st, [&](int tid, EmptyState&) {
            double A = 0.0, Q = 0.0, Z = 0.0;
            unsigned long long c = 0, nz = 0;
            uint32_t bad = 0;
            for (size_t q = tid; q < p.PB; q += nt) {
                const Octet o = segment_octet(start, p.C, p.row_vec, q);
                float b[8], f[8];
                ties_load8(p.base, p.dtype, o.i0, o.cnt, o.vec, b);
                ties_load8(p.ft, p.dtype, o.i0, o.cnt, o.vec, f);
                uint32_t sb = 0, mb = 0;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float d = f[e] - b[e];                   // (an element past the row's end: +0 - +0)
                    const uint32_t key = delta_key(d);
                    if (key >= TIES_KEY_INF) bad = 1u;
                    const bool in = e < o.cnt;
                    const bool kept = in && (p.bits == 1 || (key >= tau && key != 0u));
                    // (the product of two fp32 values is exact in fp64: fused or not, ONE rounded addition each)
                    const double dd = (double)d * (double)d;
                    A = A + (kept ? (double)fabsf(d) : 0.0);
                    Q = Q + (kept ? dd : 0.0);
                    Z = Z + (kept ? 0.0 : dd);
                    c += kept ? 1u : 0u;
                    nz += (in && key != 0u) ? 1u : 0u;
                    mb |= kept ? 1u << e : 0u;
                    sb |= (kept && d < 0.f) ? 1u << e : 0u;
                }
                p.sign[r * p.PB + q] = (uint8_t)sb;
                if (p.bits == 2) p.mask[r * p.PB + q] = (uint8_t)mb;
            }
            red[0 * nt + tid] = A; red[1 * nt + tid] = Q; red[2 * nt + tid] = Z;
            red[3 * nt + tid] = (double)c; red[4 * nt + tid] = (double)nz;
            if (bad) ex.global_atomic_or_u32(p.flags, bad);
        });
        ex.sync();
        // the fixed binary tree of geo_gram: v[t] = v[t] + v[t + s] for t < s, s = nt / 2, nt / 4, ..., 1
        for (int s = nt >> 1; s > 0; s >>= 1) {
            ex.each(st, [&](int tid, EmptyState&) {
                if (tid >= s) return;
#pragma unroll
                for (int j = 0; j < DPACK_NP; ++j) {
                    double* v = red + j * nt;
                    v[tid] = v[tid] + v[tid + s];
                }
            });
            ex.sync();
        }
        ex.each(st, [&](int tid, EmptyState&) {
            if (tid < DPACK_NP) p.part[r * DPACK_NP + tid] = red[tid * nt];
        });
        ex.sync();                                                  // (the next row's lanes write red)
    }
}

// the scale and the residual of one row (or of the totals): s = fp32(A / c), +0 when c == 0;
// e = max((Q - 2 (s A)) + c (s s), 0), one rounded fp64 operation at a time
SM_HD float dpack_scale_of(double A, double c) { return c == 0.0 ? 0.f : (float)geo_ddiv(A, c); }
SM_HD double dpack_resid_of(double A, double Q, double c, float s32) {
    const double s = (double)s32;
    const double e = geo_dadd(geo_dadd(Q, -geo_dmul(2.0, geo_dmul(s, A))), geo_dmul(c, geo_dmul(s, s)));
    return e > 0.0 ? e : 0.0;
}

struct DpackScaleParams {
    size_t rows;                // R, or 1: the row of the totals (scale_mode TENSOR)
    const double* part;         // [rows][DPACK_NP]
    float* scale;               // [rows]
    double* terms;              // [rows][DPACK_NT]: Z + e, Q + Z
};
template <class Ex>
SM_HD void k_dpack_scale(Ex& ex, const DpackScaleParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    ex.each(st, [&](int tid, EmptyState&) {
        const size_t r = (size_t)ex.bid() * ex.nthreads() + tid;
        if (r >= p.rows) return;
        const double* g = p.part + r * DPACK_NP;
        const float s = dpack_scale_of(g[0], g[3]);
        p.scale[r] = s;
        p.terms[r * DPACK_NT] = geo_dadd(g[2], dpack_resid_of(g[0], g[1], g[3], s));
        p.terms[r * DPACK_NT + 1] = geo_dadd(g[1], g[2]);
    });
}

struct DpackApplyParams {
    const void* base; int dtype;
    size_t R, C, PB;
    size_t units;               // R * PB row octets
    const uint8_t* sign;        // [R][PB]
    const uint8_t* mask;        // [R][PB], or null: every element is kept
    const float* scale;         // [R] (DPACK_ROW) or [1]
    int scale_mode;
    void* out;                  // dtype, [R][C]
    int row_vec;                // C % 8 == 0 and base, out are 16-byte aligned
    int chunks;                 // row octets per thread
};
// element e of an octet: its raw bits w (a 16-bit type in the low half) pass through unless kept
SM_HD uint32_t dpack_apply_elem(uint32_t w, int dtype, bool kept, float s) {
    if (!kept) return w;
    const float b = dtype == DT_F32 ? u2f(w) : (dtype == DT_BF16 ? bf16_to_f(w) : f16_to_f(w));
    const float r = aten_fadd_(b, s);
    return dtype == DT_F32 ? f2u(r) : (uint32_t)(dtype == DT_BF16 ? f_to_bf16_any(r) : f_to_f16_any(r));
}
template <class Ex>
SM_HD void k_dpack_apply(Ex& ex, const DpackApplyParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const int nt = ex.nthreads();
    ex.each(st, [&](int tid, EmptyState&) {
        for (int q = 0; q < p.chunks; ++q) {
            const size_t u = ((size_t)ex.bid() * p.chunks + q) * nt + tid;
            if (u >= p.units) break;
            const size_t r = p.units <= 0xffffffffull ? (size_t)((uint32_t)u / (uint32_t)p.PB) : u / p.PB, o = u - r * p.PB;
            const size_t c0 = 8 * o, i0 = r * p.C + c0;
            const int cnt = (int)((p.C - c0) < 8 ? (p.C - c0) : 8);
            const uint32_t sb = p.sign[u], mb = p.mask ? p.mask[u] : 0xffu;
            const float s = p.scale[p.scale_mode == DPACK_ROW ? r : 0];
            if (p.row_vec) {
                if (p.dtype == DT_F32) {
                    const u32x4 a = ((const u32x4*)p.base)[i0 / 4], b = ((const u32x4*)p.base)[i0 / 4 + 1];
                    uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
                    for (int e = 0; e < 8; ++e) w[e] = dpack_apply_elem(w[e], DT_F32, (mb >> e) & 1u, ((sb >> e) & 1u) ? -s : s);
                    ((u32x4*)p.out)[i0 / 4] = u32x4{w[0], w[1], w[2], w[3]};
                    ((u32x4*)p.out)[i0 / 4 + 1] = u32x4{w[4], w[5], w[6], w[7]};
                } else {
                    const u32x4 a = ((const u32x4*)p.base)[i0 / 8];
                    const uint32_t h[4] = {a.x, a.y, a.z, a.w};
                    uint32_t w[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e)
                        w[e] = dpack_apply_elem((h[e >> 1] >> (16 * (e & 1))) & 0xffffu, p.dtype, (mb >> e) & 1u, ((sb >> e) & 1u) ? -s : s);
                    ((u32x4*)p.out)[i0 / 8] = u32x4{w[0] | (w[1] << 16), w[2] | (w[3] << 16), w[4] | (w[5] << 16), w[6] | (w[7] << 16)};
                }
            } else {                                                // a row octet that starts anywhere: element by element
                for (int e = 0; e < cnt; ++e) {
                    const bool kept = (mb >> e) & 1u;
                    const float se = ((sb >> e) & 1u) ? -s : s;
                    if (p.dtype == DT_F32) ((uint32_t*)p.out)[i0 + e] = dpack_apply_elem(((const uint32_t*)p.base)[i0 + e], DT_F32, kept, se);
                    else ((uint16_t*)p.out)[i0 + e] = (uint16_t)dpack_apply_elem(((const uint16_t*)p.base)[i0 + e], p.dtype, kept, se);
                }
            }
        }
    });
}

// ---- kernel tags (sm_tag.hpp) and group 16 of smhip_side.hip (smhip_device.hpp) ----
// the fused pass over whole rows (planes, ordered fp64 sums), the scales, the streaming apply; its selection is
// ties_hist / ties_select and its folds are geo_gram_fold
SM_KERNEL_TAG_LB(KDpackPack, DpackPackParams, "dpack_pack", k_dpack_pack(ex, p), DPACK_THREADS, 4)
SM_KERNEL_TAG_LB(KDpackScale, DpackScaleParams, "dpack_scale", k_dpack_scale(ex, p), 256, 4)
SM_KERNEL_TAG_LB(KDpackApply, DpackApplyParams, "dpack_apply", k_dpack_apply(ex, p), 256, 4)
#define SM_SIDE_KERNELS_16(X) X(KDpackPack) X(KDpackScale) X(KDpackApply)

}  // namespace smhip
