// sm_emr_fused.hpp - EMR-Merging's unified model AND every task's modulator from one call (smhip_emr_merge_masks,
// include/shardmerge_hip.h): the composition of smhip_emr_merge and, per entry i, smhip_emr_mask(f_i, b_i, out), bit for
// bit.  Every tensor emr_mask reads is on the device during the merge - f_i and b_i are its inputs, the unified tensor
// its output - so the k masks cost k / 8 bytes per element on top of the merge's 2 (k + 2) instead of k (6 + 1 / 8).
//
//   emr_merge_mask  the fused pass, organised by whole rows because the order of emr_mask's fp64 sums is part of its
//                   definition: a work-group of 256 per row, lane tid takes octets tid, tid + 256, ... in ascending
//                   order.  The k deltas of an octet stay in registers across the sum that elects the sign, the largest
//                   agreeing magnitude, the ONE rounding of out (rounded, stored, the rounded bits converted back: g is
//                   what a later reader of out would load) and the k sign comparisons; per octet one 16-byte store of
//                   out, the optional delta_out and one plane byte per task.  The integer counters go emr_merge's way
//                   (slots per (finetune, thread) in LDS folded by kept_fold, the four classes through LDS totals, one
//                   global atomic per counter and work-group), the seven fp64 partials of each task through emr_mask's
//                   fixed tree in LDS into part[r][i][7].
//                   KR = 4 (k <= 4): one sweep, all tasks' sums in registers.  KR = 16: the election sweep writes the
//                   row of out, then the work-group sweeps its row once per group of four tasks (f_i, b_i and out
//                   again: k + 2 + k + (shared base ? 1 : k) + ceil(k / 4) tensor passes).  In those sweeps a lane
//                   loads exactly the octets of out it stored itself in the election sweep - the same walk - so program
//                   order alone makes them visible; no fence and no other lane's store is involved.
//   emr_fold        the ordered fold (((0.0 + part[0]) + part[1]) + ...) of the rows' partials, the bits of
//                   geo_gram_fold without its latency walk: 256 lanes stage EMR_FOLD_ROWS rows of np doubles into LDS
//                   with coalesced loads (the next block's loads are in flight while this block is added), lane t < np
//                   adds its column from LDS in row order and carries the sum across the blocks.
#pragma once
#include "sm_emr.hpp"

namespace smhip {

constexpr int EMR_FUSED_GROUP = 4;                 // tasks whose sums a lane holds at once (and the tree folds at once)
constexpr int EMR_FOLD_ROWS = 64;                  // rows per staged block of emr_fold
constexpr int EMR_FOLD_THREADS = 256;
constexpr int EMR_FOLD_NP_MAX = EMR_NP * TIES_MAX_MODELS;
constexpr int EMR_FOLD_PER = (EMR_FOLD_ROWS * EMR_FOLD_NP_MAX + EMR_FOLD_THREADS - 1) / EMR_FOLD_THREADS;   // doubles a lane stages

struct EmrFusedParams {
    TiesInputs in;              // n = R * C; aligned: every pointer (out, delta_out, base_out included) is 16-byte aligned
    const void* base_out; int base_out_dtype;
    int out_is_base0;
    float lambda;
    void* out;                  // base_out_dtype, [R][C]
    float* delta_out;           // optional fp32 [R][C]
    unsigned long long* agree;  // [k], [k], [EMR_COUNTS]: as EmrMergeParams
    unsigned long long* winner;
    unsigned long long* counts;
    uint32_t* flags;            // [0]: bit i = finetune i has a non-finite delta; [1]: bit 0 = a non-finite sum;
                                // [2]: bit i = out - base_i holds a NaN or an Inf
    size_t R, C, PB;            // rows, columns, bytes per row of a plane: ceil(C / 8)
    int row_vec;                // C % 8 == 0 and in.aligned: every octet is a 16-byte access
    uint8_t* mask[TIES_MAX_MODELS];   // [R][PB] each
    double* part;               // [R][k][EMR_NP]
};
SM_HD int emr_fused_group(int k) { return k < EMR_FUSED_GROUP ? k : EMR_FUSED_GROUP; }
// dynamic LDS in bytes: the scratch, the tree's [group][EMR_NP][nthreads] doubles, emr_merge's counters
SM_HD size_t emr_fused_lds_bytes(int k, int nthreads) {
    return (size_t)LDS_SCRATCH_FLOATS * 4 + (size_t)emr_fused_group(k) * EMR_NP * nthreads * sizeof(double) + emr_lds_words(k, nthreads) * 4;
}

struct EmrSums { double A, B, D2, X, U2; unsigned long long c, nz; };
// one octet of one task into its lane's sums, in emr_mask's words (an element past the row's end is +0 - +0);
// returns the plane byte
SM_HD uint32_t emr_task_octet(const float* d, const float* u, int cnt, EmrSums& s, bool& bad_u) {
    uint32_t mb = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        if (delta_key(u[e]) >= TIES_KEY_INF) bad_u = true;
        const bool m = (d[e] > 0.f && u[e] > 0.f) || (d[e] < 0.f && u[e] < 0.f);
        // (the product of two fp32 values is exact in fp64: fused or not, ONE rounded addition each)
        const double dd = (double)d[e], du = (double)u[e];
        s.A = s.A + (double)fabsf(d[e]);
        s.B = s.B + (m ? (double)fabsf(u[e]) : 0.0);
        s.D2 = s.D2 + dd * dd;
        s.X = s.X + (m ? dd * du : 0.0);
        s.U2 = s.U2 + (m ? du * du : 0.0);
        s.c += m ? 1u : 0u;
        s.nz += (e < cnt && delta_key(d[e]) != 0u) ? 1u : 0u;
        mb |= m ? 1u << e : 0u;
    }
    return mb;
}
SM_HD void emr_sums_to_lds(const EmrSums& s, double* v, int nt, int tid) {      // v: [EMR_NP][nt] of one task
    v[0 * nt + tid] = s.A; v[1 * nt + tid] = s.B; v[2 * nt + tid] = s.D2; v[3 * nt + tid] = s.X;
    v[4 * nt + tid] = s.U2; v[5 * nt + tid] = (double)s.c; v[6 * nt + tid] = (double)s.nz;
}
// the octet of out: r rounded ONCE into base_out's dtype and stored (with the optional delta_out), g = the fp32 value of
// the stored bits.  A row octet that is no 16-byte access goes element by element, as emr_mask reads it
SM_HD void emr_fused_store8(const EmrFusedParams& p, const Octet& o, const float* r, const float* dl, float* g) {
    const int dt = p.base_out_dtype;
    uint32_t h[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        if (dt == DT_F32) { h[e] = f2u(r[e]); g[e] = r[e]; }
        else if (dt == DT_BF16) { h[e] = f_to_bf16_any(r[e]); g[e] = bf16_to_f(h[e]); }
        else { h[e] = f_to_f16_any(r[e]); g[e] = f16_to_f(h[e]); }
    }
    if (o.vec) {
        if (p.delta_out) {
            ((cf4*)p.delta_out)[o.i0 / 4] = cf4{dl[0], dl[1], dl[2], dl[3]};
            ((cf4*)p.delta_out)[o.i0 / 4 + 1] = cf4{dl[4], dl[5], dl[6], dl[7]};
        }
        if (dt == DT_F32) {
            ((u32x4*)p.out)[o.i0 / 4] = u32x4{h[0], h[1], h[2], h[3]};
            ((u32x4*)p.out)[o.i0 / 4 + 1] = u32x4{h[4], h[5], h[6], h[7]};
        } else {
            ((u32x4*)p.out)[o.i0 / 8] = u32x4{h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16)};
        }
    } else {
        for (int e = 0; e < o.cnt; ++e) {
            if (p.delta_out) p.delta_out[o.i0 + e] = dl[e];
            if (dt == DT_F32) ((uint32_t*)p.out)[o.i0 + e] = h[e];
            else ((uint16_t*)p.out)[o.i0 + e] = (uint16_t)h[e];
        }
    }
}

template <int KR, class Ex>
SM_HD void k_emr_merge_mask(Ex& ex, const EmrFusedParams& p) {
    constexpr bool ONE = KR <= EMR_FUSED_GROUP;                    // one sweep: every task's sums beside the deltas
    constexpr int NS = ONE ? KR : 1;
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const int nt = ex.nthreads();                                  // EMR_THREADS
    const int k = p.in.k, G = emr_fused_group(k);
    double* red = (double*)(ex.lds() + LDS_SCRATCH_FLOATS);        // [G][EMR_NP][nt]
    uint32_t* la = (uint32_t*)(red + (size_t)G * EMR_NP * nt);     // agree: [k][nt], then the totals (dare_lds_words)
    uint32_t* lw = la + dare_lds_words(k, nt);                     // winner: the same
    uint32_t* tc = lw + dare_lds_words(k, nt);                     // [EMR_COUNTS]
    ex.each(st, [&](int tid, EmptyState&) { if (tid < EMR_COUNTS) tc[tid] = 0; });
    kept_zero(ex, st, la, k);
    kept_zero(ex, st, lw, k);                                      // (ends with the barrier)
    // the fixed binary tree of emr_mask over the ng tasks in red, then the row's partials of tasks g0 .. g0 + ng - 1
    auto tree = [&](size_t r, int g0, int ng) {
        ex.sync();
        for (int s = nt >> 1; s > 0; s >>= 1) {
            ex.each(st, [&](int tid, EmptyState&) {
                if (tid >= s) return;
                for (int j = 0; j < ng * EMR_NP; ++j) {
                    double* v = red + j * nt;
                    v[tid] = v[tid] + v[tid + s];
                }
            });
            ex.sync();
        }
        ex.each(st, [&](int tid, EmptyState&) {
            if (tid < ng * EMR_NP) p.part[(r * k + g0) * EMR_NP + tid] = red[tid * nt];
        });
        ex.sync();                                                  // (the next sweep's lanes write red)
    };
    for (size_t r = (size_t)ex.bid(); r < p.R; r += (size_t)ex.nblocks()) {
        const size_t start = r * p.C;
        // the election sweep (emr_merge's, over the row's octets)
        ex.each(st, [&](int tid, EmptyState&) {
            uint32_t bad = 0, bad_sum = 0, bad_u = 0, cls[EMR_COUNTS] = {0u, 0u, 0u, 0u};
            EmrSums sums[NS];
#pragma unroll
            for (int i = 0; i < NS; ++i) sums[i] = EmrSums{0.0, 0.0, 0.0, 0.0, 0.0, 0ull, 0ull};
            for (size_t q = tid; q < p.PB; q += nt) {
                const Octet o = segment_octet(start, p.C, p.row_vec, q);
                float d[KR][8], b[8], bo[8], S[8];
                delta_base8(p.in, o, b);
                delta_base_out8(p, o, b, bo);
#pragma unroll
                for (int e = 0; e < 8; ++e) S[e] = 0.f;
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
                float eps[8];
                int w[8];
                uint32_t seen[8];                                  // bit 0: an entry > 0, bit 1: an entry < 0
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
                            na += (cand && e < o.cnt) ? 1u : 0u;
                        }
                        la[i * nt + tid] += na;                    // this thread's own slot
                    }
                }
#pragma unroll
                for (int i = 0; i < KR; ++i) {
                    if (i < k) {
                        uint32_t nw = 0;
#pragma unroll
                        for (int e = 0; e < 8; ++e) nw += (w[e] == i && e < o.cnt) ? 1u : 0u;
                        lw[i * nt + tid] += nw;
                    }
                }
                float rr[8], dl[8], g[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const bool pos = S[e] >= 0.f, zero = eps[e] == 0.f;
                    const float tau = zero ? 0.f : (pos ? eps[e] : -eps[e]);
                    dl[e] = aten_fmul_(p.lambda, tau);
                    rr[e] = aten_fadd_(bo[e], dl[e]);
                    if (e < o.cnt) {
                        cls[zero ? EMR_ZERO : (pos ? EMR_POS : EMR_NEG)] += 1u;
                        cls[EMR_CONTESTED] += seen[e] == 3u ? 1u : 0u;
                    }
                }
                emr_fused_store8(p, o, rr, dl, g);
                if constexpr (ONE) {
                    // the k sign comparisons out of registers: u = g - b_i (an own base comes back through the cache)
#pragma unroll
                    for (int i = 0; i < KR; ++i) {
                        if (i < k) {
                            if (!p.in.shared_base) ties_load8(p.in.base[i], p.in.dtype, o.i0, o.cnt, o.vec, b);
                            float u[8];
#pragma unroll
                            for (int e = 0; e < 8; ++e) u[e] = g[e] - b[e];
                            bool bu = false;
                            const uint32_t mb = emr_task_octet(d[i], u, o.cnt, sums[i], bu);
                            if (bu) bad_u |= 1u << i;
                            p.mask[i][r * p.PB + q] = (uint8_t)mb;
                        }
                    }
                }
            }
            if constexpr (ONE) {
#pragma unroll
                for (int i = 0; i < KR; ++i)
                    if (i < k) emr_sums_to_lds(sums[i], red + (size_t)i * EMR_NP * nt, nt, tid);
            }
#pragma unroll
            for (int c = 0; c < EMR_COUNTS; ++c)
                if (cls[c]) ex.lds_atomic_add(&tc[c], cls[c]);
            if (bad) ex.global_atomic_or_u32(p.flags, bad);
            if (bad_sum) ex.global_atomic_or_u32(p.flags + 1, bad_sum);
            if (bad_u) ex.global_atomic_or_u32(p.flags + 2, bad_u);
        });
        if constexpr (ONE) {
            tree(r, 0, k);
        } else {
            // a sweep per group of four tasks: f_i and b_i again, and the lane's own octets of out
            for (int g0 = 0; g0 < k; g0 += EMR_FUSED_GROUP) {
                const int ng = k - g0 < EMR_FUSED_GROUP ? k - g0 : EMR_FUSED_GROUP;
                ex.each(st, [&](int tid, EmptyState&) {
                    uint32_t bad_u = 0;
                    EmrSums sums[EMR_FUSED_GROUP];
#pragma unroll
                    for (int j = 0; j < EMR_FUSED_GROUP; ++j) sums[j] = EmrSums{0.0, 0.0, 0.0, 0.0, 0.0, 0ull, 0ull};
                    for (size_t q = tid; q < p.PB; q += nt) {
                        const Octet o = segment_octet(start, p.C, p.row_vec, q);
                        float b[8], g[8];
                        delta_base8(p.in, o, b);
                        ties_load8(p.out, p.base_out_dtype, o.i0, o.cnt, o.vec, g);
#pragma unroll
                        for (int j = 0; j < EMR_FUSED_GROUP; ++j) {
                            if (j < ng) {
                                float f[8], d[8], u[8];
                                delta_load8(p.in, g0 + j, o, b, f);
#pragma unroll
                                for (int e = 0; e < 8; ++e) { d[e] = f[e] - b[e]; u[e] = g[e] - b[e]; }
                                bool bu = false;
                                const uint32_t mb = emr_task_octet(d, u, o.cnt, sums[j], bu);
                                if (bu) bad_u |= 1u << (g0 + j);
                                p.mask[g0 + j][r * p.PB + q] = (uint8_t)mb;
                            }
                        }
                    }
#pragma unroll
                    for (int j = 0; j < EMR_FUSED_GROUP; ++j)
                        if (j < ng) emr_sums_to_lds(sums[j], red + (size_t)j * EMR_NP * nt, nt, tid);
                    if (bad_u) ex.global_atomic_or_u32(p.flags + 2, bad_u);
                });
                tree(r, g0, ng);
            }
        }
    }
    kept_fold(ex, st, la, k, p.agree);                             // (starts with the barrier the totals in tc need too)
    kept_fold(ex, st, lw, k, p.winner);
    ex.each(st, [&](int tid, EmptyState&) {
        if (tid < EMR_COUNTS && tc[tid]) ex.global_atomic_add(&p.counts[tid], (unsigned long long)tc[tid]);
    });
}

struct EmrFoldParams {
    int np;                     // values per row: EMR_NP * k <= EMR_FOLD_NP_MAX
    size_t nseg;                // rows
    const double* part;         // [nseg][np]
    double* out;                // [np]: out[t] = (((0.0 + part[0][t]) + part[1][t]) + ...)
};
SM_HD size_t emr_fold_lds_bytes(int np) { return (size_t)LDS_SCRATCH_FLOATS * 4 + (size_t)2 * EMR_FOLD_ROWS * np * sizeof(double); }

template <class Ex>
SM_HD void k_emr_fold(Ex& ex, const EmrFoldParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const int nt = ex.nthreads();                                  // EMR_FOLD_THREADS
    const size_t per = (size_t)EMR_FOLD_ROWS * p.np, total = p.nseg * p.np;
    const size_t nblk = (p.nseg + EMR_FOLD_ROWS - 1) / EMR_FOLD_ROWS;
    double* buf = (double*)(ex.lds() + LDS_SCRATCH_FLOATS);        // [2][EMR_FOLD_ROWS][np]
    ex.each(st, [&](int tid, EmptyState& s) {
        s.red[0] = 0.0;                                            // the lane's running sum, carried across the blocks
        for (size_t i = tid; i < per && i < total; i += nt) buf[i] = p.part[i];
    });
    ex.sync();
    for (size_t blk = 0; blk < nblk; ++blk) {
        ex.each(st, [&](int tid, EmptyState& s) {
            // the next block's loads go out first and land in the other buffer after this block is added
            const size_t next = (blk + 1) * per;
            double v[EMR_FOLD_PER];
#pragma unroll
            for (int j = 0; j < EMR_FOLD_PER; ++j) {
                const size_t i = (size_t)j * nt + tid;
                v[j] = (i < per && next + i < total) ? p.part[next + i] : 0.0;
            }
            if (tid < p.np) {
                const double* cur = buf + (blk & 1) * per;
                const size_t left = p.nseg - blk * EMR_FOLD_ROWS;
                const int rows = left < (size_t)EMR_FOLD_ROWS ? (int)left : EMR_FOLD_ROWS;
                double a = s.red[0];
                if (rows == EMR_FOLD_ROWS) {
#pragma unroll 16
                    for (int q = 0; q < EMR_FOLD_ROWS; ++q) a = geo_dadd(a, cur[q * p.np + tid]);
                } else {
                    for (int q = 0; q < rows; ++q) a = geo_dadd(a, cur[q * p.np + tid]);
                }
                s.red[0] = a;
            }
            double* nxt = buf + ((blk + 1) & 1) * per;
#pragma unroll
            for (int j = 0; j < EMR_FOLD_PER; ++j) {
                const size_t i = (size_t)j * nt + tid;
                if (i < per && next + i < total) nxt[i] = v[j];
            }
        });
        ex.sync();
    }
    ex.each(st, [&](int tid, EmptyState& s) {
        if (tid < p.np) p.out[tid] = s.red[0];
    });
}

// ---- kernel tags (sm_tag.hpp) and group 22 of smhip_side.hip (smhip_device.hpp) ----
// the fused pass in its two register variants, and the staged ordered fold of its rows' partials
SM_KERNEL_TAG_LB(KEmrMergeMask, EmrFusedParams, "emr_merge_mask", k_emr_merge_mask<EMR_REG_SMALL>(ex, p), EMR_THREADS, 2)
SM_KERNEL_TAG_LB(KEmrMergeMaskAny, EmrFusedParams, "emr_merge_mask", k_emr_merge_mask<TIES_MAX_MODELS>(ex, p), EMR_THREADS, 1)
SM_KERNEL_TAG_LB(KEmrFold, EmrFoldParams, "emr_fold", k_emr_fold(ex, p), EMR_FOLD_THREADS, 2)
#define SM_SIDE_KERNELS_22(X) X(KEmrMergeMask) X(KEmrMergeMaskAny) X(KEmrFold)

}  // namespace smhip
