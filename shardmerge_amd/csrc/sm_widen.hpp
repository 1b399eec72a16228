// sm_widen.hpp - WIDEN merge (Yu et al. 2024, "Extend Model Merging from Fine-Tuned to Pre-Trained Large Language Models
// via Weight Disentanglement"), an operator the reference does not have.  The function is stated in
// include/shardmerge_hip.h (smhip_widen_merge).  It is the first of the delta merges that weighs a finetune per COLUMN
// of a tensor viewed as R x C (per input feature of a Linear weight): a column's magnitude and direction are compared
// with the base's, the two divergences are RANKED within their finetune (which makes the measure scale-free), and the
// ranks become per-column, per-finetune weights through a softmax across the finetunes.  Every step is one correctly
// rounded operation, an integer count or a sum in an order that is a function of the shape alone, so these kernels
// equal a plain restatement bit for bit.
//
//   widen_colstats  the hot pass (matrix mode): P = sum f^2, B = sum b^2, X = sum f b per column in fp64.  A work-group
//                   of 256 is 32 octet-columns x 8 sub-lanes and owns one segment of WIDEN_SEG_ROWS rows of one finetune:
//                   a lane keeps its eight columns and walks down the rows rho = u, u + 8, ... of the segment with
//                   16-byte loads (24 fp64 accumulators), the 8 sub-lanes are reduced by the binary tree through LDS
//                   (the upper half stores, the lower half adds), one partial per segment, finetune, sum and column.
//                   The finetune index is part of the grid: ONE launch; a shared base is re-read per finetune.
//   widen_colfold   a thread per finetune and column: the segments added in index order, then m and d (or a in vector
//                   mode, straight from the inputs) as fp64; the non-finite flags.
//   widen_rank      ranks by counting, all pairs: a work-group stages one tile of WIDEN_RANK_TILE keys in LDS as uint64
//                   (a statistic is finite and >= +0, so it orders like its bits), a thread counts the keys below its
//                   own and adds that integer partial to its column's rank (the tile index is part of the grid); the
//                   rank sums go out with one 64-bit integer atomic per work-group.
//   widen_coef      a thread per column: the two softmaxes over k through sm_exp (sm_fusion.hpp), the cuts, the weights;
//                   the calibrated columns counted in LDS, one global atomic per counter and work-group.
//   widen_combine   geo_combine with weights per column: a lane keeps its eight columns and their KR x 8 weights in
//                   registers while it strides over rows (KR = 4 serves k <= 4, KR = 16 any k, the same source);
//                   base_out is read once.
// Tensor passes with a shared base: column statistics 2 K, combine K + 2: 3 K + 2.
#pragma once
#include "sm_fusion.hpp"

namespace smhip {

constexpr int WIDEN_SEG_ROWS = 512;               // rows per segment of the column sums
constexpr int WIDEN_SUB = 8;                      // sub-lanes of a segment: row rho belongs to sub-lane rho % 8
constexpr int WIDEN_OCTS = 32;                    // octet-columns of a work-group: 256 columns
constexpr int WIDEN_COLS = 8 * WIDEN_OCTS;
constexpr int WIDEN_THREADS = WIDEN_OCTS * WIDEN_SUB;
constexpr int WIDEN_SUMS = 3;                     // P, B, X
constexpr int WIDEN_STATS = 2;                    // m, d (vector mode: a at 0, nothing at 1)
constexpr int WIDEN_RANK_TILE = 1024;             // keys a work-group of widen_rank stages in LDS and counts against
constexpr int WIDEN_REG_SMALL = 4;                // k <= 4: the instantiation of widen_combine with 32 weight registers
constexpr size_t WIDEN_MAX_COLS = 65536;
static_assert(WIDEN_THREADS == 256, "the kernels below are launched with 256 threads");

// the octet of columns 8 * oc .. 8 * oc + 7 of row r of an R x C view: vec when C % 8 == 0 and every pointer is aligned
SM_HD Octet widen_octet(size_t r, size_t C, size_t oc, int vec) {
    const size_t c0 = 8 * oc, i0 = r * C + c0;
    const int cnt = (int)(C - c0 < 8 ? C - c0 : 8);
    return Octet{i0 >> 3, i0, 0, cnt, vec && cnt == 8};
}

// ---- widen_colstats ----------------------------------------------------------------------------------------------
struct WidenColstatsParams {
    TiesInputs in;
    size_t R, C;
    int nseg;                   // ceil(R / WIDEN_SEG_ROWS)
    int ncb;                    // ceil(C / WIDEN_COLS); the grid is k * nseg * ncb
    int vec;                    // C % 8 == 0 and the inputs are 16-byte aligned
    double* part;               // [nseg][k][WIDEN_SUMS][C]
};
struct WidenColState { double acc[WIDEN_SUMS][8]; };
// dynamic LDS beyond the scratch: the upper half of the sub-lanes' accumulators
SM_HD size_t widen_colstats_lds_floats() { return LDS_SCRATCH_FLOATS + (size_t)2 * (WIDEN_SUB / 2) * WIDEN_OCTS * WIDEN_SUMS * 8; }

template <class Ex>
SM_HD void k_widen_colstats(Ex& ex, const WidenColstatsParams& p) {
    typename Ex::template State<WidenColState> st;
    ex.init(st);
    const int k = p.in.k;
    const int cb = ex.bid() % p.ncb, g = (ex.bid() / p.ncb) % p.nseg, i = ex.bid() / p.ncb / p.nseg;
    const size_t row0 = (size_t)g * WIDEN_SEG_ROWS;
    const int rows = (int)(p.R - row0 < (size_t)WIDEN_SEG_ROWS ? p.R - row0 : (size_t)WIDEN_SEG_ROWS);
    double* red = (double*)(ex.lds() + LDS_SCRATCH_FLOATS);        // [WIDEN_SUB / 2][WIDEN_OCTS][WIDEN_SUMS * 8]
    ex.each(st, [&](int tid, WidenColState& s) {
        const int u = tid / WIDEN_OCTS;
        const size_t oc = (size_t)cb * WIDEN_OCTS + tid % WIDEN_OCTS;
#pragma unroll
        for (int q = 0; q < WIDEN_SUMS; ++q)
#pragma unroll
            for (int e = 0; e < 8; ++e) s.acc[q][e] = 0.0;
        if (8 * oc >= p.C) return;
        for (int rho = u; rho < rows; rho += WIDEN_SUB) {
            const Octet o = widen_octet(row0 + rho, p.C, oc, p.vec);
            float f[8], b[8];
            ties_load8(p.in.ft[i], p.in.dtype, o.i0, o.cnt, o.vec, f);
            ties_load8(p.in.base[i], p.in.dtype, o.i0, o.cnt, o.vec, b);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                // (the product of two fp32 values is exact in fp64: fused or not, this is ONE rounded addition)
                const double fd = (double)f[e], bd = (double)b[e];
                s.acc[0][e] = s.acc[0][e] + fd * fd;
                s.acc[1][e] = s.acc[1][e] + bd * bd;
                s.acc[2][e] = s.acc[2][e] + fd * bd;
            }
        }
    });
    // the fixed binary tree over the sub-lanes: p_u = p_u + p_(u + s) for u < s, s = 4, 2, 1
    for (int s2 = WIDEN_SUB / 2; s2 > 0; s2 >>= 1) {
        ex.each(st, [&](int tid, WidenColState& s) {
            const int u = tid / WIDEN_OCTS, ol = tid % WIDEN_OCTS;
            if (u < s2 || u >= 2 * s2) return;
            double* v = red + ((size_t)(u - s2) * WIDEN_OCTS + ol) * (WIDEN_SUMS * 8);
#pragma unroll
            for (int q = 0; q < WIDEN_SUMS; ++q)
#pragma unroll
                for (int e = 0; e < 8; ++e) v[q * 8 + e] = s.acc[q][e];
        });
        ex.sync();
        ex.each(st, [&](int tid, WidenColState& s) {
            const int u = tid / WIDEN_OCTS, ol = tid % WIDEN_OCTS;
            if (u >= s2) return;
            const double* v = red + ((size_t)u * WIDEN_OCTS + ol) * (WIDEN_SUMS * 8);
#pragma unroll
            for (int q = 0; q < WIDEN_SUMS; ++q)
#pragma unroll
                for (int e = 0; e < 8; ++e) s.acc[q][e] = s.acc[q][e] + v[q * 8 + e];
        });
        ex.sync();
    }
    ex.each(st, [&](int tid, WidenColState& s) {
        if (tid >= WIDEN_OCTS) return;
        const size_t c0 = 8 * ((size_t)cb * WIDEN_OCTS + tid);
#pragma unroll
        for (int q = 0; q < WIDEN_SUMS; ++q) {
            double* dst = p.part + (((size_t)g * k + i) * WIDEN_SUMS + q) * p.C;
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (c0 + e < p.C) dst[c0 + e] = s.acc[q][e];
        }
    });
}

// ---- widen_colfold -----------------------------------------------------------------------------------------------
// step 2 of the definition from the three sums of a column
SM_HD double widen_magnitude(double P, double B) { return __builtin_fabs(geo_dadd(geo_dsqrt(P), -geo_dsqrt(B))); }
SM_HD double widen_direction(double P, double B, double X) {
    const double den = geo_dsqrt(geo_dmul(P, B));
    if (den == 0.0 || !geo_finite(den)) return P == B ? 0.0 : 1.0;
    double c = geo_ddiv(X, den);
    c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);
    return geo_dadd(1.0, -c);
}

struct WidenColfoldParams {
    TiesInputs in;
    size_t C;
    int nseg;
    int vector_mode;            // R == 1: a = |finetune - base| from the inputs, part is not read
    const double* part;         // [nseg][k][WIDEN_SUMS][C]
    double* stat;               // [k][WIDEN_STATS][C]
    uint32_t* flags;            // [0]: bit i = finetune i or its base holds a NaN or an Inf
};
template <class Ex>
SM_HD void k_widen_colfold(Ex& ex, const WidenColfoldParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const int k = p.in.k;
    const int ncb = (int)((p.C + ex.nthreads() - 1) / ex.nthreads());
    const int i = ex.bid() / ncb;
    ex.each(st, [&](int tid, EmptyState&) {
        const size_t j = (size_t)(ex.bid() % ncb) * ex.nthreads() + tid;
        if (j >= p.C) return;
        double s0, s1 = 0.0;
        bool bad;
        if (p.vector_mode) {
            const float x = load_elem(p.in.ft[i], p.in.dtype, j) - load_elem(p.in.base[i], p.in.dtype, j);
            s0 = (double)fabsf(x);
            bad = !geo_finite(s0);
        } else {
            double S[WIDEN_SUMS];
#pragma unroll
            for (int q = 0; q < WIDEN_SUMS; ++q) {
                double a = 0.0;
                for (int g = 0; g < p.nseg; ++g) a = a + p.part[(((size_t)g * k + i) * WIDEN_SUMS + q) * p.C + j];
                S[q] = a;
            }
            bad = !geo_finite(S[0]) || !geo_finite(S[1]);
            s0 = widen_magnitude(S[0], S[1]);
            s1 = widen_direction(S[0], S[1], S[2]);
        }
        p.stat[((size_t)i * WIDEN_STATS + 0) * p.C + j] = s0;
        p.stat[((size_t)i * WIDEN_STATS + 1) * p.C + j] = s1;
        if (bad) ex.global_atomic_or_u32(p.flags, 1u << i);
    });
}

// ---- widen_rank --------------------------------------------------------------------------------------------------
struct WidenRankParams {
    size_t C;
    int ns;                     // statistics that are ranked: 2, or 1 in vector mode (the ranks of the other stay 0)
    const double* stat;         // [k][WIDEN_STATS][C]
    uint32_t* rank;             // [k][WIDEN_STATS][C], device, zeroed: a work-group adds its tile's counts
    unsigned long long* ranksum;    // [k][WIDEN_STATS], device, zeroed: the sum of the ranks
};
SM_HD size_t widen_rank_lds_floats() { return LDS_SCRATCH_FLOATS + (size_t)2 * WIDEN_RANK_TILE; }
SM_HD int widen_rank_tiles(size_t C) { return (int)((C + WIDEN_RANK_TILE - 1) / WIDEN_RANK_TILE); }

// the grid is k * WIDEN_STATS * ceil(C / 256) * widen_rank_tiles(C): a work-group counts, for its 256 columns, the keys
// of ONE tile that lie below each - integer partials, added in any order
template <class Ex>
SM_HD void k_widen_rank(Ex& ex, const WidenRankParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const int nt = ex.nthreads();
    const int ncb = (int)((p.C + nt - 1) / nt), ntiles = widen_rank_tiles(p.C);
    const int is = ex.bid() / ntiles / ncb;                        // finetune * WIDEN_STATS + statistic
    const size_t j0 = (size_t)(ex.bid() / ntiles % ncb) * nt, t0 = (size_t)(ex.bid() % ntiles) * WIDEN_RANK_TILE;
    const double* keys = p.stat + (size_t)is * p.C;                // (read as their bits: fus_d2u)
    uint64_t* tile = (uint64_t*)(ex.lds() + LDS_SCRATCH_FLOATS);   // [WIDEN_RANK_TILE]
    unsigned long long* fold = (unsigned long long*)ex.lds();      // [16] in the scratch
    if (is % WIDEN_STATS >= p.ns) return;
    const int len = (int)(p.C - t0 < (size_t)WIDEN_RANK_TILE ? p.C - t0 : (size_t)WIDEN_RANK_TILE);
    ex.each(st, [&](int tid, EmptyState&) { for (int t = tid; t < len; t += nt) tile[t] = fus_d2u(keys[t0 + t]); });
    ex.sync();
    ex.each(st, [&](int tid, EmptyState& s) {
        uint32_t below = 0;
        if (j0 + tid < p.C) {
            const uint64_t mine = fus_d2u(keys[j0 + tid]);
            for (int t = 0; t < len; ++t) below += tile[t] < mine ? 1u : 0u;
            if (below) ex.global_atomic_add_u32(&p.rank[(size_t)is * p.C + j0 + tid], below);
        }
        s.keep[0] = below;
    });
    ex.sync();
    // the sum of the partials: 16 threads add 16 of the work-group's 256 each, thread 0 the 16
    uint32_t* lr = (uint32_t*)tile;
    ex.each(st, [&](int tid, EmptyState& s) { lr[tid] = (uint32_t)s.keep[0]; });
    ex.sync();
    ex.each(st, [&](int tid, EmptyState&) {
        if (tid >= 16) return;
        unsigned long long a = 0;
        for (int t = tid; t < nt; t += 16) a += lr[t];
        fold[tid] = a;
    });
    ex.sync();
    ex.each(st, [&](int tid, EmptyState&) {
        if (tid != 0) return;
        unsigned long long a = 0;
        for (int t = 0; t < 16; ++t) a += fold[t];
        if (a) ex.global_atomic_add(&p.ranksum[is], a);
    });
}

// ---- widen_coef --------------------------------------------------------------------------------------------------
// steps 3 (its end) and 4: mu from the rank sum; the score of finetune i from the ranks of one statistic of a column
SM_HD double widen_mu(unsigned long long S, double Cd) { return geo_ddiv(geo_ddiv((double)S, Cd), Cd); }
SM_HD double widen_sigma(uint32_t rank, double Cd) { return geo_ddiv((double)rank, Cd); }

struct WidenCoefParams {
    int k;
    size_t C;
    int ns;                     // 2, or 1 in vector mode
    double alpha[TIES_MAX_MODELS];
    double ratio, calibration;
    const uint32_t* rank;       // [k][WIDEN_STATS][C]
    const unsigned long long* ranksum;  // [k][WIDEN_STATS]
    float* weight;              // [k][C]
    double* mu;                 // [k][WIDEN_STATS], device (written by work-group 0)
    unsigned long long* calibrated;     // [k][WIDEN_STATS], device, zeroed
};
// dynamic LDS beyond the scratch: mu [16][2] as doubles, then the counters [16][2]
SM_HD size_t widen_coef_lds_floats() { return LDS_SCRATCH_FLOATS + (size_t)3 * TIES_MAX_MODELS * WIDEN_STATS; }

template <class Ex>
SM_HD void k_widen_coef(Ex& ex, const WidenCoefParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const int k = p.k;
    const double Cd = (double)p.C;
    double* lmu = (double*)(ex.lds() + LDS_SCRATCH_FLOATS);        // [k][WIDEN_STATS]
    uint32_t* lc = (uint32_t*)(lmu + TIES_MAX_MODELS * WIDEN_STATS);
    ex.each(st, [&](int tid, EmptyState&) {
        if (tid >= TIES_MAX_MODELS * WIDEN_STATS) return;
        lc[tid] = 0;
        const double mu = (tid < k * WIDEN_STATS && tid % WIDEN_STATS < p.ns) ? widen_mu(p.ranksum[tid], Cd) : 0.0;
        lmu[tid] = mu;
        if (ex.bid() == 0 && tid < k * WIDEN_STATS) p.mu[tid] = mu;
    });
    ex.sync();
    ex.each(st, [&](int tid, EmptyState&) {
        const size_t j = (size_t)ex.bid() * ex.nthreads() + tid;
        if (j >= p.C) return;
        // the maximum and the sum of each statistic's softmax: nothing is kept per finetune, sm_exp runs again below
        double smax[WIDEN_STATS], Z[WIDEN_STATS];
#pragma unroll
        for (int s = 0; s < WIDEN_STATS; ++s) {
            smax[s] = 0.0; Z[s] = 0.0;
            if (s >= p.ns) continue;
            for (int i = 0; i < k; ++i) {
                const double sg = widen_sigma(p.rank[((size_t)i * WIDEN_STATS + s) * p.C + j], Cd);
                smax[s] = sg > smax[s] ? sg : smax[s];
            }
            for (int i = 0; i < k; ++i) {
                const double sg = widen_sigma(p.rank[((size_t)i * WIDEN_STATS + s) * p.C + j], Cd);
                Z[s] = geo_dadd(Z[s], sm_exp(geo_dadd(sg, -smax[s])));
            }
        }
        for (int i = 0; i < k; ++i) {
            double score[WIDEN_STATS];
#pragma unroll
            for (int s = 0; s < WIDEN_STATS; ++s) {
                score[s] = 0.0;
                if (s >= p.ns) continue;
                const double sg = widen_sigma(p.rank[((size_t)i * WIDEN_STATS + s) * p.C + j], Cd);
                const bool cal = sg > geo_dmul(p.ratio, lmu[i * WIDEN_STATS + s]);
                score[s] = cal ? p.calibration : geo_ddiv(sm_exp(geo_dadd(sg, -smax[s])), Z[s]);
                if (cal) ex.lds_atomic_add(&lc[i * WIDEN_STATS + s], 1u);
            }
            const double h = p.ns == WIDEN_STATS ? geo_dmul(0.5, geo_dadd(score[0], score[1])) : score[0];
            p.weight[(size_t)i * p.C + j] = (float)geo_dmul(p.alpha[i], h);
        }
    });
    ex.sync();
    ex.each(st, [&](int tid, EmptyState&) {
        if (tid < k * WIDEN_STATS && lc[tid]) ex.global_atomic_add(&p.calibrated[tid], (unsigned long long)lc[tid]);
    });
}

// ---- widen_combine -----------------------------------------------------------------------------------------------
struct WidenCombineParams {
    TiesInputs in;
    size_t R, C;
    int ncb;                    // ceil(C / WIDEN_COLS); the grid is ncb * ceil(R / rows_per_wg)
    int rows_per_wg;            // a multiple of WIDEN_SUB
    int vec;                    // C % 8 == 0 and every pointer is 16-byte aligned
    const float* weight;        // [k][C]
    float lambda;
    const void* base_out; int base_out_dtype;
    int out_is_base0;           // base_out is base[0] in the same dtype and the bases are shared: loaded once
    void* out;                  // base_out_dtype, [n]
    float* delta_out;           // optional fp32 [n]: lambda * M
    int chunks;                 // (of delta_inputs: not used)
};

template <int KR, class Ex>
SM_HD void k_widen_combine(Ex& ex, const WidenCombineParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const int k = p.in.k;
    const int cb = ex.bid() % p.ncb;
    const size_t row0 = (size_t)(ex.bid() / p.ncb) * p.rows_per_wg;
    ex.each(st, [&](int tid, EmptyState&) {
        const int u = tid / WIDEN_OCTS;
        const size_t oc = (size_t)cb * WIDEN_OCTS + tid % WIDEN_OCTS, c0 = 8 * oc;
        if (c0 >= p.C) return;
        float w[KR][8];
#pragma unroll
        for (int i = 0; i < KR; ++i)
#pragma unroll
            for (int e = 0; e < 8; ++e) w[i][e] = (i < k && c0 + e < p.C) ? p.weight[(size_t)i * p.C + c0 + e] : 0.f;
        for (int t = u; t < p.rows_per_wg && row0 + t < p.R; t += WIDEN_SUB) {
            const Octet o = widen_octet(row0 + t, p.C, oc, p.vec);
            float b[8], bo[8], M[8];
            delta_base8(p.in, o, b);
            delta_base_out8(p, o, b, bo);
#pragma unroll
            for (int e = 0; e < 8; ++e) M[e] = 0.f;
#pragma unroll
            for (int i = 0; i < KR; ++i) {
                if (i < k) {
                    float f[8];
                    delta_load8(p.in, i, o, b, f);
#pragma unroll
                    for (int e = 0; e < 8; ++e) M[e] = aten_fadd_(M[e], aten_fmul_(w[i][e], f[e] - b[e]));
                }
            }
            float r[8], dl[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                dl[e] = aten_fmul_(p.lambda, M[e]);
                r[e] = aten_fadd_(bo[e], dl[e]);
            }
            if (o.vec) { ties_store8(p.out, p.base_out_dtype, p.delta_out, o.oi, 8, true, r, dl); continue; }
            for (int e = 0; e < o.cnt; ++e) {
                if (p.delta_out) p.delta_out[o.i0 + e] = dl[e];
                if (p.base_out_dtype == DT_F32) ((float*)p.out)[o.i0 + e] = r[e];
                else ((uint16_t*)p.out)[o.i0 + e] = p.base_out_dtype == DT_BF16 ? f_to_bf16_any(r[e]) : f_to_f16_any(r[e]);
            }
        }
    });
}

// ---- kernel tags (sm_tag.hpp) and group 13 of smhip_side.hip (smhip_device.hpp) ----
// the ordered fp64 column sums (24 accumulators per lane), their fold into the two divergences, the ranks by counting, the
// per-column weights through sm_exp, the combine pass with k <= 4 x 8 weights per lane in registers, or up to 16 x 8
SM_KERNEL_TAG_LB(KWidenColstats, WidenColstatsParams, "widen_colstats", k_widen_colstats(ex, p), WIDEN_THREADS, 4)
SM_KERNEL_TAG_LB(KWidenColfold, WidenColfoldParams, "widen_colfold", k_widen_colfold(ex, p), 256, 4)
SM_KERNEL_TAG_LB(KWidenRank, WidenRankParams, "widen_rank", k_widen_rank(ex, p), 256, 4)
SM_KERNEL_TAG_LB(KWidenCoef, WidenCoefParams, "widen_coef", k_widen_coef(ex, p), 256, 4)
SM_KERNEL_TAG_LB(KWidenCombine, WidenCombineParams, "widen_combine", k_widen_combine<WIDEN_REG_SMALL>(ex, p), WIDEN_THREADS, 4)
SM_KERNEL_TAG_LB(KWidenCombineAny, WidenCombineParams, "widen_combine", k_widen_combine<TIES_MAX_MODELS>(ex, p), WIDEN_THREADS, 2)
#define SM_SIDE_KERNELS_13(X) X(KWidenColstats) X(KWidenColfold) X(KWidenRank) X(KWidenCoef) X(KWidenCombine) X(KWidenCombineAny)

}  // namespace smhip
