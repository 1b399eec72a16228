// sm_fusion.hpp - the pairwise fusion operators (arcee_fusion, nearswap): ONE finetune grafted onto a base, element by
// element.  The function is stated in include/shardmerge_hip.h (smhip_fusion_merge).  ARCEE needs two things no other
// operator has: a per-row fp64 reduction THROUGH a transcendental (the KL divergence of the softmax of a finetune row
// from that of its base row) and a multi-rank exact select (three quartiles) over one stream of scores formed on the
// fly.  Every step is one correctly rounded operation, an exact order statistic or an integer count in a stated order,
// so these kernels equal a plain restatement bit for bit.
//
//   sm_exp / sm_log  the two functions, DEFINED here instead of borrowed from a library, as sm_sphere.hpp owns acos and
//                    sin: an argument reduction with a two-part ln 2, a Horner evaluation of a truncated Taylor series
//                    over geo_dadd / geo_dmul / geo_ddiv, one rounded fp64 operation at a time, the scale by an exactly
//                    constructed power of two - so the host, the device, the CPU emulator and a numpy restatement give
//                    the same bits.
//   fusion_fn        the probe behind smhip_fusion_fn: y[i] = sm_exp / sm_log (x[i]).
//   fusion_rowkl     one work-group of 256 per row.  Sweep 1: the two maxima (exact whatever the order), a tree in LDS.
//                    Sweep 2 (the row comes from L2: a 28672-element bf16 row pair is 112 KiB): S_a, S_b and U in fp64 in
//                    the row order of geo_gram - octet o of the row to lane o % 256, a lane adds in ascending index from
//                    +0, the 256 lanes by the fixed binary tree in LDS.  Thread 0 turns them into kappa.
//   fusion_hist      one radix level (11 + 10 + 10 bits) of the selection of THREE ranks over the ONE stream of scores
//                    s = |d| * kappa_row, formed on the fly from the finetune, the base and kappa.  Level 1: one 2048-bin
//                    histogram serves the three ranks.  Levels 2 and 3: a 1024-bin histogram per distinct prefix, a key
//                    goes to the first rank whose prefix it is under (stats_hist's rule), so equal ranks share to the end.
//   fusion_select    stats_select itself on that stream (one work-group); level 1 also folds min / max of kappa over the
//                    rows - kappa >= 0 orders like its bits, an integer tree in LDS.
//   fusion_merge     the fused gate pass, and with MODE = FUS_NEARSWAP the whole of nearswap: finetune, base and
//                    base_out are loaded once, the delta is gated (ARCEE: s > thr) or clamped (NEARSWAP: to [-t, t]) in
//                    registers and added back.  Counters: a register per thread, one LDS atomic per thread, one 64-bit
//                    global atomic per work-group.
// Tensor passes: ARCEE 2 (rowkl; its second read is L2's) + 3 x 2 (hist) + 4 (merge) = 12; NEARSWAP 4.
#pragma once
#include "sm_sphere.hpp"
#include "sm_stats.hpp"

namespace smhip {

enum { FUS_ARCEE = 0, FUS_NEARSWAP = 1 };
enum { FUS_EXP = 0, FUS_LOG = 1 };
enum { FUS_BAD_FT = 1, FUS_BAD_BASE = 2, FUS_BAD_DELTA = 4 };     // flags[0]
constexpr int FUS_RANKS = 3;                                      // Q1, Q2, Q3
static_assert(FUS_RANKS <= STATS_MAX_RANKS, "the three quartiles ride stats_select's ranks");

// ln 2 in two parts: HI carries 21 significant bits (k * HI is exact for |k| < 2^32), HI + LO = ln 2 to 2^-86
constexpr double FUS_LN2_HI = 0x1.62e42fee00000p-1, FUS_LN2_LO = 0x1.a39ef35793c76p-33;
constexpr double FUS_INV_LN2 = 0x1.71547652b82fep+0;              // fp64(1 / ln 2)
constexpr double FUS_SQRT2 = 0x1.6a09e667f3bcdp+0;                // fp64(sqrt 2)
// sm_exp is +0 below it: e^-45 < 2^-64, and S_a, S_b >= 1 (the row's maximum contributes e^0), so a row needs more than
// 2^11 such terms in ONE lane before they could move its sum by an ulp
constexpr double FUS_EXP_CUTOFF = -45.0;

SM_HD uint64_t fus_d2u(double d) { uint64_t u; memcpy(&u, &d, 8); return u; }
SM_HD double fus_u2d(uint64_t u) { double d; memcpy(&d, &u, 8); return d; }

// e^a on (-inf, 0]; +0 for a < FUS_EXP_CUTOFF (and for a NaN).  k = floor(a / ln 2 + 1/2), r = (a - k HI) - k LO with
// |r| <= ln 2 / 2 (a - k HI is exact), e^r by its Taylor series to degree 14 (the first term left out is below 2^-62),
// times 2^k built from its exponent field (k >= -65: a normal number, the product is exact).  Coefficients: 1 / n!
// rounded to fp64.  Outside the domain the value is unspecified.
SM_HD double sm_exp(double a) {
    const double c[15] = {
        0x1.0000000000000p+0, 0x1.0000000000000p+0, 0x1.0000000000000p-1, 0x1.5555555555555p-3,
        0x1.5555555555555p-5, 0x1.1111111111111p-7, 0x1.6c16c16c16c17p-10, 0x1.a01a01a01a01ap-13,
        0x1.a01a01a01a01ap-16, 0x1.71de3a556c734p-19, 0x1.27e4fb7789f5cp-22, 0x1.ae64567f544e4p-26,
        0x1.1eed8eff8d898p-29, 0x1.6124613a86d09p-33, 0x1.93974a8c07c9dp-37};
    if (!(a >= FUS_EXP_CUTOFF)) return 0.0;
    const double kd = __builtin_floor(geo_dadd(geo_dmul(a, FUS_INV_LN2), 0.5));
    const double r = geo_dadd(geo_dadd(a, -geo_dmul(kd, FUS_LN2_HI)), -geo_dmul(kd, FUS_LN2_LO));
    const double scale = fus_u2d((uint64_t)(1023 + (int)kd) << 52);
    return geo_dmul(sph_horner(c, r), scale);
}
// ln S on [1, 2^40).  S = m 2^e with m in (sqrt 2 / 2, sqrt 2] (the halving is exact), f = m - 1 (exact), s = f / (2 + f),
// ln m = 2 s P(s^2) with P the series of atanh(s) / s to degree 12 in s^2 (|s| <= 0.1716: the first term left out is
// below 2^-70), ln S = e HI + (ln m + e LO) (e HI is exact).  sm_log(1) = +0.  Coefficients: 1 / (2 j + 1) rounded to fp64.
SM_HD double sm_log(double S) {
    const double c[13] = {
        0x1.0000000000000p+0, 0x1.5555555555555p-2, 0x1.999999999999ap-3, 0x1.2492492492492p-3,
        0x1.c71c71c71c71cp-4, 0x1.745d1745d1746p-4, 0x1.3b13b13b13b14p-4, 0x1.1111111111111p-4,
        0x1.e1e1e1e1e1e1ep-5, 0x1.af286bca1af28p-5, 0x1.8618618618618p-5, 0x1.642c8590b2164p-5,
        0x1.47ae147ae147bp-5};
    const uint64_t u = fus_d2u(S);
    int e = (int)((u >> 52) & 0x7ffu) - 1023;
    double m = fus_u2d((u & 0x000fffffffffffffull) | 0x3ff0000000000000ull);
    if (m > FUS_SQRT2) { m = geo_dmul(m, 0.5); e += 1; }
    const double f = geo_dadd(m, -1.0);
    const double s = geo_ddiv(f, geo_dadd(2.0, f));
    const double lm = geo_dmul(geo_dmul(2.0, s), sph_horner(c, geo_dmul(s, s)));
    const double ed = (double)e;
    return geo_dadd(geo_dmul(ed, FUS_LN2_HI), geo_dadd(lm, geo_dmul(ed, FUS_LN2_LO)));
}
SM_HD double fusion_fn(int op, double x) { return op == FUS_EXP ? sm_exp(x) : sm_log(x); }

// step 1 of the definition from the three sums of a row: kappa = fp32(max(U / S_a - (ln S_a - ln S_b), 0)).  A row equal
// in finetune and base has a_j - b_j = +0 for every j, so U = +0, and S_a == S_b bit for bit, so both terms are +0:
// kappa = 0 exactly.
SM_HD float fusion_kappa(double sa, double sb, double u) {
    const double kl = geo_dadd(geo_ddiv(u, sa), -geo_dadd(sm_log(sa), -sm_log(sb)));
    return kl > 0.0 ? (float)kl : 0.f;
}

struct FusionFnParams {
    int op;                     // FUS_EXP / FUS_LOG
    size_t n;
    const double* x;
    double* y;
};
template <class Ex>
SM_HD void k_fusion_fn(Ex& ex, const FusionFnParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    ex.each(st, [&](int tid, EmptyState&) {
        const size_t i = (size_t)ex.bid() * ex.nthreads() + tid;
        if (i < p.n) p.y[i] = fusion_fn(p.op, p.x[i]);
    });
}

// ---- fusion_rowkl: one work-group of GEO_THREADS per row ---------------------------------------------------------
struct FusionRowKlParams {
    const void* ft;
    const void* base;
    int dtype;
    size_t C;                   // row length; the grid is the R rows
    int seg_vec;                // the pointers are 16-byte aligned and C % 8 == 0: a row starts at an octet boundary
    float* kl;                  // [R]: kappa
    uint32_t* flags;            // [0]: FUS_BAD_FT | FUS_BAD_BASE
};
// dynamic LDS beyond the scratch: the maxima's [2][nt] floats, then the sums' [3][nt] doubles
SM_HD size_t fusion_rowkl_lds_floats() { return LDS_SCRATCH_FLOATS + (size_t)2 * GEO_THREADS + (size_t)2 * 3 * GEO_THREADS; }

template <class Ex>
SM_HD void k_fusion_rowkl(Ex& ex, const FusionRowKlParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const int nt = ex.nthreads();                                  // GEO_THREADS
    float* mred = ex.lds() + LDS_SCRATCH_FLOATS;                   // [2][nt]
    double* red = (double*)(mred + 2 * nt);                        // [3][nt] (an even count of floats before it)
    const size_t start = (size_t)ex.bid() * p.C, len = p.C;
    // sweep 1: mx = max_j x_j, my = max_j y_j
    ex.each(st, [&](int tid, EmptyState&) {
        float mx = u2f(0xff800000u), my = u2f(0xff800000u);
        uint32_t bad = 0;
        for (size_t q = tid; q < segment_octets(len); q += nt) {
            const Octet o = segment_octet(start, len, p.seg_vec, q);
            float x[8], y[8];
            ties_load8(p.ft, p.dtype, o.i0, o.cnt, o.vec, x);
            ties_load8(p.base, p.dtype, o.i0, o.cnt, o.vec, y);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                if (e < o.cnt) {
                    if (delta_key(x[e]) >= TIES_KEY_INF) bad |= FUS_BAD_FT;
                    if (delta_key(y[e]) >= TIES_KEY_INF) bad |= FUS_BAD_BASE;
                    mx = x[e] > mx ? x[e] : mx;
                    my = y[e] > my ? y[e] : my;
                }
            }
        }
        mred[tid] = mx; mred[nt + tid] = my;
        if (bad) ex.global_atomic_or_u32(p.flags, bad);
    });
    ex.sync();
    for (int s = nt >> 1; s > 0; s >>= 1) {
        ex.each(st, [&](int tid, EmptyState&) {
            if (tid >= s) return;
            mred[tid] = mred[tid + s] > mred[tid] ? mred[tid + s] : mred[tid];
            mred[nt + tid] = mred[nt + tid + s] > mred[nt + tid] ? mred[nt + tid + s] : mred[nt + tid];
        });
        ex.sync();
    }
    // sweep 2: S_a = sum ea_j, S_b = sum eb_j, U = sum ea_j (a_j - b_j); octet q of the row to lane q % nt
    ex.each(st, [&](int tid, EmptyState&) {
        const double mx = (double)mred[0], my = (double)mred[nt];
        double sa = 0.0, sb = 0.0, u = 0.0;
        for (size_t q = tid; q < segment_octets(len); q += nt) {
            const Octet o = segment_octet(start, len, p.seg_vec, q);
            float x[8], y[8];
            ties_load8(p.ft, p.dtype, o.i0, o.cnt, o.vec, x);
            ties_load8(p.base, p.dtype, o.i0, o.cnt, o.vec, y);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                if (e < o.cnt) {
                    const double a = geo_dadd((double)x[e], -mx), b = geo_dadd((double)y[e], -my);
                    const double ea = sm_exp(a), eb = sm_exp(b);
                    sa = geo_dadd(sa, ea);
                    sb = geo_dadd(sb, eb);
                    u = geo_dadd(u, geo_dmul(ea, geo_dadd(a, -b)));
                }
            }
        }
        red[tid] = sa; red[nt + tid] = sb; red[2 * nt + tid] = u;
    });
    ex.sync();
    // the fixed binary tree of geo_gram: p[t] = p[t] + p[t + s] for t < s, s = nt / 2, nt / 4, ..., 1
    for (int s = nt >> 1; s > 0; s >>= 1) {
        ex.each(st, [&](int tid, EmptyState&) {
            if (tid >= s) return;
            for (int j = 0; j < 3; ++j) {
                double* v = red + j * nt;
                v[tid] = geo_dadd(v[tid], v[tid + s]);
            }
        });
        ex.sync();
    }
    ex.each(st, [&](int tid, EmptyState&) {
        if (tid == 0) p.kl[ex.bid()] = fusion_kappa(red[0], red[nt], red[2 * nt]);
    });
}

// ---- the score stream ------------------------------------------------------------------------------------------------
// step 2 of the definition: s_e = fl32(|d_e| * kappa_row(e)) for the 8 elements of octet o (those past its cnt get the
// row of element i0: never used).  C % 8 == 0 puts every octet in one row.
SM_HD void fusion_score8(const float* d, const Octet& o, const float* kl, size_t C, float* s) {
    const size_t row = o.i0 / C;
    const bool one_row = o.i0 - row * C + 8 <= C;
    const float kr = kl[row];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        float ke = kr;
        if (!one_row && e < o.cnt) ke = kl[(o.i0 + e) / C];
        s[e] = aten_fmul_(fabsf(d[e]), ke);
    }
}

struct FusionHistParams {
    TiesInputs in;              // k = 1
    int level;                  // 1, 2 or 3
    size_t C;                   // row length
    const float* kl;            // [R]
    const RadixState* state;    // [STATS_MAX_RANKS]
    unsigned long long* hist;   // of this level: level 1 [HIST1_BINS], levels 2, 3 [FUS_RANKS][HIST_LO_BINS]
    int chunks;                 // octets per thread
};
SM_HD int fusion_hist_words(int level) { return stats_hist_words(level, FUS_RANKS); }
template <class Ex>
SM_HD void k_fusion_hist(Ex& ex, const FusionHistParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    uint32_t* lh = (uint32_t*)(ex.lds() + LDS_SCRATCH_FLOATS);
    const int words = fusion_hist_words(p.level);
    hist_zero(ex, st, lh, words);
    ex.each(st, [&](int tid, EmptyState&) {
        uint32_t prefix[FUS_RANKS];
#pragma unroll
        for (int r = 0; r < FUS_RANKS; ++r) prefix[r] = p.level == 1 ? 0u : p.state[r].prefix;
        for (int q = 0; q < p.chunks; ++q) {
            Octet o;
            if (!octet_at(p.in, ex.bid(), ex.nthreads(), p.chunks, tid, q, o)) break;
            float b[8], d[8], s[8];
            ties_load8(p.in.base[0], p.in.dtype, o.i0, o.cnt, o.vec, b);
            ties_load8(p.in.ft[0], p.in.dtype, o.i0, o.cnt, o.vec, d);
#pragma unroll
            for (int e = 0; e < 8; ++e) d[e] = d[e] - b[e];
            fusion_score8(d, o, p.kl, p.C, s);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                if (e < o.cnt) {
                    // (the sign bit is masked off: a score has none for finite inputs, and a NaN from non-finite ones,
                    // where the call fails anyway, must still index inside the histogram)
                    const uint32_t key = f2u(s[e]) & 0x7fffffffu;
                    if (p.level == 1) {
                        ex.lds_atomic_add(&lh[radix_bin(1, key, 0u)], 1u);
                    } else {
                        bool taken = false;
#pragma unroll
                        for (int r = 0; r < FUS_RANKS; ++r) {
                            const int bin = radix_bin(p.level, key, prefix[r]);
                            if (!taken && bin >= 0) { ex.lds_atomic_add(&lh[r * HIST_LO_BINS + bin], 1u); taken = true; }
                        }
                    }
                }
            }
        }
    });
    hist_flush(ex, st, lh, words, [&](int b) { return &p.hist[b]; });
}

struct FusionSelectParams {
    StatsSelectParams sel;      // one stream (work-group 0), m = FUS_RANKS, rank[q] = n - rho_q: the rho_q-th SMALLEST
    size_t rows;
    const float* kl;            // [rows]
    uint32_t* kl_minmax;        // [2], device: the bits of min and max kappa (level 1)
};
constexpr size_t FUSION_SELECT_LDS = STATS_SELECT_LDS + 2 * TIES_SELECT_THREADS * sizeof(uint32_t);
template <class Ex>
SM_HD void k_fusion_select(Ex& ex, const FusionSelectParams& p) {
    k_stats_select(ex, p.sel);
    if (p.sel.level != 1) return;
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const int nt = ex.nthreads();                                  // TIES_SELECT_THREADS
    uint32_t* mm = (uint32_t*)((char*)ex.lds() + STATS_SELECT_LDS);          // [2][nt], past stats_select's partial sums
    ex.each(st, [&](int tid, EmptyState&) {
        uint32_t lo = 0xffffffffu, hi = 0u;
        for (size_t r = tid; r < p.rows; r += nt) {
            const uint32_t key = f2u(p.kl[r]);
            lo = key < lo ? key : lo;
            hi = key > hi ? key : hi;
        }
        mm[tid] = lo; mm[nt + tid] = hi;
    });
    ex.sync();
    for (int s = nt >> 1; s > 0; s >>= 1) {
        ex.each(st, [&](int tid, EmptyState&) {
            if (tid >= s) return;
            mm[tid] = mm[tid + s] < mm[tid] ? mm[tid + s] : mm[tid];
            mm[nt + tid] = umax(mm[nt + tid], mm[nt + tid + s]);
        });
        ex.sync();
    }
    ex.each(st, [&](int tid, EmptyState&) {
        if (tid == 0) { p.kl_minmax[0] = mm[0]; p.kl_minmax[1] = mm[nt]; }
    });
}

// ---- fusion_merge: the gate pass (ARCEE) and the whole of NEARSWAP ---------------------------------------------------
struct FusionMergeParams {
    TiesInputs in;              // k = 1
    const void* base_out; int base_out_dtype;
    int out_is_base0;           // base_out is the base in the same dtype: loaded once
    void* out;                  // base_out_dtype, [n]
    float* delta_out;           // optional fp32 [n]: M
    int chunks;                 // octets per thread
    size_t C;                   // ARCEE: row length
    const float* kl;            // ARCEE: [R]
    const float* quart;         // ARCEE: device, Q_q at [q * TIES_MAX_MODELS] (stats_select's tau)
    float iqr_mult;             // ARCEE: fp32(iqr_mult)
    float t;                    // NEARSWAP: fp32(t)
    float* threshold;           // ARCEE: device [1], thr (written by work-group 0)
    unsigned long long* count;  // device [1]: selected (ARCEE) / clipped (NEARSWAP)
    uint32_t* flags;            // [0]: FUS_BAD_DELTA
};
template <int MODE, class Ex>
SM_HD void k_fusion_merge(Ex& ex, const FusionMergeParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    uint32_t* tot = (uint32_t*)(ex.lds() + LDS_SCRATCH_FLOATS);    // [1]
    ex.each(st, [&](int tid, EmptyState&) { if (tid == 0) tot[0] = 0; });
    ex.sync();
    ex.each(st, [&](int tid, EmptyState&) {
        // step 3's last line: thr = fl32(Q2 + fl32(iqr * fl32(Q3 - Q1)))
        float thr = 0.f;
        if constexpr (MODE == FUS_ARCEE) {
            const float q1 = p.quart[0], q2 = p.quart[TIES_MAX_MODELS], q3 = p.quart[2 * TIES_MAX_MODELS];
            thr = aten_fadd_(q2, aten_fmul_(p.iqr_mult, aten_fadd_(q3, -q1)));
            if (ex.bid() == 0 && tid == 0) p.threshold[0] = thr;
        }
        uint32_t bad = 0, cnt = 0;
        for (int q = 0; q < p.chunks; ++q) {
            Octet o;
            if (!octet_at(p.in, ex.bid(), ex.nthreads(), p.chunks, tid, q, o)) break;
            float b[8], bo[8], d[8], s[8], r[8], M[8];
            ties_load8(p.in.base[0], p.in.dtype, o.i0, o.cnt, o.vec, b);
            delta_base_out8(p, o, b, bo);
            ties_load8(p.in.ft[0], p.in.dtype, o.i0, o.cnt, o.vec, d);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                d[e] = d[e] - b[e];
                if (delta_key(d[e]) >= TIES_KEY_INF) bad |= FUS_BAD_DELTA;
            }
            if constexpr (MODE == FUS_ARCEE) fusion_score8(d, o, p.kl, p.C, s);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                bool hit;                                          // selected / clipped
                if constexpr (MODE == FUS_ARCEE) {
                    hit = s[e] > thr;
                    M[e] = hit ? d[e] : 0.f;
                } else {
                    hit = fabsf(d[e]) > p.t;
                    M[e] = d[e] > p.t ? p.t : (d[e] < -p.t ? -p.t : d[e]);
                }
                r[e] = aten_fadd_(bo[e], M[e]);
                cnt += (hit && e < o.cnt) ? 1u : 0u;
            }
            delta_store8(p, o, r, M);
        }
        if (cnt) ex.lds_atomic_add(&tot[0], cnt);
        if (bad) ex.global_atomic_or_u32(p.flags, bad);
    });
    ex.sync();
    ex.each(st, [&](int tid, EmptyState&) {
        if (tid == 0 && tot[0]) ex.global_atomic_add(p.count, (unsigned long long)tot[0]);
    });
}

// ---- kernel tags (sm_tag.hpp) and group 10 of smhip_side.hip (smhip_device.hpp) ----
// the row KL through sm_exp / sm_log (54 VGPRs: the fp64 Horner chains run one element after another), the three-rank
// radix level over the score stream and its scan, the fused gate pass - which with FUS_NEARSWAP is the whole of
// nearswap - and the probe of the two defined functions
SM_KERNEL_TAG_LB(KFusionRowKl, FusionRowKlParams, "fusion_rowkl", k_fusion_rowkl(ex, p), GEO_THREADS, 4)
SM_KERNEL_TAG_LB(KFusionHist, FusionHistParams, "fusion_hist", k_fusion_hist(ex, p), 256, 4)
SM_KERNEL_TAG_LB(KFusionSelect, FusionSelectParams, "fusion_select", k_fusion_select(ex, p), TIES_SELECT_THREADS, 4)
SM_KERNEL_TAG_LB(KFusionMergeArcee, FusionMergeParams, "fusion_merge", k_fusion_merge<FUS_ARCEE>(ex, p), 256, 4)
SM_KERNEL_TAG_LB(KFusionMergeNear, FusionMergeParams, "fusion_merge", k_fusion_merge<FUS_NEARSWAP>(ex, p), 256, 4)
SM_KERNEL_TAG_LB(KFusionFn, FusionFnParams, "fusion_fn", k_fusion_fn(ex, p), 256, 4)
#define SM_SIDE_KERNELS_10(X) X(KFusionRowKl) X(KFusionHist) X(KFusionSelect) X(KFusionMergeArcee) X(KFusionMergeNear) X(KFusionFn)

}  // namespace smhip
