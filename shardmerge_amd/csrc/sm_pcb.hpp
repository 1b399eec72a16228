// sm_pcb.hpp - PCB merge (Du et al. 2024, "Parameter Competition Balancing for Model Merging"), an operator the
// reference does not have.  The function is stated in include/shardmerge_hip.h (smhip_pcb_merge).  It is the first of
// the delta merges whose weights are continuous, per element AND per finetune: an entry's score is how large it is
// within its own task (intra-balancing, through sm_exp) times how well it agrees with what all tasks together do to
// that weight (inter-balancing, through sm_tanh); the low scores are dropped, the rest averaged with their scores as
// weights.  Every step is one correctly rounded operation, an exact order statistic or an integer count in a stated
// order, so these kernels equal a plain restatement bit for bit.
//
//   sm_tanh      DEFINED here, next to sm_exp of sm_fusion.hpp and in its manner: the odd Taylor series below 2^-4,
//                (1 - e) / (1 + e) with e = sm_exp(-2 |x|) up to 22.5, 1 beyond - one rounded fp64 operation at a time.
//   pcb_fn       the probe behind smhip_pcb_fn: y[i] = sm_tanh(x[i]).
//   pcb_hist     one radix level (11 + 10 + 10 bits) of the selection of TWO ranks - the largest score M_i and the
//                q-th largest t_i - over the score stream of up to TIES_GROUP finetunes at once.  A score needs the sum
//                U of ALL k weighted entries of its element, so the k entries of an octet are formed once in registers
//                (KR = 4 serves k <= 4, KR = 16 any k, the same source) and the scores are recomputed from them, lo, hi
//                and U in every pass: nothing is cached between passes.  The histograms are stats_hist's ([m = 2] ranks,
//                a key goes to the first rank whose prefix it is under), so stats_select itself walks them.
//   pcb_merge    the fused pass: the entries, U and the scores as above, then the weights, the two fp32 sums, the one
//                division and the add-back; base_out is read once.  Counters: positive[i] a slot per (finetune, thread)
//                in LDS folded by kept_fold; covered and contested in registers, one LDS atomic per thread, one 64-bit
//                global atomic per counter and work-group.
// The clip's two order statistics per finetune come from stats_hist / stats_select (sm_stats.hpp) launched unchanged
// with m = 2: |tv_i| = fl32(|d_i| |alpha_i|) is monotone in |d_i|, so lo_i / hi_i are fl32(|alpha_i| q) of the order
// statistics q of |d_i|.
// The fp64 chains of a score (two sm_exp, a Horner chain, two divisions) run one entry after another in ONE rolled loop
// over the 8 elements and the KR finetunes: the register arrays are rotated by one with static indices instead of being
// indexed by the loop counters, so the kernel holds one copy of the chain and no array goes to scratch.
// Tensor passes with a shared base, k <= 4: 3 (K + 1) clip + 3 (K + 1) score + (K + 2) merge = 7 K + 8.
#pragma once
#include "sm_fusion.hpp"

namespace smhip {

constexpr int PCB_REG_SMALL = 4;                                  // k <= 4: the instantiation with four entries per element in registers
constexpr int PCB_RANKS = 2;                                      // of the score select: PCB_MAX (rank 1), PCB_CUT (rank q)
constexpr int PCB_MAX = 0, PCB_CUT = 1;
constexpr int PCB_HI = 0, PCB_LO = 1;                             // of the clip select: ranks r + 1 and n - r of |d_i|
constexpr int PCB_COVERED = 0, PCB_CONTESTED = 1, PCB_COUNTS = 2;
static_assert(PCB_RANKS <= STATS_MAX_RANKS, "both selects ride stats_select's ranks");

enum { PCB_TANH = 0 };
constexpr double PCB_TANH_SMALL = 0x1p-4, PCB_TANH_ONE = 22.5;    // the branch points: -2 * 22.5 is sm_exp's cutoff
constexpr double PCB_SCORE_MIN = 0x1p-126;                        // a score below it (or not above 0) is +0

// tanh x.  |x| < 2^-4: x P(x^2), P the Taylor series of tanh(x) / x to degree 8 in x^2 (the first term left out is
// below 2^-80 of the result).  2^-4 <= |x| <= 22.5: (1 - e) / (1 + e) with e = sm_exp(-2 |x|) (the product is exact),
// the sign of x.  Beyond (and for a NaN): +-1.  sm_tanh(+-0) = +-0.  Coefficients: 1, -1/3, 2/15, -17/315, 62/2835,
// -1382/155925, 21844/6081075, -929569/638512875, 6404582/10854718875, each rounded to fp64.
SM_HD double sm_tanh(double x) {
    const double c[9] = {
        0x1.0000000000000p+0, -0x1.5555555555555p-2, 0x1.1111111111111p-3, -0x1.ba1ba1ba1ba1cp-5,
        0x1.664f4882c10fap-6, -0x1.226e355e6c23dp-7, 0x1.d6d3d0e157de0p-9, -0x1.7da36452b75e3p-10,
        0x1.3558248036744p-11};
    const double ax = __builtin_fabs(x);
    if (ax < PCB_TANH_SMALL) return geo_dmul(x, sph_horner(c, geo_dmul(x, x)));
    double r = 1.0;
    if (ax <= PCB_TANH_ONE) {
        const double e = sm_exp(geo_dmul(-2.0, ax));
        r = geo_ddiv(geo_dadd(1.0, -e), geo_dadd(1.0, e));
    }
    return __builtin_copysign(r, x);
}
SM_HD double pcb_fn(int op, double x) { return sm_tanh(x); }

struct PcbFnParams {
    int op;                     // PCB_TANH
    size_t n;
    const double* x;
    double* y;
};
template <class Ex>
SM_HD void k_pcb_fn(Ex& ex, const PcbFnParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    ex.each(st, [&](int tid, EmptyState&) {
        const size_t i = (size_t)ex.bid() * ex.nthreads() + tid;
        if (i < p.n) p.y[i] = pcb_fn(p.op, p.x[i]);
    });
}

// ---- the score of one entry ------------------------------------------------------------------------------------------
// what steps 2 - 6 need of a finetune, in LDS: the clip bounds, the score's cut and maximum
struct PcbBounds { float lo[TIES_MAX_MODELS], hi[TIES_MAX_MODELS], t[TIES_MAX_MODELS], M[TIES_MAX_MODELS]; };
constexpr int PCB_BOUNDS_WORDS = sizeof(PcbBounds) / 4;
// step 2: lo_i / hi_i from the order statistics of |d_i| (stats_select's tau: rank q at [q * TIES_MAX_MODELS])
SM_HD float pcb_bound(float q, float alpha) { return fabsf(aten_fmul_(q, alpha)); }
// step 2: c = min(max(|tv|, lo), hi)
SM_HD float pcb_clip(float tv, float lo, float hi) {
    const float a = fabsf(tv);
    const float c = a < lo ? lo : a;
    return c > hi ? hi : c;
}
// steps 3 - 5: S of the entry tv of a finetune with bounds lo <= hi, under the sum U of its element; kd = fp64(k)
SM_HD float pcb_score(float tv, float U, float lo, float hi, double kd) {
    const double span = geo_dadd((double)hi, -(double)lo);
    const double s = hi == lo ? 0.0 : geo_ddiv(geo_dadd((double)pcb_clip(tv, lo, hi), -(double)lo), span);
    const double intra = sm_exp(geo_dmul(kd, geo_dadd(geo_dmul(s, s), -1.0)));
    const double inter = sm_tanh(geo_dmul((double)tv, (double)U));
    const double p = geo_dmul(intra, inter);
    return p >= PCB_SCORE_MIN ? (float)p : 0.f;
}
// step 6: the weight of a score S under the cut t and the maximum M of its finetune
SM_HD float pcb_scale(float S, float t, float M) {
    if (S < t || !(S > 0.f)) return 0.f;
    if (M == t) return 1.f;
    return aten_fadd_(S, -t) / aten_fadd_(M, -t);
}

// step 1 for one octet: tv[i][e] = fl32(d_i * alpha_i) for i < k (+0 beyond), U[e] their fp32 sum in index order
template <int KR, class Params>
SM_HD void pcb_entries8(const Params& p, const Octet& o, const float* b0, float (*tv)[8], float* U) {
    const int k = p.in.k;
    float b[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { b[e] = b0[e]; U[e] = 0.f; }
#pragma unroll
    for (int i = 0; i < KR; ++i) {
        if (i < k) {
            float f[8];
            delta_load8(p.in, i, o, b, f);
            const float al = p.alpha[i];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                tv[i][e] = aten_fmul_(f[e] - b[e], al);
                U[e] = aten_fadd_(U[e], tv[i][e]);
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) tv[i][e] = 0.f;
        }
    }
}
// the rotations of the rolled loops: column 0 of tv one finetune on (after KR of them it is where it was), every row
// of tv and v one element on
template <int KR>
SM_HD void pcb_next_finetune(float (*tv)[8]) {
    const float t0 = tv[0][0];
#pragma unroll
    for (int i = 0; i + 1 < KR; ++i) tv[i][0] = tv[i + 1][0];
    tv[KR - 1][0] = t0;
}
SM_HD void pcb_rotate8(float* v, float last) {
#pragma unroll
    for (int e = 0; e < 7; ++e) v[e] = v[e + 1];
    v[7] = last;
}
template <int KR>
SM_HD void pcb_next_element(float (*tv)[8], float* U) {
#pragma unroll
    for (int i = 0; i < KR; ++i) pcb_rotate8(tv[i], tv[i][0]);
    pcb_rotate8(U, U[0]);
}
// the bounds of the work-group into LDS (ends with the barrier)
template <class Ex, class St>
SM_HD void pcb_bounds(Ex& ex, St& st, PcbBounds* pb, const float* alpha, const float* q, const float* tm) {
    ex.each(st, [&](int tid, EmptyState&) {
        if (tid >= TIES_MAX_MODELS) return;
        pb->hi[tid] = pcb_bound(q[PCB_HI * TIES_MAX_MODELS + tid], alpha[tid]);
        pb->lo[tid] = pcb_bound(q[PCB_LO * TIES_MAX_MODELS + tid], alpha[tid]);
        pb->M[tid] = tm ? tm[PCB_MAX * TIES_MAX_MODELS + tid] : 0.f;
        pb->t[tid] = tm ? tm[PCB_CUT * TIES_MAX_MODELS + tid] : 0.f;
    });
    ex.sync();
}

// ---- pcb_hist: one radix level of the score select ---------------------------------------------------------------------
struct PcbHistParams {
    TiesInputs in;
    float alpha[TIES_MAX_MODELS];
    int first, count;           // the finetunes of this launch: first .. first + count - 1, count <= TIES_GROUP
    int level;                  // 1, 2 or 3
    const float* q;             // [STATS_MAX_RANKS][TIES_MAX_MODELS], device: the clip select's order statistics of |d_i|
    const RadixState* state;    // [k][STATS_MAX_RANKS]
    unsigned long long* hist;   // [k][STATS_HIST_STRIDE] of this level: level 1 [HIST1_BINS], levels 2, 3 [PCB_RANKS][HIST_LO_BINS]
    int chunks;                 // octets per thread
};
// dynamic LDS beyond the scratch: the bounds, then the histograms of the launch's finetunes
SM_HD int pcb_hist_words(int level) { return stats_hist_words(level, PCB_RANKS); }
SM_HD size_t pcb_hist_lds_words(int level, int count) { return (size_t)PCB_BOUNDS_WORDS + (size_t)count * pcb_hist_words(level); }

template <int KR, class Ex>
SM_HD void k_pcb_hist(Ex& ex, const PcbHistParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    PcbBounds* pb = (PcbBounds*)(ex.lds() + LDS_SCRATCH_FLOATS);
    uint32_t* lh = (uint32_t*)(pb + 1);                            // [count][per]
    const int per = pcb_hist_words(p.level);
    const int k = p.in.k;
    hist_zero(ex, st, lh, per * p.count);
    pcb_bounds(ex, st, pb, p.alpha, p.q, nullptr);
    ex.each(st, [&](int tid, EmptyState&) {
        const double kd = (double)k;
        for (int q = 0; q < p.chunks; ++q) {
            Octet o;
            if (!octet_at(p.in, ex.bid(), ex.nthreads(), p.chunks, tid, q, o)) break;
            float tv[KR][8], U[8], b[8];
            delta_base8(p.in, o, b);
            pcb_entries8<KR>(p, o, b, tv, U);
#pragma unroll 1
            for (int e = 0; e < 8; ++e) {
#pragma unroll 1
                for (int i = 0; i < KR; ++i) {
                    const int j = i - p.first;
                    if (j >= 0 && j < p.count && e < o.cnt) {
                        // (the sign bit is masked off: a score has none, and a NaN from non-finite deltas, where the call
                        // fails anyway, must still index inside the histogram)
                        const uint32_t key = f2u(pcb_score(tv[0][0], U[0], pb->lo[i], pb->hi[i], kd)) & 0x7fffffffu;
                        uint32_t* h = lh + j * per;
                        if (p.level == 1) {
                            ex.lds_atomic_add(&h[radix_bin(1, key, 0u)], 1u);
                        } else {
                            // the first rank whose prefix the key is under takes it: equal prefixes share that histogram
                            const int b0 = radix_bin(p.level, key, p.state[STATS_MAX_RANKS * i + PCB_MAX].prefix);
                            const int b1 = radix_bin(p.level, key, p.state[STATS_MAX_RANKS * i + PCB_CUT].prefix);
                            if (b0 >= 0) ex.lds_atomic_add(&h[PCB_MAX * HIST_LO_BINS + b0], 1u);
                            else if (b1 >= 0) ex.lds_atomic_add(&h[PCB_CUT * HIST_LO_BINS + b1], 1u);
                        }
                    }
                    pcb_next_finetune<KR>(tv);
                }
                pcb_next_element<KR>(tv, U);
            }
        }
    });
    hist_flush(ex, st, lh, per * p.count, [&](int b) { return &p.hist[(size_t)(p.first + b / per) * STATS_HIST_STRIDE + (b % per)]; });
}

// ---- pcb_merge: the fused pass of step 7 -----------------------------------------------------------------------------
struct PcbMergeParams {
    TiesInputs in;
    float alpha[TIES_MAX_MODELS];
    const void* base_out; int base_out_dtype;
    int out_is_base0;           // base_out is base[0] in the same dtype and the bases are shared: loaded once
    float lambda;
    const float* q;             // [STATS_MAX_RANKS][TIES_MAX_MODELS], device: the clip select's order statistics of |d_i|
    const float* tm;            // [STATS_MAX_RANKS][TIES_MAX_MODELS], device: M_i at [PCB_MAX], t_i at [PCB_CUT]
    void* out;                  // base_out_dtype, [n]
    float* delta_out;           // optional fp32 [n]: merged
    float* bounds;              // [2][TIES_MAX_MODELS], device: lo_i, then hi_i (written by work-group 0)
    unsigned long long* positive;   // [k], device: entries with S_i > 0
    unsigned long long* counts; // [PCB_COUNTS], device: covered, contested
    int chunks;                 // octets per thread
};
// dynamic LDS beyond the scratch: the bounds, dare_lds_words of positive counters, then the work-group's PCB_COUNTS totals
SM_HD size_t pcb_merge_lds_words(int k, int nthreads) { return (size_t)PCB_BOUNDS_WORDS + dare_lds_words(k, nthreads) + PCB_COUNTS; }

template <int KR, class Ex>
SM_HD void k_pcb_merge(Ex& ex, const PcbMergeParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const int nt = ex.nthreads();
    const int k = p.in.k;
    PcbBounds* pb = (PcbBounds*)(ex.lds() + LDS_SCRATCH_FLOATS);
    uint32_t* lc = (uint32_t*)(pb + 1);                            // [k][nt], then the totals (dare_lds_words)
    uint32_t* tot = lc + dare_lds_words(k, nt);                    // [PCB_COUNTS]
    ex.each(st, [&](int tid, EmptyState&) { if (tid < PCB_COUNTS) tot[tid] = 0; });
    kept_zero(ex, st, lc, k);                                      // (ends with the barrier)
    pcb_bounds(ex, st, pb, p.alpha, p.q, p.tm);
    ex.each(st, [&](int tid, EmptyState&) {
        if (ex.bid() == 0 && tid < k) { p.bounds[tid] = pb->lo[tid]; p.bounds[TIES_MAX_MODELS + tid] = pb->hi[tid]; }
        const double kd = (double)k;
        const float den_min = 1e-12f;
        uint32_t ncov = 0, ncon = 0;
        for (int q = 0; q < p.chunks; ++q) {
            Octet o;
            if (!octet_at(p.in, ex.bid(), nt, p.chunks, tid, q, o)) break;
            float tv[KR][8], U[8], b[8], bo[8], mg[8];
            delta_base8(p.in, o, b);
            delta_base_out8(p, o, b, bo);
            pcb_entries8<KR>(p, o, b, tv, U);
#pragma unroll
            for (int e = 0; e < 8; ++e) mg[e] = 0.f;
#pragma unroll 1
            for (int e = 0; e < 8; ++e) {
                const bool mine = e >= o.lo && e < o.cnt;
                float num = 0.f, den = 0.f;
                uint32_t nw = 0;                                   // finetunes with a weight above 0
#pragma unroll 1
                for (int i = 0; i < KR; ++i) {
                    if (i < k) {
                        const float t = tv[0][0], lo = pb->lo[i], hi = pb->hi[i];
                        const float S = pcb_score(t, U[0], lo, hi, kd);
                        const float w = pcb_scale(S, pb->t[i], pb->M[i]);
                        const float tvc = t == 0.f ? 0.f : copysignf(pcb_clip(t, lo, hi), t);
                        num = aten_fadd_(num, aten_fmul_(w, tvc));
                        den = aten_fadd_(den, w);
                        nw += w > 0.f ? 1u : 0u;
                        if (mine && S > 0.f) lc[i * nt + tid] += 1u;   // this thread's own slot
                    }
                    pcb_next_finetune<KR>(tv);
                }
                ncov += (mine && den > 0.f) ? 1u : 0u;
                ncon += (mine && nw >= 2u) ? 1u : 0u;
                pcb_rotate8(mg, num / (den > den_min ? den : den_min));
                pcb_next_element<KR>(tv, U);
            }
            float r[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) r[e] = aten_fadd_(bo[e], aten_fmul_(p.lambda, mg[e]));
            delta_store8(p, o, r, mg);
        }
        if (ncov) ex.lds_atomic_add(&tot[PCB_COVERED], ncov);
        if (ncon) ex.lds_atomic_add(&tot[PCB_CONTESTED], ncon);
    });
    kept_fold(ex, st, lc, k, p.positive);                          // (starts with the barrier the totals in tot need too)
    ex.each(st, [&](int tid, EmptyState&) {
        if (tid < PCB_COUNTS && tot[tid]) ex.global_atomic_add(&p.counts[tid], (unsigned long long)tot[tid]);
    });
}

// ---- kernel tags (sm_tag.hpp) and group 11 of smhip_side.hip (smhip_device.hpp) ----
// the two-rank radix level over the score stream (its scan is stats_select, as the clip's two order statistics are
// stats_hist / stats_select), the fused weighted pass - k <= 4 entries per element in registers, or up to 16 - and the
// probe of sm_tanh
SM_KERNEL_TAG_LB(KPcbHist, PcbHistParams, "pcb_hist", k_pcb_hist<PCB_REG_SMALL>(ex, p), 256, 4)
SM_KERNEL_TAG_LB(KPcbHistAny, PcbHistParams, "pcb_hist", k_pcb_hist<TIES_MAX_MODELS>(ex, p), 256, 2)
SM_KERNEL_TAG_LB(KPcbMerge, PcbMergeParams, "pcb_merge", k_pcb_merge<PCB_REG_SMALL>(ex, p), 256, 4)
SM_KERNEL_TAG_LB(KPcbMergeAny, PcbMergeParams, "pcb_merge", k_pcb_merge<TIES_MAX_MODELS>(ex, p), 256, 2)
SM_KERNEL_TAG_LB(KPcbFn, PcbFnParams, "pcb_fn", k_pcb_fn(ex, p), 256, 4)
#define SM_SIDE_KERNELS_11(X) X(KPcbHist) X(KPcbHistAny) X(KPcbMerge) X(KPcbMergeAny) X(KPcbFn)

}  // namespace smhip
