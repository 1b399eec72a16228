// sm_breadcrumbs.hpp - Model Breadcrumbs merge (Davari & Belilovsky 2023: trim each finetune's delta at BOTH ends - the
// smallest magnitudes, as TIES does, and the few largest ones - then add the masked deltas or elect a sign as TIES
// does), an operator the reference does not have.  The function is stated in include/shardmerge_hip.h
// (smhip_breadcrumbs_merge); every step of it is one correctly rounded fp32 operation or an exact order statistic, so
// these kernels equal a plain restatement of it bit for bit.
//
// Two order statistics per finetune - the (n_top + 1)-th largest magnitude (tau_hi) and the (n_top + k_keep)-th
// (tau_lo) - are found in the SAME three histogram passes that TIES spends on one:
//
//   crumbs_hist    one radix level for up to TIES_GROUP finetunes at once, levels of 11 + 10 + 10 bits as ties_hist.
//                  Level 1: one 2048-bin histogram per finetune serves both ranks.  Levels 2 and 3: two 1024-bin
//                  histograms per finetune, [0] for the keys under tau_hi's prefix and [1] for those under tau_lo's;
//                  while the two prefixes are equal every such key goes to [0] alone (one SHARED histogram) and the
//                  select reads [0] for both ranks.  LDS: 4 x 2048 x 4 B at every level, what ties_hist takes at level 1.
//   crumbs_select  one work-group per finetune walks that level's histogram(s) from the top for both ranks, fixes the
//                  next bits of both thresholds, the residual ranks and the counts above; after level 3 both thresholds,
//                  kept = (above_lo + count at tau_lo) - above_hi and dropped_top = above_hi are final.
//   crumbs_merge   the fused streaming pass of ties_merge with the two-sided test tau_lo <= key <= tau_hi && key != 0
//                  and the sign_election switch (0: the linear sum of dare_merge).
// Tensor passes: 3 (K + 1) for the selection + (K + 2) for the merge when the base is shared - TIES's 4K + 5.
#pragma once
#include "sm_ties.hpp"

namespace smhip {

constexpr int CRUMBS_HI = 0, CRUMBS_LO = 1;   // the two ranks of a finetune: its state is state[2 * i + which]

// selection state of one rank of one finetune (device memory)
struct CrumbsState {
    unsigned long long rank;    // 1-based rank (from the largest) wanted among the keys that share `prefix`
    unsigned long long above;   // keys known to be larger than every key with this prefix
    uint32_t prefix;            // key bits decided so far (11, 21, then all 31: the threshold)
    uint32_t pad;
};

struct CrumbsHistParams {
    TiesInputs in;
    int first, count;           // the finetunes of this launch: first .. first + count - 1, count <= TIES_GROUP
    int level;                  // 1, 2 or 3
    const CrumbsState* state;   // [k][2]
    unsigned long long* hist;   // [k][HIST1_BINS] of this level (levels 2, 3: [k][2][HIST_LO_BINS])
    uint32_t* flags;            // [0]: bit i = finetune i has a non-finite delta
    int chunks;                 // octets per thread
};
template <class Ex>
SM_HD void k_crumbs_hist(Ex& ex, const CrumbsHistParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    uint32_t* lh = (uint32_t*)(ex.lds() + LDS_SCRATCH_FLOATS);     // [count][HIST1_BINS] at every level
    const int nt = ex.nthreads();
    const size_t noct = (p.in.n + 7) / 8;
    ex.each(st, [&](int tid, EmptyState&) { for (int b = tid; b < HIST1_BINS * p.count; b += nt) lh[b] = 0; });
    ex.sync();
    ex.each(st, [&](int tid, EmptyState&) {
        const size_t start = (size_t)ex.bid() * p.chunks * nt;
        uint32_t bad = 0;
        for (int q = 0; q < p.chunks; ++q) {
            const size_t oi = start + (size_t)q * nt + tid;
            if (oi >= noct) break;
            const size_t i0 = 8 * oi;
            const int cnt = (int)((p.in.n - i0) < 8 ? (p.in.n - i0) : 8);
            const bool vec = p.in.aligned && cnt == 8;
            float b[8];
            if (p.in.shared_base) ties_load8(p.in.base[0], p.in.dtype, i0, cnt, vec, b);
            for (int j = 0; j < p.count; ++j) {
                const int i = p.first + j;
                float f[8];
                ties_load8(p.in.ft[i], p.in.dtype, i0, cnt, vec, f);
                if (!p.in.shared_base) ties_load8(p.in.base[i], p.in.dtype, i0, cnt, vec, b);
                const uint32_t phi = p.level == 1 ? 0u : p.state[2 * i + CRUMBS_HI].prefix;
                const uint32_t plo = p.level == 1 ? 0u : p.state[2 * i + CRUMBS_LO].prefix;
                uint32_t* h0 = lh + j * HIST1_BINS;
                uint32_t* h1 = h0 + HIST_LO_BINS;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    if (e < cnt) {
                        const uint32_t key = f2u(f[e] - b[e]) & 0x7fffffffu;
                        if (p.level == 1) {
                            if (key >= TIES_KEY_INF) bad |= 1u << i;
                            ex.lds_atomic_add(&h0[key >> 20], 1u);
                        } else {
                            // equal prefixes: the first test takes every such key, [1] stays empty (the shared histogram)
                            const uint32_t top = p.level == 2 ? key >> 20 : key >> 10;
                            const uint32_t bin = p.level == 2 ? (key >> 10) & 1023u : key & 1023u;
                            if (top == phi) ex.lds_atomic_add(&h0[bin], 1u);
                            else if (top == plo) ex.lds_atomic_add(&h1[bin], 1u);
                        }
                    }
                }
            }
        }
        if (bad) ex.global_atomic_or_u32(p.flags, bad);
    });
    ex.sync();
    ex.each(st, [&](int tid, EmptyState&) {
        for (int b = tid; b < HIST1_BINS * p.count; b += nt) {
            const uint32_t v = lh[b];
            if (v) ex.global_atomic_add(&p.hist[(size_t)p.first * HIST1_BINS + b], (unsigned long long)v);
        }
    });
}

// one work-group of TIES_SELECT_THREADS per finetune, both ranks; thread t owns TIES_SELECT_PER consecutive bins
struct CrumbsSelectParams {
    int level;                       // 1, 2 or 3
    unsigned long long k_keep;       // elements to keep per finetune (0: both thresholds are +inf)
    unsigned long long rank[2];      // level 1: n_top + 1 (CRUMBS_HI), n_top + k_keep (CRUMBS_LO)
    const unsigned long long* hist;  // [k][HIST1_BINS] of this level
    CrumbsState* state;              // [k][2]
    float* threshold_lo;             // [k], written after level 3
    float* threshold_hi;             // [k]
    unsigned long long* kept;        // [k]
    unsigned long long* dropped_top; // [k]
};
struct CrumbsSelectState { unsigned long long own[2]; };
template <class Ex>
SM_HD void k_crumbs_select(Ex& ex, const CrumbsSelectParams& p) {
    typename Ex::template State<CrumbsSelectState> st;
    ex.init(st);
    unsigned long long* part = (unsigned long long*)(ex.lds() + LDS_SCRATCH_FLOATS);     // [2][TIES_SELECT_THREADS]
    unsigned long long* fin = part + 2 * TIES_SELECT_THREADS;                            // [2][2]: above, count at the threshold
    const int m = ex.bid();
    const int nbins = p.level == 1 ? HIST1_BINS : HIST_LO_BINS;
    CrumbsState* s = p.state + 2 * m;
    unsigned long long rank[2], above0[2];
    uint32_t prefix0[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        rank[r] = p.level == 1 ? p.rank[r] : s[r].rank;
        above0[r] = p.level == 1 ? 0ull : s[r].above;
        prefix0[r] = p.level == 1 ? 0u : s[r].prefix;
    }
    // level 1, or equal prefixes so far: both ranks read histogram [0] (crumbs_hist left [1] empty)
    const unsigned long long* h[2];
    h[0] = p.hist + (size_t)m * HIST1_BINS;
    h[1] = (p.level == 1 || prefix0[0] == prefix0[1]) ? h[0] : h[0] + HIST_LO_BINS;
    ex.each(st, [&](int tid, CrumbsSelectState& t) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            unsigned long long a = 0;
            for (int q = 0; q < TIES_SELECT_PER; ++q) {
                const int b = tid * TIES_SELECT_PER + q;
                if (b < nbins) a += h[r][b];
            }
            t.own[r] = a;
            part[r * TIES_SELECT_THREADS + tid] = a;
        }
    });
    ex.sync();      // (every thread has read its copy of the state above: the writes below cannot reach those reads)
    ex.each(st, [&](int tid, CrumbsSelectState& t) {
        if (p.k_keep == 0) return;    // nothing is kept: no finite magnitude reaches +inf
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            unsigned long long higher = 0;                      // keys in the bins of the threads after this one
            for (int q = tid + 1; q < TIES_SELECT_THREADS; ++q) higher += part[r * TIES_SELECT_THREADS + q];
            if (!(higher < rank[r] && rank[r] <= higher + t.own[r])) continue;
            // the bin that holds the rank-th largest key is one of this thread's
            for (int q = TIES_SELECT_PER - 1; q >= 0; --q) {
                const int b = tid * TIES_SELECT_PER + q;
                const unsigned long long c = b < nbins ? h[r][b] : 0ull;
                if (rank[r] <= higher + c) {
                    s[r].prefix = (prefix0[r] << (p.level == 1 ? 0 : 10)) | (uint32_t)b;
                    s[r].rank = rank[r] - higher;
                    s[r].above = above0[r] + higher;
                    if (p.level == 3) { fin[2 * r] = above0[r] + higher; fin[2 * r + 1] = c; }
                    break;
                }
                higher += c;
            }
        }
    });
    if (p.level != 3) return;
    ex.sync();
    ex.each(st, [&](int tid, CrumbsSelectState&) {
        if (tid != 0) return;
        if (p.k_keep == 0) {
            p.threshold_lo[m] = u2f(TIES_KEY_INF); p.threshold_hi[m] = u2f(TIES_KEY_INF);
            p.kept[m] = 0; p.dropped_top[m] = 0;
            return;
        }
        // the bins are single keys now: the thresholds; ties at either are kept, a zero delta never is
        const uint32_t tau_lo = s[CRUMBS_LO].prefix;
        p.threshold_hi[m] = u2f(s[CRUMBS_HI].prefix);
        p.threshold_lo[m] = u2f(tau_lo);
        p.kept[m] = fin[2 * CRUMBS_LO] + (tau_lo != 0u ? fin[2 * CRUMBS_LO + 1] : 0ull) - fin[2 * CRUMBS_HI];
        p.dropped_top[m] = fin[2 * CRUMBS_HI];
    });
}
constexpr size_t CRUMBS_SELECT_LDS = LDS_SCRATCH_FLOATS * 4 + (2 * TIES_SELECT_THREADS + 4) * sizeof(unsigned long long);

struct CrumbsMergeParams {
    TiesInputs in;
    float alpha[TIES_MAX_MODELS];
    const void* base_out; int base_out_dtype;
    int out_is_base0;           // base_out is base[0] in the same dtype and the bases are shared: loaded once
    float lambda;
    int normalize;
    int sign_election;          // 1: breadcrumbs_ties, 0: breadcrumbs
    const float* threshold_lo;  // [k], device
    const float* threshold_hi;  // [k], device
    void* out;                  // base_out_dtype, [n]
    float* delta_out;           // optional fp32 [n]: lambda * M
    int chunks;                 // octets per thread
};
template <class Ex>
SM_HD void k_crumbs_merge(Ex& ex, const CrumbsMergeParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const int nt = ex.nthreads();
    const size_t noct = (p.in.n + 7) / 8;
    const float eps = 1e-8f;
    ex.each(st, [&](int tid, EmptyState&) {
        const size_t start = (size_t)ex.bid() * p.chunks * nt;
        float Dall = 0.f;                                          // breadcrumbs: the sum of ALL weights, kept or not
        for (int i = 0; i < p.in.k; ++i) Dall = aten_fadd_(Dall, p.alpha[i]);
        for (int q = 0; q < p.chunks; ++q) {
            const size_t oi = start + (size_t)q * nt + tid;
            if (oi >= noct) break;
            const size_t i0 = 8 * oi;
            const int cnt = (int)((p.in.n - i0) < 8 ? (p.in.n - i0) : 8);
            const bool vec = p.in.aligned && cnt == 8;
            float b[8], bo[8], S[8], P[8], N[8], DP[8], DN[8];
            if (p.in.shared_base) ties_load8(p.in.base[0], p.in.dtype, i0, cnt, vec, b);
            if (p.out_is_base0) {
#pragma unroll
                for (int e = 0; e < 8; ++e) bo[e] = b[e];
            } else {
                ties_load8(p.base_out, p.base_out_dtype, i0, cnt, vec, bo);
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) { S[e] = 0.f; P[e] = 0.f; N[e] = 0.f; DP[e] = 0.f; DN[e] = 0.f; }
            for (int i = 0; i < p.in.k; ++i) {
                float f[8];
                ties_load8(p.in.ft[i], p.in.dtype, i0, cnt, vec, f);
                if (!p.in.shared_base) ties_load8(p.in.base[i], p.in.dtype, i0, cnt, vec, b);
                const uint32_t tau_lo = f2u(p.threshold_lo[i]), tau_hi = f2u(p.threshold_hi[i]);
                const float al = p.alpha[i];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float d = f[e] - b[e];
                    const uint32_t key = f2u(d) & 0x7fffffffu;
                    const bool kept = key >= tau_lo && key <= tau_hi && key != 0u;
                    const float tv = kept ? aten_fmul_(d, al) : 0.f;
                    S[e] = aten_fadd_(S[e], tv);
                    if (p.sign_election) {       // as ties_merge: the running sums of the positive and of the negative entries
                        if (tv > 0.f) { P[e] = aten_fadd_(P[e], tv); DP[e] = aten_fadd_(DP[e], al); }
                        if (tv < 0.f) { N[e] = aten_fadd_(N[e], tv); DN[e] = aten_fadd_(DN[e], al); }
                    }
                }
            }
            float r[8], dl[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const bool pos = S[e] >= 0.f;
                float M = p.sign_election ? (pos ? P[e] : N[e]) : S[e];
                if (p.normalize) {
                    float D = p.sign_election ? (pos ? DP[e] : DN[e]) : Dall;
                    if (fabsf(D) < eps) D = 1.f;
                    M = M / D;
                }
                dl[e] = aten_fmul_(p.lambda, M);
                r[e] = aten_fadd_(bo[e], dl[e]);
            }
            ties_store8(p.out, p.base_out_dtype, p.delta_out, oi, cnt, vec, r, dl);
        }
    });
}

}  // namespace smhip
