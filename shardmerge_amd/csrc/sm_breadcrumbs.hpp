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
// The walk, the loader, the election and the radix step are sm_delta.hpp's; here are the two prefixes and the two-sided test.
// Tensor passes: 3 (K + 1) for the selection + (K + 2) for the merge when the base is shared - TIES's 4K + 5.
#pragma once
#include "sm_ties.hpp"

namespace smhip {

constexpr int CRUMBS_HI = 0, CRUMBS_LO = 1;   // the two ranks of a finetune: its state is state[2 * i + which]

struct CrumbsHistParams {
    TiesInputs in;
    int first, count;           // the finetunes of this launch: first .. first + count - 1, count <= TIES_GROUP
    int level;                  // 1, 2 or 3
    const RadixState* state;    // [k][2]
    unsigned long long* hist;   // [k][HIST1_BINS] of this level (levels 2, 3: [k][2][HIST_LO_BINS])
    uint32_t* flags;            // [0]: bit i = finetune i has a non-finite delta
    int chunks;                 // octets per thread
};
template <class Ex>
SM_HD void k_crumbs_hist(Ex& ex, const CrumbsHistParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    uint32_t* lh = (uint32_t*)(ex.lds() + LDS_SCRATCH_FLOATS);     // [count][HIST1_BINS] at every level
    hist_zero(ex, st, lh, HIST1_BINS * p.count);
    ex.each(st, [&](int tid, EmptyState&) {
        uint32_t bad = 0;
        for (int q = 0; q < p.chunks; ++q) {
            Octet o;
            if (!octet_at(p.in, ex.bid(), ex.nthreads(), p.chunks, tid, q, o)) break;
            float b[8];
            delta_base8(p.in, o, b);
            for (int j = 0; j < p.count; ++j) {
                const int i = p.first + j;
                float f[8];
                delta_load8(p.in, i, o, b, f);
                const uint32_t phi = p.level == 1 ? 0u : p.state[2 * i + CRUMBS_HI].prefix;
                const uint32_t plo = p.level == 1 ? 0u : p.state[2 * i + CRUMBS_LO].prefix;
                uint32_t* h0 = lh + j * HIST1_BINS;
                uint32_t* h1 = h0 + HIST_LO_BINS;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    if (e < o.cnt) {
                        const uint32_t key = delta_key(f[e] - b[e]);
                        if (p.level == 1 && key >= TIES_KEY_INF) bad |= 1u << i;
                        // equal prefixes: the first test takes every such key, [1] stays empty (the shared histogram)
                        const int b0 = radix_bin(p.level, key, phi), b1 = radix_bin(p.level, key, plo);
                        if (b0 >= 0) ex.lds_atomic_add(&h0[b0], 1u);
                        else if (b1 >= 0) ex.lds_atomic_add(&h1[b1], 1u);
                    }
                }
            }
        }
        if (bad) ex.global_atomic_or_u32(p.flags, bad);
    });
    hist_flush(ex, st, lh, HIST1_BINS * p.count, [&](int b) { return &p.hist[(size_t)p.first * HIST1_BINS + b]; });
}

// one work-group of TIES_SELECT_THREADS per finetune, both ranks
struct CrumbsSelectParams {
    int level;                       // 1, 2 or 3
    unsigned long long k_keep;       // elements to keep per finetune (0: both thresholds are +inf)
    unsigned long long rank[2];      // level 1: n_top + 1 (CRUMBS_HI), n_top + k_keep (CRUMBS_LO)
    const unsigned long long* hist;  // [k][HIST1_BINS] of this level
    RadixState* state;               // [k][2]
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
    const int nbins = radix_bins(p.level);
    RadixState* s = p.state + 2 * m;
    const RadixState s0[2] = {radix_start(p.level, p.rank[0], s[0]), radix_start(p.level, p.rank[1], s[1])};
    // level 1, or equal prefixes so far: both ranks read histogram [0] (crumbs_hist left [1] empty)
    const unsigned long long* h[2];
    h[0] = p.hist + (size_t)m * HIST1_BINS;
    h[1] = (p.level == 1 || s0[0].prefix == s0[1].prefix) ? h[0] : h[0] + HIST_LO_BINS;
    ex.each(st, [&](int tid, CrumbsSelectState& t) {
#pragma unroll
        for (int r = 0; r < 2; ++r) part[r * TIES_SELECT_THREADS + tid] = t.own[r] = radix_own_sum(h[r], nbins, tid);
    });
    ex.sync();      // (every thread has read its copy of the state above: the writes below cannot reach those reads)
    ex.each(st, [&](int tid, CrumbsSelectState& t) {
        if (p.k_keep == 0) return;    // nothing is kept: no finite magnitude reaches +inf
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const RadixFound f = radix_select_step(h[r], nbins, part + r * TIES_SELECT_THREADS, t.own[r], s0[r].rank, tid);
            if (!f.found) continue;
            const RadixState s1 = s[r] = radix_advance(p.level, s0[r], f);
            if (p.level == 3) { fin[2 * r] = s1.above; fin[2 * r + 1] = f.c; }
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
    ex.each(st, [&](int tid, EmptyState&) {
        const float Dall = delta_weight_sum(p.alpha, p.in.k);
        for (int q = 0; q < p.chunks; ++q) {
            Octet o;
            if (!octet_at(p.in, ex.bid(), ex.nthreads(), p.chunks, tid, q, o)) break;
            float b[8], bo[8];
            delta_base8(p.in, o, b);
            delta_base_out8(p, o, b, bo);
            Election el;
            el.clear();
            for (int i = 0; i < p.in.k; ++i) {
                float f[8];
                delta_load8(p.in, i, o, b, f);
                const uint32_t tau_lo = f2u(p.threshold_lo[i]), tau_hi = f2u(p.threshold_hi[i]);
                const float al = p.alpha[i];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float d = f[e] - b[e];
                    const uint32_t key = delta_key(d);
                    const bool kept = key >= tau_lo && key <= tau_hi && key != 0u;
                    el.add(e, kept ? aten_fmul_(d, al) : 0.f, al, p.sign_election);
                }
            }
            float r[8], dl[8];
            el.finish(p.sign_election, p.normalize, Dall, p.lambda, bo, r, dl);
            delta_store8(p, o, r, dl);
        }
    });
}

// ---- kernel tags (sm_tag.hpp) and this header's share of group 7 of smhip_side.hip (smhip_device.hpp) ----
// the two-rank radix level, its scan, and the fused two-sided merge pass
SM_KERNEL_TAG_LB(KCrumbsHist, CrumbsHistParams, "crumbs_hist", k_crumbs_hist(ex, p), 256, 4)
SM_KERNEL_TAG_LB(KCrumbsSelect, CrumbsSelectParams, "crumbs_select", k_crumbs_select(ex, p), TIES_SELECT_THREADS, 4)
SM_KERNEL_TAG_LB(KCrumbsMerge, CrumbsMergeParams, "crumbs_merge", k_crumbs_merge(ex, p), 256, 4)
#define SM_KERNELS_CRUMBS(X) X(KCrumbsHist) X(KCrumbsSelect) X(KCrumbsMerge)

}  // namespace smhip
