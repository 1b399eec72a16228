// sm_ties.hpp - TIES merge (Yadav et al. 2023: trim, elect a sign, merge the agreeing entries), an operator the
// reference does not have.  The function is stated in include/shardmerge_hip.h (smhip_ties_merge); every step of
// it is one correctly rounded fp32 operation or an exact order statistic, so these kernels equal a plain
// restatement of it bit for bit.
//
//   ties_hist    one radix level of the selection of the k-th largest |ft_i - base_i| for up to TIES_GROUP
//                finetunes at once: the deltas are formed on the fly from 16-byte loads, the magnitude of a finite
//                fp32 value orders like its low 31 bits, levels of 11 + 10 + 10 bits (HIST1_BINS / HIST_LO_BINS).
//                One LDS histogram per finetune, flushed with 64-bit global atomics.  Level 1 also raises a flag
//                bit per finetune whose delta holds a NaN or an Inf.
//   ties_select  one work-group per finetune walks that level's histogram from the top, fixes the next bits of the
//                threshold, the rank that is left inside the bin and the count of elements above it; after level 3
//                the threshold and the kept count (everything >= it, zeros excepted) are final.  All on the device.
//   ties_merge   the fused streaming pass: K finetunes, their bases and base_out are loaded once, trim / weights /
//                sign election / masked sums / division / add-back happen in registers, out is written once.
// Every level re-reads the inputs (no candidate lists): selection reads 3 (K + 1) tensors when the base is shared.
// The octet walk, the loader, the election and the radix step are sm_delta.hpp's; here are the keep test key >= tau and
// what ties_select writes.
#pragma once
#include "sm_delta.hpp"

namespace smhip {

struct TiesHistParams {
    TiesInputs in;
    int first, count;           // the finetunes of this launch: first .. first + count - 1, count <= TIES_GROUP
    int level;                  // 1, 2 or 3
    const RadixState* state;    // [k]
    unsigned long long* hist;   // [k][HIST1_BINS] of this level
    uint32_t* flags;            // [0]: bit i = finetune i has a non-finite delta
    int chunks;                 // octets per thread
};
template <class Ex>
SM_HD void k_ties_hist(Ex& ex, const TiesHistParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    uint32_t* lh = (uint32_t*)(ex.lds() + LDS_SCRATCH_FLOATS);
    const int nbins = radix_bins(p.level);
    hist_zero(ex, st, lh, nbins * p.count);
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
                const uint32_t prefix = p.level == 1 ? 0u : p.state[i].prefix;
                uint32_t* h = lh + j * nbins;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    if (e < o.cnt) {
                        const uint32_t key = delta_key(f[e] - b[e]);
                        if (p.level == 1 && key >= TIES_KEY_INF) bad |= 1u << i;
                        const int bin = radix_bin(p.level, key, prefix);
                        if (bin >= 0) ex.lds_atomic_add(&h[bin], 1u);
                    }
                }
            }
        }
        if (bad) ex.global_atomic_or_u32(p.flags, bad);
    });
    hist_flush(ex, st, lh, nbins * p.count, [&](int b) { return &p.hist[(size_t)(p.first + b / nbins) * HIST1_BINS + (b % nbins)]; });
}

struct TiesSelectParams {
    int level;                       // 1, 2 or 3
    unsigned long long k_keep;       // elements to keep per finetune (0: the threshold is +inf)
    const unsigned long long* hist;  // [k][HIST1_BINS] of this level
    RadixState* state;               // [k]
    float* threshold;                // [k], written after level 3
    unsigned long long* kept;        // [k], written after level 3
};
struct TiesSelectState { double red[2]; unsigned long long own; };
template <class Ex>
SM_HD void k_ties_select(Ex& ex, const TiesSelectParams& p) {
    typename Ex::template State<TiesSelectState> st;
    ex.init(st);
    unsigned long long* part = (unsigned long long*)(ex.lds() + LDS_SCRATCH_FLOATS);     // [TIES_SELECT_THREADS]
    const int m = ex.bid();
    const int nbins = radix_bins(p.level);
    const unsigned long long* h = p.hist + (size_t)m * HIST1_BINS;
    RadixState* s = p.state + m;
    const RadixState s0 = radix_start(p.level, p.k_keep, *s);
    ex.each(st, [&](int tid, TiesSelectState& t) { part[tid] = t.own = radix_own_sum(h, nbins, tid); });
    ex.sync();
    ex.each(st, [&](int tid, TiesSelectState& t) {
        if (p.k_keep == 0) {          // nothing is kept: no finite magnitude reaches +inf
            if (tid == 0 && p.level == 3) { p.threshold[m] = u2f(TIES_KEY_INF); p.kept[m] = 0; }
            return;
        }
        const RadixFound f = radix_select_step(h, nbins, part, t.own, s0.rank, tid);
        if (!f.found) return;
        const RadixState s1 = *s = radix_advance(p.level, s0, f);
        if (p.level == 3) {                                  // the bin is one key: the threshold; ties at it are all kept
            p.threshold[m] = u2f(s1.prefix);
            p.kept[m] = s1.above + (s1.prefix != 0u ? f.c : 0ull);       // a zero delta is never kept
        }
    });
}

struct TiesMergeParams {
    TiesInputs in;
    float alpha[TIES_MAX_MODELS];
    const void* base_out; int base_out_dtype;
    int out_is_base0;           // base_out is base[0] in the same dtype and the bases are shared: loaded once
    float lambda;
    int normalize;
    const float* threshold;     // [k], device
    void* out;                  // base_out_dtype, [n]
    float* delta_out;           // optional fp32 [n]: lambda * M
    int chunks;                 // octets per thread
};
template <class Ex>
SM_HD void k_ties_merge(Ex& ex, const TiesMergeParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    ex.each(st, [&](int tid, EmptyState&) {
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
                const uint32_t tau = f2u(p.threshold[i]);
                const float al = p.alpha[i];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float d = f[e] - b[e];
                    const uint32_t key = delta_key(d);
                    const bool kept = key >= tau && key != 0u;
                    el.add(e, kept ? aten_fmul_(d, al) : 0.f, al, 1);
                }
            }
            float r[8], dl[8];
            el.finish(1, p.normalize, 0.f, p.lambda, bo, r, dl);
            delta_store8(p, o, r, dl);
        }
    });
}

// ---- kernel tags (sm_tag.hpp) and this header's share of group 7 of smhip_side.hip (smhip_device.hpp) ----
// one radix level of the magnitude selection, its scan, and the fused merge pass
SM_KERNEL_TAG_LB(KTiesHist, TiesHistParams, "ties_hist", k_ties_hist(ex, p), 256, 4)
SM_KERNEL_TAG_LB(KTiesSelect, TiesSelectParams, "ties_select", k_ties_select(ex, p), TIES_SELECT_THREADS, 4)
SM_KERNEL_TAG_LB(KTiesMerge, TiesMergeParams, "ties_merge", k_ties_merge(ex, p), 256, 4)
#define SM_KERNELS_TIES(X) X(KTiesHist) X(KTiesSelect) X(KTiesMerge)

}  // namespace smhip
