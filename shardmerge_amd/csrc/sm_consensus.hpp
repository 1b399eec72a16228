// sm_consensus.hpp - Consensus merge (Wang et al. 2024, "Localizing Task Information for Improved Model Merging and
// Compression": TALL masks and their consensus), an operator the reference does not have.  The function is stated in
// include/shardmerge_hip.h (smhip_consensus_merge); every step of it is one correctly rounded fp32 operation, a
// comparison or an integer count, so the kernel equals a plain restatement of it bit for bit.
//
//   consensus_merge   the one fused streaming pass.  It is the first of the delta merges that needs the multi-task vector
//                     U of an element BEFORE it can judge each finetune's entry, so the k weighted entries of an octet
//                     stay in registers across the sum (or the TIES election): sweep one loads, forms tv_i and U, sweep
//                     two compares |tv_i| with mask_lambda * |U - tv_i| out of registers - the finetunes are read once.
//                     KR = 4 serves k <= 4 (32 registers of entries), KR = 16 any k (128), the same source.
//                     Counters: masked[i] a slot per (finetune, thread) in LDS folded by kept_fold; agree[c] and selected
//                     in packed per-thread registers, added to a work-group's LDS totals, then one 64-bit global atomic
//                     per counter and work-group.
// The TIES flavour's thresholds come from ties_hist / ties_select (sm_ties.hpp) through the shared select host path.
#pragma once
#include "sm_ties.hpp"

namespace smhip {

constexpr int CONSENSUS_REG_SMALL = 4;                            // k <= 4: the instantiation with four entries per element in registers
constexpr int CONSENSUS_COUNTS = TIES_MAX_MODELS + 2;             // agree[0 .. 16], then selected
constexpr int CONSENSUS_FLUSH_OCTETS = 31;                        // 8-bit fields: at most 8 * 31 = 248 elements between two flushes

struct ConsensusMergeParams {
    TiesInputs in;
    float alpha[TIES_MAX_MODELS];
    const void* base_out; int base_out_dtype;
    int out_is_base0;           // base_out is base[0] in the same dtype and the bases are shared: loaded once
    float lambda;
    int normalize;
    int ties;                   // 1: U is the TIES merge under `threshold`; 0: the plain sum of the weighted entries
    const float* threshold;     // [k], device (ties)
    float mask_lambda;
    uint32_t need;              // min(consensus_k, k): masks that must agree
    void* out;                  // base_out_dtype, [n]
    float* delta_out;           // optional fp32 [n]: lambda * M
    unsigned long long* masked; // [k], device: elements whose mask m_i is set
    unsigned long long* counts; // [CONSENSUS_COUNTS], device: agree[c], then selected
    uint32_t* flags;            // [0]: bit i = finetune i has a non-finite delta
    int chunks;                 // octets per thread
};
// dynamic LDS beyond the scratch: dare_lds_words of masked counters, then the work-group's CONSENSUS_COUNTS totals
SM_HD size_t consensus_lds_words(int k, int nthreads) { return dare_lds_words(k, nthreads) + CONSENSUS_COUNTS; }

template <int KR, class Ex>
SM_HD void k_consensus_merge(Ex& ex, const ConsensusMergeParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    constexpr int NW = KR / 8 + 1;                                 // 64-bit words of eight 8-bit fields: agree[0 .. KR]
    const int nt = ex.nthreads();
    const int k = p.in.k;
    const float eps = 1e-8f;
    uint32_t* lc = (uint32_t*)(ex.lds() + LDS_SCRATCH_FLOATS);     // [k][nt], then the totals (dare_lds_words)
    uint32_t* ag = lc + dare_lds_words(k, nt);                     // [CONSENSUS_COUNTS]
    ex.each(st, [&](int tid, EmptyState&) { if (tid < CONSENSUS_COUNTS) ag[tid] = 0; });
    kept_zero(ex, st, lc, k);                                      // (ends with the barrier)
    ex.each(st, [&](int tid, EmptyState&) {
        uint32_t bad = 0, nsel = 0;
        unsigned long long acc[NW];
#pragma unroll
        for (int w = 0; w < NW; ++w) acc[w] = 0ull;
        auto flush = [&]() {
#pragma unroll
            for (int c = 0; c <= KR; ++c) {
                const uint32_t v = (uint32_t)(acc[c >> 3] >> (8 * (c & 7))) & 0xffu;
                if (v) ex.lds_atomic_add(&ag[c], v);
            }
#pragma unroll
            for (int w = 0; w < NW; ++w) acc[w] = 0ull;
        };
        const float Dall = delta_weight_sum(p.alpha, k);
        for (int q = 0; q < p.chunks; ++q) {
            Octet o;
            if (!octet_at(p.in, ex.bid(), nt, p.chunks, tid, q, o)) break;
            float tv[KR][8], b[8], bo[8];
            delta_base8(p.in, o, b);
            delta_base_out8(p, o, b, bo);
            Election el;
            el.clear();
            // sweep one: the weighted entries (kept in tv) and their sum, or the election over the trimmed ones
#pragma unroll
            for (int i = 0; i < KR; ++i) {
                if (i < k) {
                    float f[8];
                    delta_load8(p.in, i, o, b, f);
                    const float al = p.alpha[i];
                    const uint32_t tau = p.ties ? f2u(p.threshold[i]) : 0u;
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float d = f[e] - b[e];
                        const uint32_t key = delta_key(d);
                        if (key >= TIES_KEY_INF) bad |= 1u << i;
                        const float t = aten_fmul_(d, al);
                        const bool trimmed = p.ties && !(key >= tau && key != 0u);
                        el.add(e, trimmed ? 0.f : t, al, p.ties);
                        tv[i][e] = t;                              // trimming does not touch the mask's entry
                    }
                }
            }
            float U[8];
            uint32_t c[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) { U[e] = p.ties ? el.merged(e, 1, p.normalize, 0.f) : el.S[e]; c[e] = 0u; }
            // sweep two, out of registers: m_i = |tv_i| >= mask_lambda * |U - tv_i| (a NaN on the right compares false)
#pragma unroll
            for (int i = 0; i < KR; ++i) {
                if (i < k) {
                    uint32_t nm = 0;
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float rhs = aten_fmul_(p.mask_lambda, fabsf(aten_fadd_(U[e], -tv[i][e])));
                        const bool m = fabsf(tv[i][e]) >= rhs;
                        c[e] += m ? 1u : 0u;
                        nm += (m && e >= o.lo && e < o.cnt) ? 1u : 0u;     // (an element past the end is all zeros: every mask set)
                    }
                    lc[i * nt + tid] += nm;                        // this thread's own slot
                }
            }
            float r[8], dl[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const bool sel = c[e] >= p.need;
                float M = U[e];
                if (!p.ties && p.normalize) {
                    float D = Dall;
                    if (fabsf(D) < eps) D = 1.f;
                    M = M / D;
                }
                if (!sel) M = 0.f;
                dl[e] = aten_fmul_(p.lambda, M);
                r[e] = aten_fadd_(bo[e], dl[e]);
                if (e >= o.lo && e < o.cnt) {
#pragma unroll
                    for (int w = 0; w < NW; ++w)
                        if ((int)(c[e] >> 3) == w) acc[w] += 1ull << (8 * (c[e] & 7u));
                    nsel += sel ? 1u : 0u;
                }
            }
            delta_store8(p, o, r, dl);
            if (q % CONSENSUS_FLUSH_OCTETS == CONSENSUS_FLUSH_OCTETS - 1) flush();
        }
        flush();
        if (nsel) ex.lds_atomic_add(&ag[TIES_MAX_MODELS + 1], nsel);
        if (bad) ex.global_atomic_or_u32(p.flags, bad);
    });
    kept_fold(ex, st, lc, k, p.masked);                            // (starts with the barrier the totals in ag need too)
    ex.each(st, [&](int tid, EmptyState&) {
        if (tid < CONSENSUS_COUNTS && ag[tid]) ex.global_atomic_add(&p.counts[tid], (unsigned long long)ag[tid]);
    });
}

// ---- kernel tags (sm_tag.hpp) and this header's share of group 7 of smhip_side.hip (smhip_device.hpp) ----
// the one fused pass with the k weighted entries of an octet in registers across the sum / election; k <= 4 at
// dare_merge's residency, or up to 16
SM_KERNEL_TAG_LB(KConsensusMerge, ConsensusMergeParams, "consensus_merge", k_consensus_merge<CONSENSUS_REG_SMALL>(ex, p), 256, 4)
SM_KERNEL_TAG_LB(KConsensusMergeAny, ConsensusMergeParams, "consensus_merge", k_consensus_merge<TIES_MAX_MODELS>(ex, p), 256, 2)
#define SM_KERNELS_CONSENSUS(X) X(KConsensusMerge) X(KConsensusMergeAny)

}  // namespace smhip
