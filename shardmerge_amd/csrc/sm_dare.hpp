// sm_dare.hpp - DARE merge (Yu et al. 2023: drop each delta entry at random, rescale the survivors, then add the
// weighted deltas or elect a sign as TIES does), an operator the reference does not have.  The function is stated in
// include/shardmerge_hip.h (smhip_dare_merge).  The drop mask is a FUNCTION of (key, stream id, element index): one
// Philox4x32-10 block (Salmon et al. 2011) per octet of eight consecutive elements, 16 bits per element, computed in
// registers - no tables, no LDS, no state in memory - so the result does not depend on the grid, the traversal order or
// the number of processes, and every other step is one correctly rounded fp32 operation: the kernel equals a plain
// restatement bit for bit.
//
//   dare_merge   the one fused streaming pass: per octet the base (once when shared), per finetune one 16-byte load,
//                one Philox block, eight compares, the fp32 chain; out is written once.  Kept counts: a counter per
//                thread and finetune in LDS, reduced per work-group, one 64-bit global atomic per finetune.
#pragma once
#include "sm_delta.hpp"

namespace smhip {

constexpr uint32_t DARE_T_ONE = 65536u;       // the threshold of density 1: every 16-bit draw is below it

// (hi, lo) of the 64-bit product a * b
SM_HD void philox_mulhilo(uint32_t a, uint32_t b, uint32_t& hi, uint32_t& lo) {
#if defined(__HIP_DEVICE_COMPILE__)
    hi = __umulhi(a, b);
    lo = a * b;
#else
    const uint64_t p = (uint64_t)a * (uint64_t)b;
    hi = (uint32_t)(p >> 32);
    lo = (uint32_t)p;
#endif
}

// Philox4x32-10: counter c[4] -> c[4] under the key (k0, k1)
SM_HD void philox4x32_10(uint32_t* c, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        uint32_t hi0, lo0, hi1, lo1;
        philox_mulhilo(0xD2511F53u, c[0], hi0, lo0);
        philox_mulhilo(0xCD9E8D57u, c[2], hi1, lo1);
        c[0] = hi1 ^ c[1] ^ k0;
        c[1] = lo1;
        c[2] = hi0 ^ c[3] ^ k1;
        c[3] = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

// The eight 16-bit draws h of the octet that holds element j of the finetune with this stream id: one Philox block whose
// counter is (j >> 3, stream_id, 0).
SM_HD void dare_draws8(uint64_t key, uint32_t stream_id, uint64_t j, uint32_t* h) {
    const uint64_t oct = j >> 3;
    uint32_t c[4] = {(uint32_t)oct, (uint32_t)(oct >> 32), stream_id, 0u};
    philox4x32_10(c, (uint32_t)key, (uint32_t)(key >> 32));
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const uint32_t w = c[e >> 1];
        h[e] = (e & 1) ? (w >> 16) : (w & 0xffffu);
    }
}
// THE mask: bit e of the result is set iff element 8 * (j >> 3) + e draws a value below T.
SM_HD uint32_t dare_mask8(uint64_t key, uint32_t stream_id, uint64_t j, uint32_t T) {
#if defined(SM_DARE_NO_PHILOX)      // A/B measurement only (tools/dare_bench.py --ab-lib): no generator, every element kept
    return 0xffu;
#endif
    uint32_t h[8], m = 0;
    dare_draws8(key, stream_id, j, h);
#pragma unroll
    for (int e = 0; e < 8; ++e) m |= (h[e] < T ? 1u : 0u) << e;
    return m;
}

struct DareMergeParams {
    TiesInputs in;
    float alpha[TIES_MAX_MODELS];
    uint32_t stream_id[TIES_MAX_MODELS];
    uint64_t key;
    uint32_t T;                 // keep threshold on the 16-bit draw, 1 .. 65536
    float rescale;              // 1 or fp32(65536 / T)
    const void* base_out; int base_out_dtype;
    int out_is_base0;           // base_out is base[0] in the same dtype and the bases are shared: loaded once
    float lambda;
    int normalize;
    int sign_election;          // 1: dare_ties, 0: dare_linear
    void* out;                  // base_out_dtype, [n]
    float* delta_out;           // optional fp32 [n]: lambda * M
    unsigned long long* kept;   // [k], device: elements kept per finetune
    uint32_t* flags;            // [0]: bit i = finetune i has a non-finite delta
    int chunks;                 // octets per thread
};

template <class Ex>
SM_HD void k_dare_merge(Ex& ex, const DareMergeParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const int nt = ex.nthreads();
    const int k = p.in.k;
    uint32_t* lc = (uint32_t*)(ex.lds() + LDS_SCRATCH_FLOATS);     // [k][nt], then the totals (dare_lds_words)
    kept_zero(ex, st, lc, k);
    ex.each(st, [&](int tid, EmptyState&) {
        uint32_t bad = 0;
        const float Dall = delta_weight_sum(p.alpha, k);
        for (int q = 0; q < p.chunks; ++q) {
            Octet o;
            if (!octet_at(p.in, ex.bid(), nt, p.chunks, tid, q, o)) break;
            float b[8], bo[8];
            delta_base8(p.in, o, b);
            delta_base_out8(p, o, b, bo);
            Election el;
            el.clear();
            for (int i = 0; i < k; ++i) {
                float f[8];
                delta_load8(p.in, i, o, b, f);                             // (elements past n load as 0: never kept)
                const uint32_t mask = dare_mask8(p.key, p.stream_id[i], (uint64_t)o.i0, p.T);
                const float al = p.alpha[i];
                uint32_t nkept = 0;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float d = f[e] - b[e];
                    const uint32_t mag = delta_key(d);
                    if (mag >= TIES_KEY_INF) bad |= 1u << i;
                    const bool kept = ((mask >> e) & 1u) != 0u && mag != 0u;
                    nkept += kept ? 1u : 0u;
                    el.add(e, kept ? aten_fmul_(aten_fmul_(d, p.rescale), al) : 0.f, al, p.sign_election);
                }
                lc[i * nt + tid] += nkept;                                 // this thread's own slot
            }
            float r[8], dl[8];
            el.finish(p.sign_election, p.normalize, Dall, p.lambda, bo, r, dl);
            delta_store8(p, o, r, dl);
        }
        if (bad) ex.global_atomic_or_u32(p.flags, bad);
    });
    kept_fold(ex, st, lc, k, p.kept);
}

// ---- kernel tag (sm_tag.hpp) and this header's share of group 7 of smhip_side.hip (smhip_device.hpp) ----
// the one fused pass, the drop mask from a Philox block per octet in registers
SM_KERNEL_TAG_LB(KDareMerge, DareMergeParams, "dare_merge", k_dare_merge(ex, p), 256, 4)
#define SM_KERNELS_DARE(X) X(KDareMerge)

}  // namespace smhip
