// sm_cabs.hpp - CABS merge (Yang et al. 2025, "CABS: Conflict-Aware and Balanced Sparsification for Enhancing Model
// Merging", as recalled: PAPERS.md), an operator the reference does not have.  The function is stated in
// include/shardmerge_hip.h (smhip_cabs_merge); every step of it is an integer function, an exact order statistic or one
// correctly rounded fp32 operation, so the kernel equals a plain restatement of it bit for bit.
//
//   cabs_merge   the one fused streaming pass.  The tensor is R rows of C elements; a lane works on a ROW OCTET, columns
//                [c0, c0 + 8) of one row with c0 a multiple of 8, so an octet never leaves its group (group M >= 8) or holds
//                exactly two (M == 4).  The L = max(M, 8) / 8 lanes of a group are a TEAM: teams are numbered by the global
//                group number r * G + g, L divides the work-group, so a team never leaves its work-group or (L <= 64) its
//                wave.  The k deltas of the octet stay in registers (KR = 4: 32 of them, KR = 16: 128, the same source);
//                the finetunes are selected one after another, the kept bits of the earlier ones mask the candidates of
//                the later ones.
//                The selection of one finetune in one group is "kept iff fewer than q candidates are strictly larger":
//                  L == 1  counted in the lane, 8 x 8 comparisons, no LDS, no barrier;
//                  L >= 2  tau, the q-th largest candidate key, by a digit descent over the 31 magnitude bits: 3 bits,
//                          then 7 x 4.  A level: every lane counts its keys under the prefix in a register (16 x 4 bits)
//                          and adds them to the team's 16 bins in LDS, two 16-bit bins to a word and an atomic per
//                          word it has keys in (magnitudes share their leading digits: one atomic, not eight), ONE
//                          barrier, every lane of the team scans the same bins.  Three histograms rotate (phase p
//                          fills p % 3 and clears (p + 2) % 3, last read before the barrier of p), so a level costs one
//                          barrier: 8 per tile and finetune.
//                Counters: kept[i] a slot per (finetune, thread) in LDS folded by kept_fold; short groups and surplus by
//                the team's first lane, covered and overlap per lane, into the work-group's LDS totals, then one 64-bit
//                global atomic per counter and work-group.
#pragma once
#include "sm_delta.hpp"

namespace smhip {

constexpr int CABS_REG_SMALL = 4;                                 // k <= 4: the instantiation with 32 delta registers
constexpr int CABS_THREADS = 256;
constexpr int CABS_MIN_GROUP = 4, CABS_MAX_GROUP = 512;
constexpr int CABS_LEVELS = 8;                                    // digits of the descent: bits 30..28, then 27..24, ..., 3..0
constexpr int CABS_BINS = 16;
constexpr int CABS_WORDS = CABS_BINS / 2;                         // a team's histogram in LDS: two 16-bit counts (at most 512) per word
constexpr int CABS_COUNTS = 2 * TIES_MAX_MODELS + 2;              // short[16], surplus[16], covered, overlap

struct CabsMergeParams {
    TiesInputs in;
    float alpha[TIES_MAX_MODELS];
    const void* base_out; int base_out_dtype;
    int out_is_base0;           // base_out is base[0] in the same dtype and the bases are shared: loaded once
    float lambda;
    void* out;                  // base_out_dtype, [n]
    float* delta_out;           // optional fp32 [n]: lambda * M
    uint16_t* mask_out;         // optional [n]: bit i = finetune i kept the element
    size_t R, C;                // n = R * C
    size_t G;                   // groups of max(M, 8) columns per row
    size_t units;               // R * G * L row octets, the idle ones of a tail group included
    int M, N, L, log2L;         // group, n_keep, lanes per team
    int conflict_aware;
    int row_vec;                // C % 8 == 0 and every pointer is 16-byte aligned: every row octet is a 16-byte access
    unsigned long long* kept;   // [k], device
    unsigned long long* counts; // [CABS_COUNTS], device
    uint32_t* flags;            // [0]: bit i = finetune i has a non-finite delta
    int chunks;                 // tiles (row octets per thread) per work-group
};
// dynamic LDS beyond the scratch: the three rotating histograms of the work-group's teams (none when L == 1), the kept
// counters (dare_lds_words), the work-group's CABS_COUNTS totals
SM_HD size_t cabs_hist_words(int L, int nthreads) { return L == 1 ? 0 : (size_t)3 * (nthreads / L) * CABS_WORDS; }
SM_HD size_t cabs_lds_words(int k, int L, int nthreads) { return cabs_hist_words(L, nthreads) + dare_lds_words(k, nthreads) + CABS_COUNTS; }
// the quota of a group of mlen columns: ceil(N * mlen / M)
SM_HD uint32_t cabs_quota(int N, int M, uint32_t mlen) { return ((uint32_t)N * mlen + (uint32_t)M - 1u) / (uint32_t)M; }

template <int KR>
struct CabsState {
    float d[KR][8], bo[8];
    uint32_t key[8];            // the current finetune's candidate keys, 0: no candidate
    uint32_t km[KR / 4];        // kept bits: a byte per finetune, bit e = element e
    uint32_t prefix, rank, above, eq;
    uint32_t q[2];              // the quota of the octet's group (M == 4: of its two groups; 0: the group does not exist)
    uint32_t ncov, novl, bad;
    Octet o;
    bool valid, lead, all;
};

template <int KR, class Ex>
SM_HD void k_cabs_merge(Ex& ex, const CabsMergeParams& p) {
    using S = CabsState<KR>;
    typename Ex::template State<S> st;
    ex.init(st);
    const int nt = ex.nthreads();
    const int k = p.in.k, L = p.L, M = p.M;
    const int teams = nt / L;
    uint32_t* hist = (uint32_t*)(ex.lds() + LDS_SCRATCH_FLOATS);      // [3][teams][CABS_WORDS]
    uint32_t* lc = hist + cabs_hist_words(L, nt);                     // [k][nt], then the totals (dare_lds_words)
    uint32_t* ct = lc + dare_lds_words(k, nt);                        // [CABS_COUNTS]
    const int nhist = (int)cabs_hist_words(L, nt);
    ex.each(st, [&](int tid, S& s) {
        for (int b = tid; b < nhist; b += nt) hist[b] = 0;
        if (tid < CABS_COUNTS) ct[tid] = 0;
        s.ncov = 0; s.novl = 0; s.bad = 0;
    });
    kept_zero(ex, st, lc, k);                                         // (ends with the barrier)
    uint32_t phase = 0;                                               // levels run so far, by every lane alike
    for (int t = 0; t < p.chunks; ++t) {
        const size_t u0 = ((size_t)ex.bid() * p.chunks + t) * nt;     // the tile's first row octet
        if (u0 >= p.units) break;                                     // (the whole work-group leaves)
        // the lane's row octet: its deltas into registers, base_out once
        ex.each(st, [&](int tid, S& s) {
            const size_t u = u0 + tid;
            const size_t gi = u >> p.log2L;
            const size_t r = p.units <= 0xffffffffull ? (size_t)((uint32_t)gi / (uint32_t)p.G) : gi / p.G, g = gi - r * p.G;
            const size_t Mu = (size_t)(M < 8 ? 8 : M);
            const size_t c0 = g * Mu + 8 * (u - gi * (size_t)L);
            s.valid = u < p.units && c0 < p.C;
            s.lead = u < p.units && u == gi * (size_t)L;
#pragma unroll
            for (int w = 0; w < KR / 4; ++w) s.km[w] = 0;
            s.q[0] = s.q[1] = 0;
            if (!s.valid) {
#pragma unroll
                for (int e = 0; e < 8; ++e) s.key[e] = 0;
                return;
            }
            const size_t i0 = r * p.C + c0;
            const int cnt = (int)((p.C - c0) < 8 ? (p.C - c0) : 8);
            s.o = Octet{i0 >> 3, i0, 0, cnt, p.row_vec != 0};
            if (M == 4) {
                s.q[0] = cabs_quota(p.N, M, (uint32_t)(cnt < 4 ? cnt : 4));
                s.q[1] = cnt > 4 ? cabs_quota(p.N, M, (uint32_t)(cnt - 4)) : 0u;
            } else {
                const size_t gl = p.C - g * Mu;
                s.q[0] = cabs_quota(p.N, M, (uint32_t)(gl < Mu ? gl : Mu));
            }
            float b[8];
            delta_base8(p.in, s.o, b);
            delta_base_out8(p, s.o, b, s.bo);
#pragma unroll
            for (int i = 0; i < KR; ++i) {
                if (i < k) {
                    float f[8];
                    delta_load8(p.in, i, s.o, b, f);
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        s.d[i][e] = f[e] - b[e];
                        if (delta_key(s.d[i][e]) >= TIES_KEY_INF) s.bad |= 1u << i;
                    }
                }
            }
        });
        // the finetunes in order
        static_for<0, KR>([&](auto i_c) {
            constexpr int i = decltype(i_c)::value;
            if (i >= k) return;
            // candidates: non-zero and, under CA, kept by no earlier finetune
            ex.each(st, [&](int tid, S& s) {
                if (!s.valid) return;
                uint32_t taken = 0;
                if (p.conflict_aware) {
#pragma unroll
                    for (int w = 0; w < KR / 4; ++w) taken |= s.km[w];
                    taken |= taken >> 16; taken |= taken >> 8;
                }
#pragma unroll
                for (int e = 0; e < 8; ++e) s.key[e] = ((taken >> e) & 1u) ? 0u : delta_key(s.d[i][e]);
            });
            if (L == 1) {
                // in the lane: kept iff fewer than q candidates of its group are strictly larger
                ex.each(st, [&](int tid, S& s) {
                    if (!s.valid) return;
                    uint32_t bits = 0, nshort = 0, nsur = 0;
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const uint32_t q = s.q[h];
                        if (!q) continue;                             // (M >= 8: one group; M == 4: its second one may not exist)
                        uint32_t c = 0, kc = 0;
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            const bool mine = M == 4 ? (e >> 2) == h : true;
                            uint32_t gt = 0;
#pragma unroll
                            for (int e2 = 0; e2 < 8; ++e2) {
                                const bool same = M == 4 ? (e2 >> 2) == h : true;
                                gt += (same && s.key[e2] > s.key[e]) ? 1u : 0u;
                            }
                            const bool cand = mine && s.key[e] != 0u;
                            const bool kp = cand && gt < q;
                            c += cand ? 1u : 0u; kc += kp ? 1u : 0u;
                            bits |= kp ? 1u << e : 0u;
                        }
                        nshort += c < q ? 1u : 0u;
                        nsur += kc > q ? kc - q : 0u;
                    }
                    s.km[i / 4] |= bits << (8 * (i % 4));
                    lc[i * nt + tid] += (uint32_t)__builtin_popcount(bits);
                    if (nshort) ex.lds_atomic_add(&ct[i], nshort);
                    if (nsur) ex.lds_atomic_add(&ct[TIES_MAX_MODELS + i], nsur);
                });
                return;
            }
            // the team's digit descent to tau, the q-th largest candidate key (1 when there are fewer than q)
            ex.each(st, [&](int tid, S& s) { s.prefix = 0; s.rank = s.q[0]; s.above = 0; s.eq = 0; s.all = false; });
            for (int level = 0; level < CABS_LEVELS; ++level, ++phase) {
                const int shift = 28 - 4 * level;
                uint32_t* hfill = hist + (size_t)(phase % 3) * teams * CABS_WORDS;
                uint32_t* hclear = hist + (size_t)((phase + 2) % 3) * teams * CABS_WORDS;
                ex.each(st, [&](int tid, S& s) {
                    if (!s.valid || s.all) return;
                    uint32_t* h = hfill + (size_t)(tid / L) * CABS_WORDS;
                    unsigned long long pk = 0;                        // the lane's own 16 counts, 4 bits each (at most 8)
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const uint32_t key = s.key[e];
                        const bool under = level == 0 || (key >> (shift + 4)) == s.prefix;
                        if (key != 0u && under) pk += 1ull << (4 * ((key >> shift) & 15u));
                    }
#pragma unroll
                    for (int w = 0; w < CABS_WORDS; ++w) {            // one atomic per word of two bins the lane has keys in
                        const uint32_t two = (uint32_t)(pk >> (8 * w)) & 0xffu;
                        if (two) ex.lds_atomic_add(&h[w], (two & 15u) | ((two >> 4) << 16));
                    }
                });
                ex.sync();
                ex.each(st, [&](int tid, S& s) {
                    const int team = tid / L, j = tid - team * L;
                    for (int w = j; w < CABS_WORDS; w += L) hclear[(size_t)team * CABS_WORDS + w] = 0;
                    if (!s.valid || s.all) return;
                    const uint32_t* h = hfill + (size_t)team * CABS_WORDS;
                    uint32_t higher = 0, bin = 0, c = 0;
                    bool found = false;
#pragma unroll
                    for (int b = CABS_BINS - 1; b >= 0; --b) {
                        const uint32_t v = (h[b >> 1] >> (16 * (b & 1))) & 0xffffu;
                        if (!found && higher + v >= s.rank) { found = true; bin = (uint32_t)b; c = v; }
                        if (!found) higher += v;
                    }
                    if (!found) { s.all = true; s.prefix = 1u; s.above = higher; s.eq = 0; return; }    // (level 0 only: fewer than q candidates)
                    s.prefix = (s.prefix << 4) | bin; s.rank -= higher; s.above += higher; s.eq = c;
                });
            }
            ex.each(st, [&](int tid, S& s) {
                if (s.lead) {
                    if (s.all && s.above < s.q[0]) ex.lds_atomic_add(&ct[i], 1u);
                    const uint32_t kc = s.above + s.eq;
                    if (!s.all && kc > s.q[0]) ex.lds_atomic_add(&ct[TIES_MAX_MODELS + i], kc - s.q[0]);
                }
                if (!s.valid) return;
                uint32_t bits = 0;
#pragma unroll
                for (int e = 0; e < 8; ++e) bits |= (s.key[e] != 0u && s.key[e] >= s.prefix) ? 1u << e : 0u;
                s.km[i / 4] |= bits << (8 * (i % 4));
                lc[i * nt + tid] += (uint32_t)__builtin_popcount(bits);
            });
        });
        // the weighted sum of the kept entries, the add-back, the stores
        ex.each(st, [&](int tid, S& s) {
            if (!s.valid) return;
            float Msum[8];
            uint32_t mk[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) { Msum[e] = 0.f; mk[e] = 0; }
#pragma unroll
            for (int i = 0; i < KR; ++i) {
                if (i < k) {
                    const uint32_t bits = (s.km[i / 4] >> (8 * (i % 4))) & 0xffu;
                    const float al = p.alpha[i];
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const bool kp = (bits >> e) & 1u;
                        Msum[e] = aten_fadd_(Msum[e], kp ? aten_fmul_(s.d[i][e], al) : 0.f);
                        mk[e] |= kp ? 1u << i : 0u;
                    }
                }
            }
            float r[8], dl[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                dl[e] = aten_fmul_(p.lambda, Msum[e]);
                r[e] = aten_fadd_(s.bo[e], dl[e]);
                s.ncov += mk[e] ? 1u : 0u;
                s.novl += (mk[e] & (mk[e] - 1u)) ? 1u : 0u;
            }
            const Octet& o = s.o;
            if (o.vec) {
                delta_store8(p, o, r, dl);
                if (p.mask_out) {
                    u32x4 w;
                    w.x = mk[0] | (mk[1] << 16); w.y = mk[2] | (mk[3] << 16); w.z = mk[4] | (mk[5] << 16); w.w = mk[6] | (mk[7] << 16);
                    ((u32x4*)p.mask_out)[o.oi] = w;
                }
            } else {                                                  // a row octet that starts anywhere: element by element
                for (int e = 0; e < o.cnt; ++e) {
                    if (p.delta_out) p.delta_out[o.i0 + e] = dl[e];
                    if (p.base_out_dtype == DT_F32) ((float*)p.out)[o.i0 + e] = r[e];
                    else ((uint16_t*)p.out)[o.i0 + e] = p.base_out_dtype == DT_BF16 ? f_to_bf16_any(r[e]) : f_to_f16_any(r[e]);
                    if (p.mask_out) p.mask_out[o.i0 + e] = (uint16_t)mk[e];
                }
            }
        });
    }
    ex.each(st, [&](int tid, S& s) {
        if (s.ncov) ex.lds_atomic_add(&ct[2 * TIES_MAX_MODELS], s.ncov);
        if (s.novl) ex.lds_atomic_add(&ct[2 * TIES_MAX_MODELS + 1], s.novl);
        if (s.bad) ex.global_atomic_or_u32(p.flags, s.bad);
    });
    kept_fold(ex, st, lc, k, p.kept);                                 // (starts with the barrier the totals in ct need too)
    ex.each(st, [&](int tid, S&) {
        if (tid < CABS_COUNTS && ct[tid]) ex.global_atomic_add(&p.counts[tid], (unsigned long long)ct[tid]);
    });
}

// ---- kernel tags (sm_tag.hpp) and group 14 of smhip_side.hip (smhip_device.hpp) ----
// the one fused pass with the k deltas of a row octet in registers across the sequential n:m selections of the finetunes;
// k <= 4 at dare_merge's residency, or up to 16
SM_KERNEL_TAG_LB(KCabsMerge, CabsMergeParams, "cabs_merge", k_cabs_merge<CABS_REG_SMALL>(ex, p), CABS_THREADS, 4)
SM_KERNEL_TAG_LB(KCabsMergeAny, CabsMergeParams, "cabs_merge_any", k_cabs_merge<TIES_MAX_MODELS>(ex, p), CABS_THREADS, 2)
#define SM_SIDE_KERNELS_14(X) X(KCabsMerge) X(KCabsMergeAny)

}  // namespace smhip
