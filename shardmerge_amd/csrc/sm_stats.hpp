// sm_stats.hpp - per-tensor task-vector statistics (smhip_delta_stats; the function is stated in
// include/shardmerge_hip.h): what a trim at up to STATS_MAX_RANKS candidate densities would keep of every finetune, in
// elements and in energy, how the kept sets overlap and how much the TIES election would discard - without writing a
// tensor.  Every value is an integer, an exact order statistic or an fp64 sum in a stated order, so these kernels equal
// a plain restatement bit for bit.
//
//   stats_hist    one radix level for up to TIES_GROUP finetunes at once and ALL ranks of each: crumbs_hist generalised
//                 from two ranks to m.  Level 1: one 2048-bin histogram per finetune serves every rank.  Levels 2 and 3:
//                 a 1024-bin histogram per rank, [q] for the keys under rank q's prefix; a key goes to the FIRST rank
//                 whose prefix it is under, so ranks whose prefixes are still equal share that rank's histogram and the
//                 later ones stay empty.  Equal ranks (duplicate densities, small n) keep equal prefixes to the end and
//                 need no case of their own.  LDS: at most 4 finetunes x 4 ranks x 4 KiB.
//   stats_select  one work-group per finetune walks that level's histogram(s) from the top for every rank; after level 3
//                 tau[q][i] and kept[q][i] are final and stay on the device.
//   stats_pass    the ONE fused pass, organised like geo_gram: a work-group of 256 per 32768-element segment, octet o to
//                 lane o % 256.  The k deltas of an octet are formed once in registers; per density the keep tests, the
//                 k energies in fp64 (the order of geo_gram and sce_energy), the TIES election and the integer counters.
//                 Counters: 8-bit fields packed four to a register (a thread sees at most 128 elements of a segment),
//                 added to the work-group's LDS totals at the end, then one global atomic per non-zero counter and
//                 work-group, as consensus_merge does.  KR = 4 serves k <= 4: the segment is read once, every density's
//                 accumulators and counters in registers.  KR = 16 serves any k (the same source): 16 deltas per octet
//                 leave registers for one density's, so the densities are tiled inside the launch, a sweep each.
//   stats_fold    the segments' energies added in index order, a thread per (density, finetune) (k_geo_fold, sm_geo.hpp).
// The Gram is geo_gram / geo_gram_fold themselves, launched unchanged.
// Tensor passes with a shared base, k <= 4: 3 (K + 1) selection + (K + 1) Gram + (K + 1) stats_pass = 5 (K + 1), whatever m
// (k > 4: geo_gram re-reads per tile of pairs and stats_pass per density).
#pragma once
#include "sm_sce.hpp"

namespace smhip {

constexpr int STATS_MAX_RANKS = 4;                                  // densities per call (SMHIP_STATS_MAX_DENSITIES)
constexpr int STATS_REG_SMALL = 4;                                  // k <= 4: the instantiation with four deltas per octet in registers
constexpr int STATS_HIST_STRIDE = STATS_MAX_RANKS * HIST_LO_BINS;   // 64-bit words per finetune and level in device memory
static_assert(STATS_HIST_STRIDE >= HIST1_BINS, "level 1 needs HIST1_BINS words per finetune");
static_assert(GEO_SEG_ELEMS / GEO_THREADS <= 255, "a thread's 8-bit counter fields hold its share of a segment");

// the integer counters of a call (device memory and a work-group's LDS totals)
constexpr int STATS_NONZERO = 0;                                                        // [16]
constexpr int STATS_OPPOSED = STATS_NONZERO + TIES_MAX_MODELS;                          // [4][16]
constexpr int STATS_ALONE = STATS_OPPOSED + STATS_MAX_RANKS * TIES_MAX_MODELS;          // [4][16]
constexpr int STATS_COVER = STATS_ALONE + STATS_MAX_RANKS * TIES_MAX_MODELS;            // [4][17]
constexpr int STATS_CONFLICT = STATS_COVER + STATS_MAX_RANKS * (TIES_MAX_MODELS + 1);   // [4]
constexpr int STATS_COUNTS = STATS_CONFLICT + STATS_MAX_RANKS;

// the histogram of rank q at levels 2 and 3: that of the first rank with the same prefix
SM_HD int stats_shared_rank(const uint32_t* prefix, int q) {
    for (int r = 0; r < q; ++r)
        if (prefix[r] == prefix[q]) return r;
    return q;
}

struct StatsHistParams {
    TiesInputs in;
    int first, count;           // the finetunes of this launch: first .. first + count - 1, count <= TIES_GROUP
    int level;                  // 1, 2 or 3
    int m;                      // ranks per finetune, 1 .. STATS_MAX_RANKS
    const RadixState* state;    // [k][STATS_MAX_RANKS]
    unsigned long long* hist;   // [k][STATS_HIST_STRIDE] of this level: level 1 [HIST1_BINS], levels 2, 3 [m][HIST_LO_BINS]
    uint32_t* flags;            // [0]: bit i = finetune i has a non-finite delta
    int chunks;                 // octets per thread
};
// LDS words per finetune of a launch
SM_HD int stats_hist_words(int level, int m) { return level == 1 ? HIST1_BINS : m * HIST_LO_BINS; }
template <class Ex>
SM_HD void k_stats_hist(Ex& ex, const StatsHistParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    uint32_t* lh = (uint32_t*)(ex.lds() + LDS_SCRATCH_FLOATS);     // [count][per]
    const int per = stats_hist_words(p.level, p.m);
    hist_zero(ex, st, lh, per * p.count);
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
                uint32_t prefix[STATS_MAX_RANKS];
#pragma unroll
                for (int r = 0; r < STATS_MAX_RANKS; ++r)
                    prefix[r] = (p.level == 1 || r >= p.m) ? 0u : p.state[STATS_MAX_RANKS * i + r].prefix;
                uint32_t* h = lh + j * per;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    if (e < o.cnt) {
                        const uint32_t key = delta_key(f[e] - b[e]);
                        if (p.level == 1) {
                            if (key >= TIES_KEY_INF) bad |= 1u << i;
                            ex.lds_atomic_add(&h[radix_bin(1, key, 0u)], 1u);
                        } else {
                            // the first rank whose prefix the key is under takes it: equal prefixes share that histogram
                            bool taken = false;
#pragma unroll
                            for (int r = 0; r < STATS_MAX_RANKS; ++r) {
                                const int bin = radix_bin(p.level, key, prefix[r]);
                                if (r < p.m && !taken && bin >= 0) { ex.lds_atomic_add(&h[r * HIST_LO_BINS + bin], 1u); taken = true; }
                            }
                        }
                    }
                }
            }
        }
        if (bad) ex.global_atomic_or_u32(p.flags, bad);
    });
    hist_flush(ex, st, lh, per * p.count, [&](int b) { return &p.hist[(size_t)(p.first + b / per) * STATS_HIST_STRIDE + (b % per)]; });
}

// one work-group of TIES_SELECT_THREADS per finetune, every rank
struct StatsSelectParams {
    int level;                                   // 1, 2 or 3
    int m;                                       // ranks, 1 .. STATS_MAX_RANKS
    unsigned long long rank[STATS_MAX_RANKS];    // k_keep of each density (0: that threshold is +inf)
    const unsigned long long* hist;              // [k][STATS_HIST_STRIDE] of this level
    RadixState* state;                           // [k][STATS_MAX_RANKS]
    float* tau;                                  // [STATS_MAX_RANKS][TIES_MAX_MODELS], written after level 3
    unsigned long long* kept;                    // [STATS_MAX_RANKS][TIES_MAX_MODELS]
};
struct StatsSelectState { unsigned long long own[STATS_MAX_RANKS]; };
constexpr size_t STATS_SELECT_LDS = LDS_SCRATCH_FLOATS * 4 + STATS_MAX_RANKS * TIES_SELECT_THREADS * sizeof(unsigned long long);
template <class Ex>
SM_HD void k_stats_select(Ex& ex, const StatsSelectParams& p) {
    typename Ex::template State<StatsSelectState> st;
    ex.init(st);
    unsigned long long* part = (unsigned long long*)(ex.lds() + LDS_SCRATCH_FLOATS);     // [m][TIES_SELECT_THREADS]
    const int i = ex.bid();
    const int nbins = radix_bins(p.level);
    RadixState* s = p.state + STATS_MAX_RANKS * i;
    RadixState s0[STATS_MAX_RANKS];
    uint32_t prefix[STATS_MAX_RANKS];
    const unsigned long long* h[STATS_MAX_RANKS];
#pragma unroll
    for (int r = 0; r < STATS_MAX_RANKS; ++r) {
        s0[r] = radix_start(p.level, p.rank[r], s[r]);         // (ranks past m: copies of rank 0 on zeroed states, never used)
        prefix[r] = s0[r].prefix;
    }
    // level 1, or equal prefixes so far: the ranks read one histogram (stats_hist left the later ones empty)
#pragma unroll
    for (int r = 0; r < STATS_MAX_RANKS; ++r)
        h[r] = p.hist + (size_t)i * STATS_HIST_STRIDE + (p.level == 1 ? 0 : stats_shared_rank(prefix, r) * HIST_LO_BINS);
    ex.each(st, [&](int tid, StatsSelectState& t) {
#pragma unroll
        for (int r = 0; r < STATS_MAX_RANKS; ++r)
            if (r < p.m) part[r * TIES_SELECT_THREADS + tid] = t.own[r] = radix_own_sum(h[r], nbins, tid);
    });
    ex.sync();      // (every thread has read its copy of the states above: the writes below cannot reach those reads)
    ex.each(st, [&](int tid, StatsSelectState& t) {
#pragma unroll
        for (int r = 0; r < STATS_MAX_RANKS; ++r) {
            if (r >= p.m) continue;
            if (p.rank[r] == 0) {     // nothing is kept: no finite magnitude reaches +inf
                if (tid == 0 && p.level == 3) { p.tau[r * TIES_MAX_MODELS + i] = u2f(TIES_KEY_INF); p.kept[r * TIES_MAX_MODELS + i] = 0; }
                continue;
            }
            const RadixFound f = radix_select_step(h[r], nbins, part + r * TIES_SELECT_THREADS, t.own[r], s0[r].rank, tid);
            if (!f.found) continue;
            const RadixState s1 = s[r] = radix_advance(p.level, s0[r], f);
            if (p.level == 3) {                                  // the bin is one key: the threshold; ties at it are all kept
                p.tau[r * TIES_MAX_MODELS + i] = u2f(s1.prefix);
                p.kept[r * TIES_MAX_MODELS + i] = s1.above + (s1.prefix != 0u ? f.c : 0ull);     // a zero delta is never kept
            }
        }
    });
}

struct StatsPassParams {
    TiesInputs in;
    float alpha[TIES_MAX_MODELS];
    int m;                      // densities, 1 .. STATS_MAX_RANKS
    const float* tau;           // [STATS_MAX_RANKS][TIES_MAX_MODELS], device
    size_t nseg;                // segments of GEO_SEG_ELEMS elements
    int seg_vec;                // the pointers are 16-byte aligned (a segment starts at an octet boundary)
    double* part;               // [nseg][m * k]: the energies of each segment, (q, i) at q * k + i
    unsigned long long* counts; // [STATS_COUNTS], device
};
// dynamic LDS beyond the scratch: the tree's [m * k][nt] doubles, then the work-group's STATS_COUNTS totals
SM_HD size_t stats_pass_lds_floats(int m, int k) { return LDS_SCRATCH_FLOATS + (size_t)2 * m * k * GEO_THREADS + STATS_COUNTS; }
// bit i of a 4-bit mask to the 8-bit field i of a word
SM_HD uint32_t stats_spread4(uint32_t bits) { return ((bits & 15u) * 0x204081u) & 0x01010101u; }

// one density of one octet: the energies onto acc[KR], the election, the packed counters of this density
template <int KR>
SM_HD void stats_octet(const StatsPassParams& p, const float (*d)[8], const Octet& o, int q, double* acc, uint32_t* opp, uint32_t* alo, uint32_t* cov) {
    constexpr int NWI = KR / 4, NWC = (KR + 2 + 3) / 4;
    const int k = p.in.k;
    uint32_t tau[KR];
#pragma unroll
    for (int i = 0; i < KR; ++i) tau[i] = i < k ? f2u(p.tau[q * TIES_MAX_MODELS + i]) : 0u;
    // per element: the keep tests, the energies (an entry that is not kept is x = +0: its product +0 leaves the lane as
    // it is), the election and the counts
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        float S = 0.f;
        uint32_t kp = 0, ps = 0, ng = 0;           // bit i: entry i is kept / its tv is > 0 / < 0
#pragma unroll
        for (int i = 0; i < KR; ++i) {
            if (i < k) {
                const float x = d[i][e];
                const uint32_t key = delta_key(x);
                const bool kept = key >= tau[i] && key != 0u;
                if (kept) acc[i] = geo_dadd(acc[i], geo_dmul((double)x, (double)x));
                const float tv = kept ? aten_fmul_(x, p.alpha[i]) : 0.f;
                S = aten_fadd_(S, tv);
                kp |= (kept ? 1u : 0u) << i;
                ps |= (tv > 0.f ? 1u : 0u) << i;
                ng |= (tv < 0.f ? 1u : 0u) << i;
            }
        }
        const uint32_t against = kp & ~(S >= 0.f ? ps : ng);     // kept, and not of the elected sign
        const uint32_t c = (uint32_t)__builtin_popcount(kp);
        const uint32_t only = c == 1u ? kp : 0u;
#pragma unroll
        for (int w = 0; w < NWI; ++w) {
            opp[w] += stats_spread4(against >> (4 * w));
            alo[w] += stats_spread4(only >> (4 * w));
        }
        if (e < o.cnt) {                                         // (an element past the end is kept by nobody, but is no element)
#pragma unroll
            for (int w = 0; w < NWC; ++w)
                if ((int)(c >> 2) == w) cov[w] += 1u << (8 * (c & 3u));
        }
        cov[(KR + 1) >> 2] += ((ps != 0u && ng != 0u) ? 1u : 0u) << (8 * ((KR + 1) & 3));
    }
}
// field f of words of four 8-bit fields
SM_HD uint32_t stats_field(const uint32_t* w, int f) { return (w[f >> 2] >> (8 * (f & 3))) & 0xffu; }
// a thread's fields of density q to the work-group's totals cnt, its energies to the tree's array red
template <int KR, class Ex>
SM_HD void stats_flush(Ex& ex, int k, int q, int nt, int tid, const double* acc, const uint32_t* opp, const uint32_t* alo, const uint32_t* cov,
                       double* red, uint32_t* cnt) {
#pragma unroll
    for (int i = 0; i < KR; ++i) {
        if (i < k) {
            const uint32_t vo = stats_field(opp, i), va = stats_field(alo, i);
            if (vo) ex.lds_atomic_add(&cnt[STATS_OPPOSED + q * TIES_MAX_MODELS + i], vo);
            if (va) ex.lds_atomic_add(&cnt[STATS_ALONE + q * TIES_MAX_MODELS + i], va);
            red[((size_t)q * k + i) * nt + tid] = acc[i];
        }
    }
#pragma unroll
    for (int c = 0; c <= KR; ++c) {
        const uint32_t v = stats_field(cov, c);
        if (c <= k && v) ex.lds_atomic_add(&cnt[STATS_COVER + q * (TIES_MAX_MODELS + 1) + c], v);
    }
    const uint32_t vc = stats_field(cov, KR + 1);
    if (vc) ex.lds_atomic_add(&cnt[STATS_CONFLICT + q], vc);
}

template <int KR, class Ex>
SM_HD void k_stats_pass(Ex& ex, const StatsPassParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    constexpr int MR = STATS_MAX_RANKS;
    // k <= 4: the segment is read once, every density's accumulators and counters in registers.  Any k: 16 deltas per
    // octet leave registers for one density's, so the densities are tiled inside the launch - a sweep of the segment each
    constexpr bool TILE_Q = KR > STATS_REG_SMALL;
    constexpr int NWI = KR / 4;                                    // words of four 8-bit fields: a field per finetune
    constexpr int NWC = (KR + 2 + 3) / 4;                          // cover[0 .. KR], then conflict
    const int nt = ex.nthreads();                                  // GEO_THREADS
    const int k = p.in.k, m = p.m;
    const size_t seg = (size_t)ex.bid();
    double* red = (double*)(ex.lds() + LDS_SCRATCH_FLOATS);        // [m * k][nt] (LDS_SCRATCH_FLOATS is even)
    uint32_t* cnt = (uint32_t*)(red + (size_t)m * k * nt);         // [STATS_COUNTS]
    const size_t start = seg * GEO_SEG_ELEMS;
    const size_t len = p.in.n - start < GEO_SEG_ELEMS ? p.in.n - start : GEO_SEG_ELEMS;
    ex.each(st, [&](int tid, EmptyState&) { for (int c = tid; c < STATS_COUNTS; c += nt) cnt[c] = 0; });
    ex.sync();
    ex.each(st, [&](int tid, EmptyState&) {
        uint32_t nzc[NWI];
#pragma unroll
        for (int w = 0; w < NWI; ++w) nzc[w] = 0u;
        // nonzero[i] of an octet (an element past the end is +0)
        auto count_nonzero = [&](const float (*d)[8]) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                uint32_t nz = 0;
#pragma unroll
                for (int i = 0; i < KR; ++i)
                    if (i < k) nz |= (d[i][e] != 0.f ? 1u : 0u) << i;
#pragma unroll
                for (int w = 0; w < NWI; ++w) nzc[w] += stats_spread4(nz >> (4 * w));
            }
        };
        constexpr int QR = TILE_Q ? 1 : MR;                        // densities held at once
        for (int q0 = 0; q0 < (TILE_Q ? m : 1); q0 += QR) {
            double acc[QR][KR];
            uint32_t opp[QR][NWI], alo[QR][NWI], cov[QR][NWC];
#pragma unroll
            for (int r = 0; r < QR; ++r) {
#pragma unroll
                for (int i = 0; i < KR; ++i) acc[r][i] = 0.0;
#pragma unroll
                for (int w = 0; w < NWI; ++w) { opp[r][w] = 0u; alo[r][w] = 0u; }
#pragma unroll
                for (int w = 0; w < NWC; ++w) cov[r][w] = 0u;
            }
            for (size_t oq = tid; oq < segment_octets(len); oq += nt) {
                const Octet o = segment_octet(start, len, p.seg_vec, oq);
                float d[KR][8];
                uint32_t bad = 0;                                  // (stats_hist and geo_gram raise the flags)
                sce_delta8<KR>(p.in, o, d, bad);
                if (q0 == 0) count_nonzero(d);
#pragma unroll
                for (int r = 0; r < QR; ++r)
                    if (q0 + r < m) stats_octet<KR>(p, d, o, q0 + r, acc[r], opp[r], alo[r], cov[r]);
            }
#pragma unroll
            for (int r = 0; r < QR; ++r)
                if (q0 + r < m) stats_flush<KR>(ex, k, q0 + r, nt, tid, acc[r], opp[r], alo[r], cov[r], red, cnt);
        }
#pragma unroll
        for (int i = 0; i < KR; ++i)
            if (i < k) { const uint32_t v = stats_field(nzc, i); if (v) ex.lds_atomic_add(&cnt[STATS_NONZERO + i], v); }
    });
    ex.sync();
    // the fixed binary tree of geo_gram: p[t] = p[t] + p[t + s] for t < s, s = nt / 2, nt / 4, ..., 1
    for (int s = nt >> 1; s > 0; s >>= 1) {
        ex.each(st, [&](int tid, EmptyState&) {
            if (tid >= s) return;
            for (int j = 0; j < m * k; ++j) {
                double* v = red + (size_t)j * nt;
                v[tid] = geo_dadd(v[tid], v[tid + s]);
            }
        });
        ex.sync();
    }
    ex.each(st, [&](int tid, EmptyState&) {
        if (tid < m * k) p.part[seg * (size_t)(m * k) + tid] = red[(size_t)tid * nt];
        for (int c = tid; c < STATS_COUNTS; c += nt)
            if (cnt[c]) ex.global_atomic_add(&p.counts[c], (unsigned long long)cnt[c]);
    });
}

// ---- kernel tags (sm_tag.hpp) and group 8 of smhip_side.hip (smhip_device.hpp) ----
// the m-rank radix level and its scan, the one fused pass over the k deltas of an octet (k <= 4 with every density in
// registers, or up to 16 with the densities tiled), the fold of its energies (the fold of sm_geo.hpp under its own
// profile name, a row of k per rank at the report's pitch)
SM_KERNEL_TAG_LB(KStatsHist, StatsHistParams, "stats_hist", k_stats_hist(ex, p), 256, 4)
SM_KERNEL_TAG_LB(KStatsSelect, StatsSelectParams, "stats_select", k_stats_select(ex, p), TIES_SELECT_THREADS, 4)
SM_KERNEL_TAG_LB(KStatsPass, StatsPassParams, "stats_pass", k_stats_pass<STATS_REG_SMALL>(ex, p), GEO_THREADS, 2)
SM_KERNEL_TAG_LB(KStatsPassAny, StatsPassParams, "stats_pass", k_stats_pass<TIES_MAX_MODELS>(ex, p), GEO_THREADS, 1)
SM_KERNEL_TAG_LB(KStatsFold, GeoFoldParams, "stats_fold", k_geo_fold(ex, p), 256, 4)
#define SM_SIDE_KERNELS_8(X) X(KStatsHist) X(KStatsSelect) X(KStatsPass) X(KStatsPassAny) X(KStatsFold)

}  // namespace smhip
