// sm_select.hpp - the selection and reduction kernels of the spectral-merge pipeline: the exact k-th order statistic
// by three radix levels (histogram, scan, candidate lists), the masked slerp sums and constants, the class norm
// statistics, and the mailbox the host reads results from.  Where they stand in a pair merge: sm_kernels.hpp.
#pragma once
#include "sm_common.hpp"
#include "sm_tag.hpp"

namespace smhip {

// =====================================================================
// streaming kernels over the half-spectrum planes [Cb][R]
// =====================================================================
// selection state (device memory): exact k-th smallest key by radix levels
struct SelState {
    unsigned long long rank;    // in: 0-based rank wanted; updated to rank within the prefix
    uint32_t prefix;            // key bits decided so far
    uint32_t level;             // levels done
    float value;                // final: the k-th smallest |x|
    uint32_t pad;
};

struct HistParams {
    const float* X; const float* Y;     // Y may be null
    int R, C, Cb;
    int vec4;                           // R % 4 == 0: float4 loads, one weight per quad
    int level;                          // 1, 2 or 3
    const SelState* sel;
    unsigned long long* hist;
    int chunks;                         // quads per thread
    const uint32_t* only_if;            // when set: run only if *only_if != 0 (fallback after a list overflow)
};

// load up to 4 consecutive plane values starting at element i0
SM_HD int load_quad(const float* src, size_t i0, size_t total, int vec4, float* out) {
    if (vec4) {
        const cf4 v = *(const cf4*)(src + i0);
        out[0] = v.x; out[1] = v.y; out[2] = v.z; out[3] = v.w;
        return 4;
    }
    int n = 0;
    for (int e = 0; e < 4; ++e) {
        if (i0 + e < total) { out[e] = src[i0 + e]; n = e + 1; } else out[e] = 0.f;
    }
    return n;
}

template <class Ex>
SM_HD void k_hist(Ex& ex, const HistParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    uint32_t* lh = (uint32_t*)(ex.lds() + LDS_SCRATCH_FLOATS);
    const int nt = ex.nthreads();
    const int nbins = p.level == 1 ? HIST1_BINS : HIST_LO_BINS;
    const size_t total = (size_t)p.Cb * p.R;
    const size_t nquad = (total + 3) / 4;
    if (p.only_if && !*p.only_if) return;
    const uint32_t prefix = p.sel->prefix;
    const WeightRanges wr = weight_ranges(p.R, p.C, p.Cb);
    ex.each(st, [&](int tid, EmptyState&) { for (int b = tid; b < nbins; b += nt) lh[b] = 0; });
    ex.sync();
    ex.each(st, [&](int tid, EmptyState&) {
        const size_t start = (size_t)ex.bid() * p.chunks * nt;
        for (int c = 0; c < p.chunks; ++c) {
            const size_t qi = start + (size_t)c * nt + tid;
            if (qi >= nquad) break;
            const size_t i0 = 4 * qi;
            for (int which = 0; which < 2; ++which) {
                const float* src = which ? p.Y : p.X;
                if (!src) continue;
                float v[4];
                const int n = load_quad(src, i0, total, p.vec4, v);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (e < n) {
                        const uint32_t w = weight_at(wr, i0 + e);
                        const uint32_t key = f2u(v[e]) & 0x7fffffffu;
                        if (p.level == 1) ex.lds_atomic_add(&lh[key >> 20], w);
                        else if (p.level == 2) { if ((key >> 20) == prefix) ex.lds_atomic_add(&lh[(key >> 10) & 1023u], w); }
                        else { if ((key >> 10) == prefix) ex.lds_atomic_add(&lh[key & 1023u], w); }
                    }
                }
            }
        }
    });
    ex.sync();
    ex.each(st, [&](int tid, EmptyState&) {
        for (int b = tid; b < nbins; b += nt) {
            const uint32_t v = lh[b];
            if (v) ex.global_atomic_add(&p.hist[b], (unsigned long long)v);
        }
    });
}

// ---------------------------------------------------------------------------
// Level-2 selection pass with candidate compaction (and, for the cutoff
// threshold, the masked slerp sums fused in).
//
// After level 1 the k-th smallest key is known to lie in bin B1 = sel->prefix
// (key >> 20).  One streaming pass over the plane(s)
//   * histograms bits [19:10] of the keys in B1 (as k_hist level 2 does), and
//   * appends those keys (~1 % of the data) to a candidate list, so that level 3
//     runs on the list instead of re-reading the planes;
//   * with `fuse_reduce`: accumulates the slerp-class sums over every bin whose
//     class does not depend on the exact threshold (|r1|'s level-1 bin above B1),
//     and appends the undecided bins (|r1| in B1, signs agree) to a pair list that
//     k_reduce_cand settles once the threshold is known.
// Lists are staged in LDS and appended with one global atomic per work-group.
// Any overflow (staging or list capacity) raises *overflow; the caller then
// falls back to the plain full passes (k_hist level 3 / k_reduce), which exit
// immediately otherwise.
// ---------------------------------------------------------------------------
constexpr int STAGE_KEYS = 2048;     // per work-group staging (expected ~160 keys / ~40 pairs)
constexpr int STAGE_PAIRS = 1024;
struct CandLists {
    uint32_t* keys;        // key | (weight-1) << 31
    cf4* pairs;            // (r0, r1, weight, 0)
    uint32_t cap_keys, cap_pairs;
    uint32_t* counters;    // [0] n_keys, [1] n_pairs, [2] overflow
};
// blend constants (device memory), written by k_slerp_consts
struct Select2Params {
    const float* X; const float* Y;     // Y may be null
    int R, C, Cb;
    int vec4;
    SelState* sel;                      // written by work-group 0: level-1 bin and rank inside it
    const unsigned long long* hist1;    // level-1 histogram (HIST1_BINS), complete
    unsigned long long rank;            // 0-based rank wanted
    unsigned long long* hist;           // level-2 histogram (HIST_LO_BINS), accumulated here
    CandLists cand;
    int fuse_reduce;                    // needs Y: X = Re a, Y = Re b
    int sumsq;                          // Y == null: partials[4*wg] += sum w x^2 over the elements whose level-1 bin lies
                                        // ABOVE the threshold's (they survive the cull whatever its low bits): the
                                        // Parseval norm of a spectral intermediate, fused into the cull selection
    double* partials;                   // [grid][4] when fuse_reduce or sumsq
    int chunks;
    int flush_always;          // test hook: flush the staged candidates after every round
    const uint32_t* skip;      // plain mode, optional: *skip != 0 -> nothing to do (the speculative pass below did it)
    // BLEND mode (k_select2<true>): X = Re a, blendB = Re b; the kernel computes Re R = blend(a, b), stores it,
    // takes its level-1 histogram - and, SPECULATING that the cull threshold's level-1 bin is *guess - 1 (what
    // it was the last time, 0 = no guess), does this selection pass's work on it in the same sweep.
    // k_spec_check confirms the guess from the complete histogram or voids the speculative output.
    const float* blendB; float* blendR;
    const BlendConsts* consts; float t_sum;
    unsigned long long* hist1_out;
    const uint32_t* guess;
};

template <bool BLEND = false, class Ex>
SM_HD void k_select2(Ex& ex, const Select2Params& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    uint32_t* lh = (uint32_t*)(ex.lds() + LDS_SCRATCH_FLOATS);
    uint32_t* lctl = lh + HIST_LO_BINS;                 // [0] nkeys [1] npairs [2] base keys [3] base pairs [4..6] resolve
    uint32_t* lkeys = lctl + 8;
    cf4* lpairs = (cf4*)(lkeys + STAGE_KEYS);
    const int nt = ex.nthreads();
    const size_t total = (size_t)p.Cb * p.R;
    const size_t nquad = (total + 3) / 4;
    uint32_t* lh1 = lkeys + STAGE_KEYS;                 // BLEND: level-1 histogram of Re R (no pair staging there)
    uint32_t prefix;
    BlendConsts bc;
    if constexpr (BLEND) {
        prefix = *p.guess - 1u;                          // 0xffffffff: no guess, nothing matches
        bc = *p.consts;
    } else {
        if (p.skip && *p.skip) return;
        // level 1: every work-group resolves it for itself (the staging area doubles as scratch)
        wg_resolve(ex, st, p.hist1, HIST1_BINS, p.rank, (unsigned long long*)lkeys, lctl + 4);
        prefix = lctl[4];
        if (ex.bid() == 0) {
            ex.each(st, [&](int tid, EmptyState&) {
                if (tid == 0) {
                    p.sel->prefix = prefix; p.sel->level = 1;
                    p.sel->rank = (unsigned long long)lctl[5] | ((unsigned long long)lctl[6] << 32);
                }
            });
        }
        ex.sync();
    }
    const WeightRanges wr = weight_ranges(p.R, p.C, p.Cb);
    ex.each(st, [&](int tid, EmptyState&) {
        for (int b = tid; b < HIST_LO_BINS; b += nt) lh[b] = 0;
        if (tid < 8) lctl[tid] = 0;
        if constexpr (BLEND) for (int b = tid; b < HIST1_BINS; b += nt) lh1[b] = 0;
    });
    ex.sync();
    // The stream is cut into rounds of ROUND steps; after each round the staged candidates go
    // to the global lists, so a work-group's staging area only has to hold one round's worth
    // (a 235 M-element tensor used to overflow it - and redo the whole layer in safe mode)
#ifndef SM_SEL_ROUND
#define SM_SEL_ROUND 16
#endif
#ifndef SM_SEL_U
#define SM_SEL_U 4
#endif
#ifndef SM_DIAG_SEL
#define SM_DIAG_SEL 0          // diagnostic builds: bit 0 drops the staging path, bit 1 the sums
#endif
    constexpr int ROUND = SM_SEL_ROUND;
    ex.each(st, [&](int, EmptyState& s) { s.red[0] = s.red[1] = s.red[2] = s.red[3] = 0.0; });
    for (int r0 = 0; r0 < p.chunks; r0 += ROUND) {
    const int r1 = (r0 + ROUND < p.chunks) ? r0 + ROUND : p.chunks;
    ex.each(st, [&](int tid, EmptyState& s) {
        double s00 = 0, s01 = 0, s11 = 0, cnt = 0;
        const size_t start = (size_t)ex.bid() * p.chunks * nt;
        const bool hasY = !BLEND && p.Y != nullptr;
        // up to 4 consecutive plane elements from i0 on
        // uniform_w: the 4 elements lie in one column (R % 4 == 0), one weight serves all
        auto quad = [&](size_t i0, const float* a_in, const float* b, int n, bool uniform_w) {
            float q00 = 0.f, q01 = 0.f, q11 = 0.f, qc = 0.f;
            const uint32_t w0 = weight_at(wr, i0);
            float rr[4];
            const float* a = a_in;
            if constexpr (BLEND) {
#pragma unroll
                for (int e = 0; e < 4; ++e) rr[e] = blend_slerp_one(bc, p.t_sum, a_in[e], b[e]);
                if (n == 4 && uniform_w) { cf4 v = {rr[0], rr[1], rr[2], rr[3]}; *(cf4*)(p.blendR + i0) = v; }
                else for (int e = 0; e < n; ++e) p.blendR[i0 + e] = rr[e];
                a = rr;
            }
            // keys of the selected level-1 bin: lo <= key < lo + 2^20, i.e. (key - lo) < 2^20 unsigned; above it: key >= hi
            // (prefix 0xffffffff - no guess - gives lo = 0xfff00000, which no 31-bit key reaches from either side)
            const uint32_t lo = prefix << 20, hi = lo + (1u << 20);
            const bool has_hi = prefix < 2047u;
            uint32_t ka[4], kb[4], wv[4];
            bool hit = false;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                wv[e] = (e < n) ? (uniform_w ? w0 : weight_at(wr, i0 + e)) : 0u;
                ka[e] = f2u(a[e]) & 0x7fffffffu;
                kb[e] = hasY ? (f2u(b[e]) & 0x7fffffffu) : 0u;
                hit = hit || ((e < n) && ((ka[e] - lo) < (1u << 20) || (hasY && (kb[e] - lo) < (1u << 20))));
            }
            if constexpr (BLEND) {
#pragma unroll
                for (int e = 0; e < 4; ++e) if (e < n) ex.lds_atomic_add(&lh1[ka[e] >> 20], wv[e]);
            }
            // The bin holds a few per cent of the elements: one test per quad, the staging work behind it
            if (hit && !(SM_DIAG_SEL & 1)) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (e < n) {
                        const uint32_t w = wv[e];
                        if ((ka[e] - lo) < (1u << 20)) {
                            ex.lds_atomic_add(&lh[(ka[e] >> 10) & 1023u], w);
                            const uint32_t pos = ex.lds_atomic_add_ret(&lctl[0], 1u);
                            if (pos < (uint32_t)STAGE_KEYS) lkeys[pos] = ka[e] | ((w - 1u) << 31);
                        }
                        if (hasY && (kb[e] - lo) < (1u << 20)) {
                            ex.lds_atomic_add(&lh[(kb[e] >> 10) & 1023u], w);
                            const uint32_t pos = ex.lds_atomic_add_ret(&lctl[0], 1u);
                            if (pos < (uint32_t)STAGE_KEYS) lkeys[pos] = kb[e] | ((w - 1u) << 31);
                            if (p.fuse_reduce && same_sign(a[e], b[e])) {
                                const uint32_t pp = ex.lds_atomic_add_ret(&lctl[1], 1u);
                                if (pp < (uint32_t)STAGE_PAIRS) { cf4 v = {a[e], b[e], (float)w, 0.f}; lpairs[pp] = v; }
                            }
                        }
                    }
                }
            }
            // the sums over what lies ABOVE the bin (it survives whatever the threshold's low bits): branch-free, a value
            // outside the class enters as an exact zero
            if (p.sumsq) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const bool in = (e < n) && has_hi && ka[e] >= hi;
                    const float av = in ? a[e] : 0.f;
                    q00 += ((float)wv[e] * av) * av;
                }
            }
            if (hasY && p.fuse_reduce && !(SM_DIAG_SEL & 2)) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const bool in = (e < n) && has_hi && kb[e] >= hi && same_sign(a[e], b[e]);   // |r1| >= threshold whatever its low bits
                    const float wf = (float)wv[e];
                    const float av = in ? a[e] : 0.f, bv = in ? b[e] : 0.f;
                    const float wa = wf * av;
                    q00 += wa * av; q01 += wa * bv; q11 += (wf * bv) * bv; qc += in ? wf : 0.f;
                }
            }
            s00 += q00; s01 += q01; s11 += q11; cnt += qc;
        };
        if (p.vec4) {
            // 16-byte loads, U steps in flight together: the address is clamped instead of
            // branched around so that the loads issue back to back
            constexpr int U = SM_SEL_U;
            const cf4* X4 = (const cf4*)p.X;
            const cf4* Y4 = (const cf4*)(BLEND ? p.blendB : p.Y);
            for (int c0 = r0; c0 < r1; c0 += U) {
                cf4 av[U], bv[U];
                size_t qv[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    qv[u] = start + (size_t)(c0 + u) * nt + tid;
                    av[u] = X4[qv[u] < nquad ? qv[u] : nquad - 1];
                }
                if (hasY || BLEND) {
#pragma unroll
                    for (int u = 0; u < U; ++u) bv[u] = Y4[qv[u] < nquad ? qv[u] : nquad - 1];
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (c0 + u < r1 && qv[u] < nquad) {
                        const float a[4] = {av[u].x, av[u].y, av[u].z, av[u].w};
                        const float b[4] = {bv[u].x, bv[u].y, bv[u].z, bv[u].w};
                        quad(4 * qv[u], a, b, 4, !wr.full);
                    }
                }
            }
        } else {
            for (int c = r0; c < r1; ++c) {
                const size_t qi = start + (size_t)c * nt + tid;
                if (qi >= nquad) break;
                float a[4], b[4] = {0.f, 0.f, 0.f, 0.f};
                const int n = load_quad(p.X, 4 * qi, total, 0, a);
                if (hasY) load_quad(p.Y, 4 * qi, total, 0, b);
                if constexpr (BLEND) load_quad(p.blendB, 4 * qi, total, 0, b);
                quad(4 * qi, a, b, n, false);
            }
        }
        s.red[0] += s00; s.red[1] += s01; s.red[2] += s11; s.red[3] += cnt;
    });
    ex.sync();
    // flush when the staging area is more than half full (the counts are the same for every
    // thread after the barrier, so the branch is uniform), and at the end
    const bool last_round = r1 >= p.chunks;
    if (!last_round && !p.flush_always && lctl[0] <= (uint32_t)STAGE_KEYS / 2 && lctl[1] <= (uint32_t)STAGE_PAIRS / 2) continue;
    ex.each(st, [&](int tid, EmptyState&) {
        if (tid == 0) {
            uint32_t nk = lctl[0], np = lctl[1];
            bool over = false;
            if (nk > (uint32_t)STAGE_KEYS) { nk = STAGE_KEYS; over = true; }
            if (np > (uint32_t)STAGE_PAIRS) { np = STAGE_PAIRS; over = true; }
            const uint32_t bk = nk ? ex.global_atomic_add_ret_u32(&p.cand.counters[0], nk) : 0u;
            const uint32_t bp = np ? ex.global_atomic_add_ret_u32(&p.cand.counters[1], np) : 0u;
            if (bk + nk > p.cand.cap_keys || bp + np > p.cand.cap_pairs) over = true;
            // (a speculative pass leaves the sticky word to k_spec_check: an overflow on a wrong guess is void)
            if (over) { ex.global_atomic_or_u32(&p.cand.counters[2], 1u); if (!BLEND) ex.global_atomic_or_u32(&p.cand.counters[3], 1u); }
            lctl[0] = nk; lctl[1] = np; lctl[2] = bk; lctl[3] = bp;
        }
    });
    ex.sync();
    ex.each(st, [&](int tid, EmptyState&) {
        const uint32_t nk = lctl[0], np = lctl[1], bk = lctl[2], bp = lctl[3];
        for (uint32_t q = tid; q < nk; q += nt) if (bk + q < p.cand.cap_keys) p.cand.keys[bk + q] = lkeys[q];
        for (uint32_t q = tid; q < np; q += nt) if (bp + q < p.cand.cap_pairs) p.cand.pairs[bp + q] = lpairs[q];
    });
    ex.sync();
    ex.each(st, [&](int tid, EmptyState&) { if (tid < 4) lctl[tid] = 0; });
    ex.sync();
    }   // rounds
    ex.each(st, [&](int tid, EmptyState&) {
        for (int b = tid; b < HIST_LO_BINS; b += nt) {
            const uint32_t v = lh[b];
            if (v) ex.global_atomic_add(&p.hist[b], (unsigned long long)v);
        }
        if constexpr (BLEND) {
            for (int b = tid; b < HIST1_BINS; b += nt) {
                const uint32_t v = lh1[b];
                if (v) ex.global_atomic_add(&p.hist1_out[b], (unsigned long long)v);
            }
        }
    });
    if (p.fuse_reduce || p.sumsq) {
        ex.sync();
        ex.template block_sum<4>(st, [&](const double* tot) {
            for (int q = 0; q < 4; ++q) p.partials[4 * (size_t)ex.bid() + q] = tot[q];
        });
    }
}

// Single work-group: was the speculated level-1 bin of k_select2<true> the right one?  Resolves level 1 from
// the complete histogram, remembers it as the next guess and either confirms (writes the selection state
// exactly as the plain pass's work-group 0 does, *flag = 1: the plain pass that follows returns at once)
// or voids the speculative output (level-2 histogram and list counters cleared, *flag = 0).
struct SpecCheckParams {
    const unsigned long long* hist1; unsigned long long rank;
    uint32_t* guess; uint32_t* flag;
    SelState* sel;
    unsigned long long* hist2;
    uint32_t* counters;
};
template <class Ex>
SM_HD void k_spec_check(Ex& ex, const SpecCheckParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const int nt = ex.nthreads();
    unsigned long long* scratch = (unsigned long long*)(ex.lds() + LDS_SCRATCH_FLOATS);
    uint32_t* res = (uint32_t*)(scratch + nt + 16);             // behind wg_resolve's partials and group totals
    wg_resolve(ex, st, p.hist1, HIST1_BINS, p.rank, scratch, res);
    ex.each(st, [&](int tid, EmptyState&) {
        if (tid == 0) {
            const uint32_t g = *p.guess;
            const uint32_t hit = (g == res[0] + 1u) ? 1u : 0u;
            res[3] = hit;
            *p.flag = hit;
            p.flag[1] += 1u; p.flag[2] += hit;               // running totals: speculations checked / confirmed
            *p.guess = res[0] + 1u;
            if (hit) {
                p.sel->prefix = res[0]; p.sel->level = 1;
                p.sel->rank = (unsigned long long)res[1] | ((unsigned long long)res[2] << 32);
                if (p.counters[2]) p.counters[3] = 1u;           // the overflow was real
            }
        }
    });
    ex.sync();
    ex.each(st, [&](int tid, EmptyState&) {
        if (res[3]) return;
        for (int b = tid; b < HIST_LO_BINS; b += nt) p.hist2[b] = 0ull;
        if (tid < 3) p.counters[tid] = 0u;
    });
}

// level 3 on the candidate list (or nothing when the list overflowed)
struct Select3Params {
    CandLists cand;
    SelState* sel;                      // in: level-1 prefix/rank; work-group 0 writes the level-2 ones
    const unsigned long long* hist2;    // level-2 histogram, complete
    unsigned long long* hist;           // level-3 histogram, accumulated here
};
template <class Ex>
SM_HD void k_select3(Ex& ex, const Select3Params& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    uint32_t* lh = (uint32_t*)(ex.lds() + LDS_SCRATCH_FLOATS);
    uint32_t* lres = lh + HIST_LO_BINS;
    unsigned long long* part = (unsigned long long*)(lres + 8);
    const int nt = ex.nthreads();
    const uint32_t n = p.cand.counters[2] ? 0u : p.cand.counters[0];     // overflow: the caller redoes the layer
    const uint32_t prefix1 = p.sel->prefix;
    const unsigned long long rank1 = p.sel->rank;
    wg_resolve(ex, st, p.hist2, HIST_LO_BINS, rank1, part, lres);
    const uint32_t prefix = (prefix1 << 10) | lres[0];
    const unsigned long long rank2 = (unsigned long long)lres[1] | ((unsigned long long)lres[2] << 32);
    ex.each(st, [&](int tid, EmptyState&) { for (int b = tid; b < HIST_LO_BINS; b += nt) lh[b] = 0; });
    ex.sync();
    ex.each(st, [&](int tid, EmptyState&) {
        for (size_t q = (size_t)ex.bid() * nt + tid; q < n; q += (size_t)ex.nblocks() * nt) {
            const uint32_t v = p.cand.keys[q];
            const uint32_t key = v & 0x7fffffffu;
            if ((key >> 10) == prefix) ex.lds_atomic_add(&lh[key & 1023u], 1u + (v >> 31));
        }
    });
    ex.sync();
    ex.each(st, [&](int tid, EmptyState&) {
        for (int b = tid; b < HIST_LO_BINS; b += nt) {
            const uint32_t v = lh[b];
            if (v) ex.global_atomic_add(&p.hist[b], (unsigned long long)v);
        }
    });
    // every work-group has read the level-1 state before any can get here? No: work-group 0
    // may run ahead, so the level-2 state goes to the SECOND slot (sel + 1)
    if (ex.bid() == 0) {
        ex.each(st, [&](int tid, EmptyState&) {
            if (tid == 0) { p.sel[1].prefix = prefix; p.sel[1].rank = rank2; p.sel[1].level = 2; }
        });
    }
}

// settle the undecided pairs once the cutoff threshold is known
struct ReduceCandParams {
    CandLists cand;
    const float* thr;
    double* partials;          // [nblocks][4], appended after the fused pass's partials
};
template <class Ex>
SM_HD void k_reduce_cand(Ex& ex, const ReduceCandParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const int nt = ex.nthreads();
    const bool over = p.cand.counters[2] != 0;
    const uint32_t n = over ? 0u : p.cand.counters[1];
    const float thr = *p.thr;
    ex.each(st, [&](int tid, EmptyState& s) {
        double s00 = 0, s01 = 0, s11 = 0, cnt = 0;
        for (size_t q = (size_t)ex.bid() * nt + tid; q < n; q += (size_t)ex.nblocks() * nt) {
            const cf4 v = p.cand.pairs[q];
            if (!(fabsf(v.y) < thr)) {
                s00 += (double)v.z * v.x * v.x; s01 += (double)v.z * v.x * v.y; s11 += (double)v.z * v.y * v.y; cnt += v.z;
            }
        }
        s.red[0] = s00; s.red[1] = s01; s.red[2] = s11; s.red[3] = cnt;
    });
    ex.template block_sum<4>(st, [&](const double* tot) {
        for (int q = 0; q < 4; ++q) p.partials[4 * (size_t)ex.bid() + q] = tot[q];
    });
}

// Work-group-wide resolution of one radix-select level: which bin of `hist` holds the
// element of 0-based rank `rank`, and its rank inside that bin.  Every thread of a
// 256-thread work-group takes part; the result lands in res[0] (bin), res[1..2] (new
// rank, lo/hi).  Consumer kernels run this on the previous level's histogram instead of
// waiting for a separate single-work-group scan launch.
template <class Ex, class StT>
SM_HD void wg_resolve(Ex& ex, StT& st, const unsigned long long* hist, int nbins, unsigned long long rank,
                      unsigned long long* part, uint32_t* res) {
    using S = typename StT::value_type;
    const int nt = ex.nthreads();                       // 256
    const int per = (nbins + nt - 1) / nt;              // <= 8: the thread's bins stay in its state
    unsigned long long* grp = part + nt;                // 16 group totals (the scratch holds 2 * nt words)
    ex.each(st, [&](int tid, S& s) {
        unsigned long long sum = 0;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int b = tid * per + q;
            const unsigned long long h = (q < per && b < nbins) ? hist[b] : 0ull;
            s.keep[q] = h;
            sum += h;
        }
        part[tid] = sum;
        if (tid == 0) { res[0] = 0; res[1] = 0; res[2] = 0; }
    });
    ex.sync();
    ex.each(st, [&](int tid, S&) {                      // 16 threads total 16 partials each
        if (tid < 16) {
            unsigned long long g = 0;
            for (int q = 0; q < 16; ++q) { const int i = tid * 16 + q; if (i < nt) g += part[i]; }
            grp[tid] = g;
        }
    });
    ex.sync();
    ex.each(st, [&](int tid, S& s) {
        unsigned long long excl = 0, total = 0;
        const int g0 = tid / 16;
        for (int g = 0; g < 16; ++g) { const unsigned long long v = grp[g]; total += v; if (g < g0) excl += v; }
        for (int q = g0 * 16; q < tid; ++q) excl += part[q];
        if (total == 0) return;
        unsigned long long r = rank >= total ? total - 1 : rank;
        if (r >= excl && r < excl + part[tid]) {
            unsigned long long cum = excl;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const unsigned long long h = s.keep[q];
                if (q < per && r >= cum && r < cum + h) {
                    res[0] = (uint32_t)(tid * per + q);
                    const unsigned long long nr = r - cum;
                    res[1] = (uint32_t)(nr & 0xffffffffull); res[2] = (uint32_t)(nr >> 32);
                }
                cum += h;
            }
        }
    });
    ex.sync();
}

struct ScanParams {
    unsigned long long* hist;   // consumed and zeroed
    SelState* sel;
    int nbins;                  // HIST1_BINS or HIST_LO_BINS
    int shift;                  // bits this level contributes (11 or 10)
    int final_level;            // 1: write sel->value
    float* value_out;           // optional extra copy of the value
    int init;                   // 1: first level, start from rank_init / empty prefix
    unsigned long long rank_init;
    unsigned long long* zero_also; int zero_count;   // further histogram words to clear (fast path: all levels)
    uint32_t* zero_u32; int zero_u32_count;          // and 32-bit words (the candidate-list counters)
};

// single work-group of 256 threads
template <class Ex>
SM_HD void k_scan(Ex& ex, const ScanParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    unsigned long long* part = (unsigned long long*)(ex.lds() + LDS_SCRATCH_FLOATS);
    const int nt = ex.nthreads();                       // 256
    const int per = (p.nbins + nt - 1) / nt;            // <= 8
    unsigned long long* grp = part + nt;                // 16 group totals
    ex.each(st, [&](int tid, EmptyState& s) {
        unsigned long long sum = 0;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int b = tid * per + q;
            const unsigned long long h = (q < per && b < p.nbins) ? p.hist[b] : 0ull;
            s.keep[q] = h;
            sum += h;
        }
        part[tid] = sum;
    });
    ex.sync();
    ex.each(st, [&](int tid, EmptyState&) {
        if (tid < 16) {
            unsigned long long g = 0;
            for (int q = 0; q < 16; ++q) { const int i = tid * 16 + q; if (i < nt) g += part[i]; }
            grp[tid] = g;
        }
    });
    ex.sync();
    ex.each(st, [&](int tid, EmptyState& s) {
        unsigned long long excl = 0, total = 0;
        const int g0 = tid / 16;
        for (int g = 0; g < 16; ++g) { const unsigned long long v = grp[g]; total += v; if (g < g0) excl += v; }
        for (int q = g0 * 16; q < tid; ++q) excl += part[q];
        unsigned long long rank = p.init ? p.rank_init : p.sel->rank;
        const uint32_t prefix0 = p.init ? 0u : p.sel->prefix;
        const uint32_t level0 = p.init ? 0u : p.sel->level;
        if (total == 0) { if (tid == 0) { p.sel->value = 0.f; if (p.value_out) *p.value_out = 0.f; } return; }
        if (rank >= total) rank = total - 1;
        if (rank >= excl && rank < excl + part[tid]) {
            unsigned long long cum = excl;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const unsigned long long h = s.keep[q];
                if (q < per && rank >= cum && rank < cum + h) {
                    const uint32_t np = (prefix0 << p.shift) | (uint32_t)(tid * per + q);
                    p.sel->prefix = np;
                    p.sel->rank = rank - cum;
                    p.sel->level = level0 + 1;
                    if (p.final_level) {
                        p.sel->value = u2f(np);
                        if (p.value_out) *p.value_out = u2f(np);
                    }
                }
                cum += h;
            }
        }
    });
    ex.sync();
    ex.each(st, [&](int tid, EmptyState&) {
        for (int b = tid * per; b < (tid + 1) * per && b < p.nbins; ++b) p.hist[b] = 0;
        if (p.zero_also) for (int b = tid; b < p.zero_count; b += nt) p.zero_also[b] = 0;
        if (p.zero_u32) for (int b = tid; b < p.zero_u32_count; b += nt) p.zero_u32[b] = 0u;
    });
}


struct ReduceParams {
    const float* reA; const float* reB;
    int R, C, Cb;
    int vec4;
    const float* thr;           // device scalar (cutoff threshold) or null (-> 0)
    double* partials;           // [grid][4]: s00, s01, s11, count
    int chunks;
    const uint32_t* only_if;    // when set: if *only_if == 0 write zero partials and leave
};


template <class Ex>
SM_HD void k_reduce(Ex& ex, const ReduceParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const int nt = ex.nthreads();
    const size_t total = (size_t)p.Cb * p.R;
    const size_t nquad = (total + 3) / 4;
    const float thr = p.thr ? *p.thr : 0.f;
    const WeightRanges wr = weight_ranges(p.R, p.C, p.Cb);
    const bool skip = p.only_if && !*p.only_if;
    ex.each(st, [&](int tid, EmptyState& s) {
        double s00 = 0, s01 = 0, s11 = 0, cnt = 0;
        const size_t start = (size_t)ex.bid() * p.chunks * nt;
        for (int c = 0; c < p.chunks && !skip; ++c) {
            const size_t qi = start + (size_t)c * nt + tid;
            if (qi >= nquad) break;
            const size_t i0 = 4 * qi;
            float a[4], b[4];
            const int n = load_quad(p.reA, i0, total, p.vec4, a);
            load_quad(p.reB, i0, total, p.vec4, b);
            float q00 = 0.f, q01 = 0.f, q11 = 0.f, qc = 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (e < n && same_sign(a[e], b[e]) && !(fabsf(b[e]) < thr)) {
                    const float w = (float)weight_at(wr, i0 + e);
                    q00 += w * a[e] * a[e]; q01 += w * a[e] * b[e]; q11 += w * b[e] * b[e]; qc += w;
                }
            }
            s00 += q00; s01 += q01; s11 += q11; cnt += qc;
        }
        s.red[0] = s00; s.red[1] = s01; s.red[2] = s11; s.red[3] = cnt;
    });
    ex.template block_sum<4>(st, [&](const double* tot) {
        for (int q = 0; q < 4; ++q) p.partials[4 * (size_t)ex.bid() + q] = tot[q];
    });
}

struct SlerpConstParams {
    const double* partials; int nparts;      // fused/definite part + candidate part (contiguous)
    const double* fallback; int nfallback;   // full-pass partials, used instead when *overflow != 0
    const uint32_t* overflow;
    const float* thr;           // device scalar or null (-> 0)
    float t;
    BlendConsts* out;
    uint32_t* zero_u32; int zero_u32_count;  // candidate-list counters to clear for the next selection (or null)
    const float* ref_norms;     // norm_mode = reference_cpu, ordered emulation (test hook): ||v0||, ||v1|| of the gathered
                                // class as torch.norm returns them on CPU (sm_aten_norm.hpp), or null
    const double* emf_part;     // norm_mode = reference_cpu: k_class_emf's partials [emf_nparts][2 * EMF_VALS] (or null)
    int emf_nparts;
    int emf_elo;                // binade of its first rounding level
};

// ---- norm_mode = reference_cpu: what torch.norm makes of the gathered slerp-class vectors -----------------------
// (reference functions.py:36,40: v0.norm(), v1.norm() on fp32 CPU tensors of ~0.4 n elements.)  ATen's kernel
// accumulates fma(x, x, acc) serially in 8 fp32 lanes (sm_aten_norm.hpp), which loses low bits once a lane's sum is
// large: -2e-4 at 16 M elements, -1.5e-3 at 67 M.  The reference's cosine is taken with THOSE norms.  Bit-identity
// is not on offer here (the reference gathers its own spectrum's values in its own order), but the bias is a
// statistical property of the values: while a lane's sum S sits in the binade with ulp u, an element moves it by
// rne(x^2 / u) u, so with g(u) = the class mean of that quantity the sum follows dS/di = g(ulp(S)) binade by binade.
// k_class_emf takes g for EMF_LEVELS consecutive binades (and the exact mean) from a sample of the planes (all of
// them below 4 M elements, 1 piece in 16 from 64 M on); k_slerp_consts integrates the trajectory for cnt / 8 elements per lane and scales the exact norm by the
// ratio.  Against torch.norm on the reference's own gathered vectors: 1e-6 ... 4e-6 where the exact norm is off by
// 2e-4 (4096^2; oracle/aten_norm_model_probe.py); the ordered emulation of sm_aten_norm.hpp (test hook
// "class_norms" = 2) gives the same to 2e-6.
constexpr int EMF_LEVELS = 16;
constexpr int EMF_VALS = EMF_LEVELS + 2;        // weighted count, sum of squares, EMF_LEVELS sums of rounded squares
#ifndef SM_EMF_MAX_SAMPLE
#define SM_EMF_MAX_SAMPLE 16
#endif
constexpr int EMF_MAX_SAMPLE = SM_EMF_MAX_SAMPLE;   // at most one piece of 8 rows (64 plane elements) in every 16 is read ...
constexpr size_t EMF_MIN_SAMPLED = (size_t)2 << 20;   // ... as long as this many elements are
struct ClassEmfParams {
    const float* reA; const float* reB;         // planes [Cb][R]
    const float* thr;                           // device scalar (cutoff threshold) or null (-> 0)
    int R, C, Cb;
    size_t n;                                   // plane elements
    int elo;                                    // level k rounds to multiples of 2^(elo + k - 23)
    int sample;                                 // one piece of 8 rows in every `sample`
    int iters;                                  // pieces per 8 threads
    double* partials;                           // [grid][2 * EMF_VALS]
};
struct EmfState { double red[2 * EMF_VALS]; };
SM_HD double emf_pow2(int e) {
    if (e < -1000) e = -1000;
    if (e > 1000) e = 1000;
    const unsigned long long b = (unsigned long long)(1023 + e) << 52;
    double d; memcpy(&d, &b, 8); return d;
}
template <class Ex>
SM_HD void k_class_emf(Ex& ex, const ClassEmfParams& p) {
    typename Ex::template State<EmfState> st;
    ex.init(st);
    const int nt = ex.nthreads();                       // 256: 32 pieces of 8 rows per sweep
    const size_t rows = (p.n + 7) / 8;
    const size_t npieces = (rows + 8 * (size_t)p.sample - 1) / (8 * (size_t)p.sample);
    const float thr = p.thr ? *p.thr : 0.f;
    const WeightRanges wr = weight_ranges(p.R, p.C, p.Cb);
    const double sc0 = emf_pow2(23 - p.elo);
    ex.each(st, [&](int tid, EmfState& q) {
        double acc[2 * EMF_VALS];
#pragma unroll
        for (int i = 0; i < 2 * EMF_VALS; ++i) acc[i] = 0.0;
        for (int it = 0; it < p.iters; ++it) {
            const size_t piece = ((size_t)ex.bid() * p.iters + it) * (nt / 8) + (size_t)(tid / 8);
            const size_t r = piece * (8 * (size_t)p.sample) + (size_t)(tid % 8);
            // (the address is clamped instead of branched around: a load behind a branch is waited for on the spot;
            // a ragged last row of fewer than 8 elements is left out of the sample)
            const bool live = piece < npieces && r < rows && r * 8 + 8 <= p.n;
            const size_t i0 = live ? r * 8 : 0;
            const cf4 a0 = ((const cf4*)p.reA)[i0 / 4], a1 = ((const cf4*)p.reA)[i0 / 4 + 1];
            const cf4 b0 = ((const cf4*)p.reB)[i0 / 4], b1 = ((const cf4*)p.reB)[i0 / 4 + 1];
            const float a[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
            const float b[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const bool in = live && same_sign(a[e], b[e]) && !(fabsf(b[e]) < thr);
                if (!in) continue;
                const double w = (double)weight_at(wr, i0 + e);
                const double ya = (double)a[e] * (double)a[e], yb = (double)b[e] * (double)b[e];
                acc[0] += w; acc[1] += w * ya;
                acc[EMF_VALS] += w; acc[EMF_VALS + 1] += w * yb;
                double va = ya * sc0, vb = yb * sc0;
#pragma unroll
                for (int k = 0; k < EMF_LEVELS; ++k) {
                    acc[2 + k] += w * floor(va + 0.5);
                    acc[EMF_VALS + 2 + k] += w * floor(vb + 0.5);
                    va *= 0.5; vb *= 0.5;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 2 * EMF_VALS; ++i) q.red[i] = acc[i];
    });
    ex.template block_sum<2 * EMF_VALS>(st, [&](const double* tot) {
        double* o = p.partials + (size_t)ex.bid() * (2 * EMF_VALS);
        for (int i = 0; i < 2 * EMF_VALS; ++i) o[i] = tot[i];
    });
}
// torch.norm / exact norm of a gathered class vector of `cnt` elements from its sampled statistics v[EMF_VALS]
SM_HD double emf_norm_ratio(const double* v, int elo, double cnt) {
    const double cnt_s = v[0], s_s = v[1];
    const double N = floor(cnt / 8.0);
    if (!(cnt_s > 0) || !(s_s > 0) || !(N >= 1)) return 1.0;
    const double mean_y = s_s / cnt_s;
    unsigned long long mb; memcpy(&mb, &mean_y, 8);
    int e = (int)((mb >> 52) & 0x7ffu) - 1023 - 2;
    double S = 0.0, left = N;
    for (int guard = 0; guard < 400 && left > 0; ++guard) {
        const double hi = emf_pow2(e + 1);
        if (S >= hi) { ++e; continue; }
        const int k = e - elo;
        double g = (k >= 0 && k < EMF_LEVELS) ? v[2 + k] * emf_pow2(e - 23) / cnt_s : mean_y;
        if (!(g > 0)) break;                     // every square rounds to nothing: the sum stalls here
        const double need = (hi - S) / g;
        if (need >= left) { S += left * g; left = 0; }
        else { S = hi; left -= need; ++e; }
    }
    const double r = S / (N * mean_y);
    return r > 0 ? sqrt(r) : 1.0;
}

// one work-group: sum the partials (fixed order per thread, then the block
// reduction) and derive the constants (reference functions.py:36-43 on the
// gathered slerp-class vectors)
struct SlerpConstsState { double red[2 * EMF_VALS]; };
template <class Ex>
SM_HD void k_slerp_consts(Ex& ex, const SlerpConstParams& p) {
    typename Ex::template State<SlerpConstsState> st;
    ex.init(st);
    const int nt = ex.nthreads();
    const bool use_fb = p.overflow && *p.overflow;
    const double* src = use_fb ? p.fallback : p.partials;
    const int nsrc = use_fb ? p.nfallback : p.nparts;
    double* emf_tot = (double*)(ex.lds() + 2 * LDS_SCRATCH_FLOATS);       // [2 * EMF_VALS] (the 36-value block sum's scratch
                                                                          // runs past LDS_SCRATCH_FLOATS)
    if (p.emf_part) {
        ex.each(st, [&](int tid, SlerpConstsState& s) {
            double a[2 * EMF_VALS];
#pragma unroll
            for (int q = 0; q < 2 * EMF_VALS; ++q) a[q] = 0.0;
            for (int i = tid; i < p.emf_nparts; i += nt) {
#pragma unroll
                for (int q = 0; q < 2 * EMF_VALS; ++q) a[q] += p.emf_part[(size_t)i * (2 * EMF_VALS) + q];
            }
#pragma unroll
            for (int q = 0; q < 2 * EMF_VALS; ++q) s.red[q] = a[q];
        });
        ex.template block_sum<2 * EMF_VALS>(st, [&](const double* tot) {
            for (int q = 0; q < 2 * EMF_VALS; ++q) emf_tot[q] = tot[q];
        });
    }
    ex.each(st, [&](int tid, SlerpConstsState& s) {
        double a0 = 0, a1 = 0, a2 = 0, a3 = 0;
        for (int i = tid; i < nsrc; i += nt) {
            a0 += src[4 * i]; a1 += src[4 * i + 1];
            a2 += src[4 * i + 2]; a3 += src[4 * i + 3];
        }
        if (p.zero_u32 && tid < p.zero_u32_count) p.zero_u32[tid] = 0u;
        s.red[0] = a0; s.red[1] = a1; s.red[2] = a2; s.red[3] = a3;
    });
    ex.template block_sum<4>(st, [&](const double* tot) {
        const double s00 = tot[0], s01 = tot[1], s11 = tot[2], cnt = tot[3];
        BlendConsts c;
        c.thr = p.thr ? *p.thr : 0.f;
        c.s00 = s00; c.s01 = s01; c.s11 = s11; c.n_slerp = (unsigned long long)cnt;
        double n0 = sqrt(s00), n1 = sqrt(s11), rel_bias = 1.0;
        if (s00 > 0 && s11 > 0) {
            // the reference's cosine divides by ITS norms; F.normalize's norm of (v1 - dot v0) carries about v1's bias
            if (p.ref_norms) {
                rel_bias = (double)p.ref_norms[1] / n1;
                n0 = (double)p.ref_norms[0]; n1 = (double)p.ref_norms[1];
            } else if (p.emf_part) {
                rel_bias = emf_norm_ratio(emf_tot + EMF_VALS, p.emf_elo, cnt);
                n0 *= emf_norm_ratio(emf_tot, p.emf_elo, cnt);
                n1 *= rel_bias;
            }
        }
        double dot = s01 / (n0 * n1);
        if (dot > 1.0) dot = 1.0;
        if (dot < -1.0) dot = -1.0;
        const float dotf = (float)dot;
        const float theta = acosf(dotf) * p.t;
        double rel2 = s11 - 2.0 * (double)dotf * s01 + (double)dotf * (double)dotf * s00;
        if (rel2 < 0) rel2 = 0;
        double reln = sqrt(rel2) * rel_bias;
        if (reln < 1e-12) reln = 1e-12;
        c.dot = dotf; c.cos_t = cosf(theta); c.sin_t = sinf(theta); c.inv_rel = (float)(1.0 / reln);
        c.pad[0] = c.pad[1] = c.pad[2] = 0.f;
        *p.out = c;
    });
}

// sum [n][2] double partials into out[2] (norm^2 of the two signals of F1 / combine)
// Results the host waits for are written by the last small kernel straight into a host-mapped
// "mailbox" (pinned, device-visible): a stream synchronisation replaces the copy kernels and
// staging of hipMemcpyAsync into pageable memory.
struct Mailbox {
    double norm2[16];           // k_sum_partials (2) / k_delta_norms' reduction (up to 16 models)
    uint32_t flags[12];         // NaN/Inf flags [0..7] + candidate counters [8..11] (k_publish)
    float thr[4];               // d_thr(0..3)
    BlendConsts consts;
    float snorm[16];            // k_serial_norm results (norm_mode = reference_cpu)
    float corr[64];             // k_corr_finish: the K x K matrix of correlate_pairs
};
struct PublishParams {
    const uint32_t* flags;      // device flags + counters (12 words)
    const float* thr;
    const BlendConsts* consts;
    Mailbox* mail;
    uint32_t* zero_flags;       // when set: the 12 flag words are cleared after the copy
};
template <class Ex>
SM_HD void k_publish(Ex& ex, const PublishParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    ex.each(st, [&](int tid, EmptyState&) {
        if (tid < 12) {
            p.mail->flags[tid] = p.flags[tid];
            if (p.zero_flags) p.zero_flags[tid] = 0u;
        }
        if (tid < 4) p.mail->thr[tid] = p.thr[tid];
        if (tid == 0) p.mail->consts = *p.consts;
    });
}

struct SumPartialsParams { const double* partials; int nparts; double* out; };
template <class Ex>
SM_HD void k_sum_partials(Ex& ex, const SumPartialsParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const int nt = ex.nthreads();
    ex.each(st, [&](int tid, EmptyState& s) {
        double a0 = 0, a1 = 0;
        for (int i = tid; i < p.nparts; i += nt) { a0 += p.partials[2 * i]; a1 += p.partials[2 * i + 1]; }
        s.red[0] = a0; s.red[1] = a1;
    });
    ex.template block_sum<2>(st, [&](const double* tot) { p.out[0] = tot[0]; p.out[1] = tot[1]; });
}

// ---- kernel tags (sm_tag.hpp) ----
SM_KERNEL_TAG(KPublish, PublishParams, "publish", k_publish(ex, p))
SM_KERNEL_TAG(KHist, HistParams, "select_hist", k_hist(ex, p))
SM_KERNEL_TAG(KScan, ScanParams, "select_scan", k_scan(ex, p))
SM_KERNEL_TAG(KSelect2, Select2Params, "select_lvl2", k_select2<false>(ex, p))
SM_KERNEL_TAG(KSelect2Cull, Select2Params, "select_lvl2_cull", k_select2<false>(ex, p))     // the cull's pass: returns at once after a confirmed speculation
SM_KERNEL_TAG(KBlendSel, Select2Params, "blend", k_select2<true>(ex, p))
SM_KERNEL_TAG(KSpecCheck, SpecCheckParams, "select_spec_check", k_spec_check(ex, p))
SM_KERNEL_TAG(KSelect3, Select3Params, "select_lvl3_cand", k_select3(ex, p))
SM_KERNEL_TAG(KReduceCand, ReduceCandParams, "slerp_reduce_cand", k_reduce_cand(ex, p))
SM_KERNEL_TAG(KReduce, ReduceParams, "slerp_reduce", k_reduce(ex, p))
SM_KERNEL_TAG(KSlerpConsts, SlerpConstParams, "slerp_consts", k_slerp_consts(ex, p))
SM_KERNEL_TAG_LB(KClassEmf, ClassEmfParams, "class_norm_stats", k_class_emf(ex, p), 256, 2)
SM_KERNEL_TAG(KSumPartials, SumPartialsParams, "sum_partials", k_sum_partials(ex, p))
// this header's share of group 1 of smhip_side.hip (smhip_device.hpp; the group itself: sm_side_1.hpp)
#define SM_KERNELS_SELECT(X) X(KPublish) X(KHist) X(KScan) X(KSelect2) X(KSelect2Cull) X(KBlendSel) \
    X(KSpecCheck) X(KSelect3) X(KReduceCand) X(KReduce) X(KSlerpConsts) X(KSumPartials) X(KClassEmf)

}  // namespace smhip
