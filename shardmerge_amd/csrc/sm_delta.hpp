// sm_delta.hpp - what the delta-merge operators (sm_ties.hpp, sm_dare.hpp, sm_breadcrumbs.hpp, sm_geo.hpp, sm_sce.hpp,
// sm_della.hpp, sm_consensus.hpp) share on the device, written once:
//
//   Octet, octet_at, segment_octet    block / chunk / thread -> the 8 elements a thread works on
//   ties_load8, delta_base8, delta_load8, delta_base_out8, delta_store8
//                                     the operands of an octet's deltas (the base once when shared), base_out, the store
//   Election                          S / P / N / DP / DN of the TIES sign election: clear, add, merged, finish
//   kept_zero, kept_fold              the kept counters of a drop mask: [k][nt] in LDS -> one global atomic per finetune
//   RadixState, radix_start, radix_own_sum, radix_select_step, radix_advance
//                                     one level of the exact select of the rank-th largest 31-bit key
//   radix_bin, hist_zero, hist_flush  one level of its histograms in LDS
// A kernel of an operator is these plus the lines that ARE the operator: its keep test, its scale, its extra loads.
#pragma once
#include "sm_common.hpp"
#include "sm_tag.hpp"

namespace smhip {

constexpr int TIES_MAX_MODELS = 16;
constexpr int TIES_GROUP = 4;                 // finetunes per *_hist launch (an LDS histogram each)
constexpr uint32_t TIES_KEY_INF = 0x7f800000u;

struct TiesInputs {
    int k;
    const void* ft[TIES_MAX_MODELS];
    const void* base[TIES_MAX_MODELS];
    int dtype;                  // finetunes and their bases
    size_t n;
    int aligned;                // every pointer (out included) is 16-byte aligned: full octets use 16-byte accesses
    int shared_base;            // every base[i] is base[0]
};

// the magnitude of a delta as a key: a finite fp32 value orders like its low 31 bits; >= TIES_KEY_INF: NaN or Inf
SM_HD uint32_t delta_key(float d) { return f2u(d) & 0x7fffffffu; }

// ---- the octet walk ----
// elements i0 .. i0 + 7 of the flat index (i0 = 8 * oi); lo <= e < cnt are the thread's, the others load as they come
// (e < lo) or as +0 (e >= cnt) and are never stored.  vec: all 8 and every pointer aligned, 16-byte accesses
struct Octet { size_t oi, i0; int lo, cnt; bool vec; };

// octet q of thread tid of work-group bid over the elements [lo, hi): `chunks` per thread, a work-group apart; false: past the end
SM_HD bool octet_at(size_t lo, size_t hi, int aligned, int bid, int nt, int chunks, int tid, int q, Octet& o) {
    const size_t oct0 = lo >> 3, noct = ((hi + 7) >> 3) - oct0;
    const size_t oq = ((size_t)bid * chunks + q) * nt + tid;
    if (oq >= noct) return false;
    const size_t oi = oct0 + oq, i0 = 8 * oi;
    const int e_lo = i0 < lo ? (int)(lo - i0) : 0, cnt = (int)((hi - i0) < 8 ? (hi - i0) : 8);
    o = Octet{oi, i0, e_lo, cnt, aligned && e_lo == 0 && cnt == 8};
    return true;
}
// ... over the whole tensor
SM_HD bool octet_at(const TiesInputs& in, int bid, int nt, int chunks, int tid, int q, Octet& o) {
    return octet_at(0, in.n, in.aligned, bid, nt, chunks, tid, q, o);
}
// octet q of ONE segment [start, start + len) that a work-group owns, counted from the segment's start; thread tid takes
// q = tid, tid + nt, ... (the order of the fp64 sums of geo_gram and sce_energy)
SM_HD size_t segment_octets(size_t len) { return (len + 7) / 8; }
SM_HD Octet segment_octet(size_t start, size_t len, int seg_vec, size_t q) {
    const int cnt = (int)((len - 8 * q) < 8 ? (len - 8 * q) : 8);
    return Octet{q, start + 8 * q, 0, cnt, seg_vec && cnt == 8};
}

// ---- the loader and the store ----
// 8 elements from i0 on (cnt of them exist)
SM_HD void ties_load8(const void* src, int dtype, size_t i0, int cnt, bool vec, float* dst) {
    if (vec) { load_elem8(src, dtype, i0, dst); return; }
    for (int e = 0; e < 8; ++e) dst[e] = e < cnt ? load_elem(src, dtype, i0 + e) : 0.f;
}
// the base of the octet's deltas when all finetunes share it (else delta_load8 loads each finetune's own into b)
SM_HD void delta_base8(const TiesInputs& in, const Octet& o, float* b) {
    if (in.shared_base) ties_load8(in.base[0], in.dtype, o.i0, o.cnt, o.vec, b);
}
// finetune i into f and, unless shared, its base into b: element e of its delta is f[e] - b[e]
SM_HD void delta_load8(const TiesInputs& in, int i, const Octet& o, float* b, float* f) {
    ties_load8(in.ft[i], in.dtype, o.i0, o.cnt, o.vec, f);
    if (!in.shared_base) ties_load8(in.base[i], in.dtype, o.i0, o.cnt, o.vec, b);
}
// base_out of a *MergeParams; out_is_base0: it is the shared base b, loaded already
template <class MergeParams>
SM_HD void delta_base_out8(const MergeParams& p, const Octet& o, const float* b, float* bo) {
    if (p.out_is_base0) {
#pragma unroll
        for (int e = 0; e < 8; ++e) bo[e] = b[e];
    } else {
        ties_load8(p.base_out, p.base_out_dtype, o.i0, o.cnt, o.vec, bo);
    }
}
// the store tail of a fused merge pass: octet oi of out (r, rounded once to out_dtype) and of the optional fp32 delta_out
// (dl); cnt of the 8 elements exist, vec: one 16-byte store per 8 x 16 bit / two per 8 x fp32
SM_HD void ties_store8(void* out, int out_dtype, float* delta_out, size_t oi, int cnt, bool vec, const float* r, const float* dl) {
    const size_t i0 = 8 * oi;
    if (delta_out) {
        if (vec) {
            cf4 w0 = {dl[0], dl[1], dl[2], dl[3]}, w1 = {dl[4], dl[5], dl[6], dl[7]};
            ((cf4*)delta_out)[i0 / 4] = w0; ((cf4*)delta_out)[i0 / 4 + 1] = w1;
        } else {
            for (int e = 0; e < cnt; ++e) delta_out[i0 + e] = dl[e];
        }
    }
    if (out_dtype == DT_F32) {
        if (vec) {
            cf4 w0 = {r[0], r[1], r[2], r[3]}, w1 = {r[4], r[5], r[6], r[7]};
            ((cf4*)out)[i0 / 4] = w0; ((cf4*)out)[i0 / 4 + 1] = w1;
        } else {
            for (int e = 0; e < cnt; ++e) ((float*)out)[i0 + e] = r[e];
        }
    } else {
        uint16_t h[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) h[e] = out_dtype == DT_BF16 ? f_to_bf16_any(r[e]) : f_to_f16_any(r[e]);
        if (vec) {
            u32x4 w;
            w.x = (uint32_t)h[0] | ((uint32_t)h[1] << 16); w.y = (uint32_t)h[2] | ((uint32_t)h[3] << 16);
            w.z = (uint32_t)h[4] | ((uint32_t)h[5] << 16); w.w = (uint32_t)h[6] | ((uint32_t)h[7] << 16);
            ((u32x4*)out)[oi] = w;
        } else {
            for (int e = 0; e < cnt; ++e) ((uint16_t*)out)[i0 + e] = h[e];
        }
    }
}
// ... of a *MergeParams; an octet whose first elements are another's (o.lo > 0, a slab's edge) goes element by element
template <class MergeParams>
SM_HD void delta_store8(const MergeParams& p, const Octet& o, const float* r, const float* dl) {
    if (o.lo == 0) { ties_store8(p.out, p.base_out_dtype, p.delta_out, o.oi, o.cnt, o.vec, r, dl); return; }
    for (int e = o.lo; e < o.cnt; ++e) {
        if (p.delta_out) p.delta_out[o.i0 + e] = dl[e];
        if (p.base_out_dtype == DT_F32) ((float*)p.out)[o.i0 + e] = r[e];
        else ((uint16_t*)p.out)[o.i0 + e] = p.base_out_dtype == DT_BF16 ? f_to_bf16_any(r[e]) : f_to_f16_any(r[e]);
    }
}

// ---- the sign election ----
// The sum over the agreeing entries equals the running sum of the positive (elected +1) or of the negative (elected -1)
// weighted terms: the skipped terms are +0 and x + 0 = x.  Both are kept, the election picks.  elect == 0 (the linear
// variants): M is the sum of all terms S, its divisor Dall, the sum of ALL weights, kept or not.
SM_HD float delta_weight_sum(const float* alpha, int k) {
    float Dall = 0.f;
    for (int i = 0; i < k; ++i) Dall = aten_fadd_(Dall, alpha[i]);
    return Dall;
}
struct Election {
    float S[8], P[8], N[8], DP[8], DN[8];
    SM_HD void clear() {
#pragma unroll
        for (int e = 0; e < 8; ++e) { S[e] = 0.f; P[e] = 0.f; N[e] = 0.f; DP[e] = 0.f; DN[e] = 0.f; }
    }
    // element e gains the term tv (+0: trimmed or dropped) of a finetune of weight al
    SM_HD void add(int e, float tv, float al, int elect) {
        S[e] = aten_fadd_(S[e], tv);
        if (elect) {
            if (tv > 0.f) { P[e] = aten_fadd_(P[e], tv); DP[e] = aten_fadd_(DP[e], al); }
            if (tv < 0.f) { N[e] = aten_fadd_(N[e], tv); DN[e] = aten_fadd_(DN[e], al); }
        }
    }
    // M of element e: the elected (or the plain) sum, over its divisor when normalize
    SM_HD float merged(int e, int elect, int normalize, float Dall) const {
        const float eps = 1e-8f;
        const bool pos = S[e] >= 0.f;
        float M = elect ? (pos ? P[e] : N[e]) : S[e];
        if (normalize) {
            float D = elect ? (pos ? DP[e] : DN[e]) : Dall;
            if (fabsf(D) < eps) D = 1.f;
            M = M / D;
        }
        return M;
    }
    // dl = lambda * M, r = bo + dl
    SM_HD void finish(int elect, int normalize, float Dall, float lambda, const float* bo, float* r, float* dl) const {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float M = merged(e, elect, normalize, Dall);
            dl[e] = aten_fmul_(lambda, M);
            r[e] = aten_fadd_(bo[e], dl[e]);
        }
    }
};

// ---- the kept counters of dare_merge and della_merge ----
// dynamic LDS beyond the scratch: a kept counter per (finetune, thread) lc[k][nt], then the k work-group totals
SM_HD size_t dare_lds_words(int k, int nthreads) { return (size_t)k * nthreads + TIES_MAX_MODELS; }
template <class Ex, class St>
SM_HD void kept_zero(Ex& ex, St& st, uint32_t* lc, int k) {
    const int nt = ex.nthreads();
    uint32_t* tot = lc + (size_t)k * nt;
    ex.each(st, [&](int tid, auto&) {
        for (int i = 0; i < k; ++i) lc[i * nt + tid] = 0;
        if (tid < TIES_MAX_MODELS) tot[tid] = 0;
    });
    ex.sync();
}
// 16 threads per finetune add up its nt counters, one LDS atomic each; then one global atomic per finetune
template <class Ex, class St>
SM_HD void kept_fold(Ex& ex, St& st, uint32_t* lc, int k, unsigned long long* kept) {
    const int nt = ex.nthreads();
    uint32_t* tot = lc + (size_t)k * nt;
    ex.sync();
    ex.each(st, [&](int tid, auto&) {
        const int groups = nt >= 16 ? nt >> 4 : 1;
        for (int i = tid >> 4; i < k; i += groups) {
            uint32_t s = 0;
            for (int t = tid & 15; t < nt; t += 16) s += lc[i * nt + t];
            if (s) ex.lds_atomic_add(&tot[i], s);
        }
    });
    ex.sync();
    ex.each(st, [&](int tid, auto&) {
        if (tid < k && tot[tid]) ex.global_atomic_add(&kept[tid], (unsigned long long)tot[tid]);
    });
}

// ---- one level of the radix select: keys of 31 bits in levels of 11 + 10 + 10 (HIST1_BINS / HIST_LO_BINS) ----
// selection state of one rank (device memory)
struct RadixState {
    unsigned long long rank;    // 1-based rank (from the largest) wanted among the keys that share `prefix`
    unsigned long long above;   // keys known to be larger than every key with this prefix
    uint32_t prefix;            // key bits decided so far (11, 21, then all 31: the threshold)
    uint32_t pad;
};
SM_HD int radix_bins(int level) { return level == 1 ? HIST1_BINS : HIST_LO_BINS; }
// the bin of a key in the histogram of the keys under `prefix`, -1: the key is not under it
SM_HD int radix_bin(int level, uint32_t key, uint32_t prefix) {
    if (level == 1) return (int)(key >> 20);
    if (level == 2) return (key >> 20) == prefix ? (int)((key >> 10) & 1023u) : -1;
    return (key >> 10) == prefix ? (int)(key & 1023u) : -1;
}
// the LDS histograms of a work-group: zeroed, filled with ex.lds_atomic_add, then the non-zero words added to
// *dst(word) with 64-bit global atomics
template <class Ex, class St>
SM_HD void hist_zero(Ex& ex, St& st, uint32_t* lh, int words) {
    const int nt = ex.nthreads();
    ex.each(st, [&](int tid, auto&) { for (int b = tid; b < words; b += nt) lh[b] = 0; });
    ex.sync();
}
template <class Ex, class St, class Dst>
SM_HD void hist_flush(Ex& ex, St& st, const uint32_t* lh, int words, Dst&& dst) {
    const int nt = ex.nthreads();
    ex.sync();
    ex.each(st, [&](int tid, auto&) {
        for (int b = tid; b < words; b += nt) {
            const uint32_t v = lh[b];
            if (v) ex.global_atomic_add(dst(b), (unsigned long long)v);
        }
    });
}

// one work-group of TIES_SELECT_THREADS per selection; thread t owns TIES_SELECT_PER consecutive bins
constexpr int TIES_SELECT_THREADS = 256;
constexpr int TIES_SELECT_PER = HIST1_BINS / TIES_SELECT_THREADS;
constexpr size_t TIES_SELECT_LDS = LDS_SCRATCH_FLOATS * 4 + TIES_SELECT_THREADS * sizeof(unsigned long long);
// where a level starts: level 1 from the wanted rank, the later ones from what the level before left in s
SM_HD RadixState radix_start(int level, unsigned long long rank1, const RadixState& s) {
    return level == 1 ? RadixState{rank1, 0ull, 0u, 0u} : s;
}
// the keys in this thread's bins of histogram h (to part[tid]; the step below runs after a barrier)
SM_HD unsigned long long radix_own_sum(const unsigned long long* h, int nbins, int tid) {
    unsigned long long a = 0;
    for (int q = 0; q < TIES_SELECT_PER; ++q) {
        const int b = tid * TIES_SELECT_PER + q;
        if (b < nbins) a += h[b];
    }
    return a;
}
// found: the bin that holds the rank-th largest key is this thread's bin `bin` of c keys, `higher` keys lie in the bins above it
struct RadixFound { bool found; int bin; unsigned long long c, higher; };
SM_HD RadixFound radix_select_step(const unsigned long long* h, int nbins, const unsigned long long* part,
                                   unsigned long long own, unsigned long long rank, int tid) {
    unsigned long long higher = 0;                       // keys in the bins of the threads after this one
    for (int q = tid + 1; q < TIES_SELECT_THREADS; ++q) higher += part[q];
    if (!(higher < rank && rank <= higher + own)) return RadixFound{false, 0, 0ull, 0ull};
    for (int q = TIES_SELECT_PER - 1; q >= 0; --q) {
        const int b = tid * TIES_SELECT_PER + q;
        const unsigned long long c = b < nbins ? h[b] : 0ull;
        if (rank <= higher + c) return RadixFound{true, b, c, higher};
        higher += c;
    }
    return RadixFound{false, 0, 0ull, 0ull};
}
// the state after the level that started at s0 found f: the next bits of the prefix, the rank inside the bin, the keys above
SM_HD RadixState radix_advance(int level, const RadixState& s0, const RadixFound& f) {
    return RadixState{s0.rank - f.higher, s0.above + f.higher, (s0.prefix << (level == 1 ? 0 : 10)) | (uint32_t)f.bin, 0u};
}

}  // namespace smhip
