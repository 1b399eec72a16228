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
#pragma once
#include "sm_kernels.hpp"

namespace smhip {

constexpr int TIES_MAX_MODELS = 16;
constexpr int TIES_GROUP = 4;                 // finetunes per ties_hist launch (an LDS histogram each)
constexpr uint32_t TIES_KEY_INF = 0x7f800000u;

// selection state of one finetune (device memory)
struct TiesState {
    unsigned long long rank;    // 1-based rank (from the largest) wanted among the keys that share `prefix`
    unsigned long long above;   // keys known to be larger than every key with this prefix
    uint32_t prefix;            // key bits decided so far (11, 21, then all 31: the threshold)
    uint32_t pad;
};

struct TiesInputs {
    int k;
    const void* ft[TIES_MAX_MODELS];
    const void* base[TIES_MAX_MODELS];
    int dtype;                  // finetunes and their bases
    size_t n;
    int aligned;                // every pointer (out included) is 16-byte aligned: full octets use 16-byte accesses
    int shared_base;            // every base[i] is base[0]
};

// 8 elements from i0 on (cnt of them exist)
SM_HD void ties_load8(const void* src, int dtype, size_t i0, int cnt, bool vec, float* dst) {
    if (vec) { load_elem8(src, dtype, i0, dst); return; }
    for (int e = 0; e < 8; ++e) dst[e] = e < cnt ? load_elem(src, dtype, i0 + e) : 0.f;
}

struct TiesHistParams {
    TiesInputs in;
    int first, count;           // the finetunes of this launch: first .. first + count - 1, count <= TIES_GROUP
    int level;                  // 1, 2 or 3
    const TiesState* state;     // [k]
    unsigned long long* hist;   // [k][HIST1_BINS] of this level
    uint32_t* flags;            // [0]: bit i = finetune i has a non-finite delta
    int chunks;                 // octets per thread
};
template <class Ex>
SM_HD void k_ties_hist(Ex& ex, const TiesHistParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    uint32_t* lh = (uint32_t*)(ex.lds() + LDS_SCRATCH_FLOATS);
    const int nt = ex.nthreads();
    const int nbins = p.level == 1 ? HIST1_BINS : HIST_LO_BINS;
    const size_t noct = (p.in.n + 7) / 8;
    ex.each(st, [&](int tid, EmptyState&) { for (int b = tid; b < nbins * p.count; b += nt) lh[b] = 0; });
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
                const uint32_t prefix = p.level == 1 ? 0u : p.state[i].prefix;
                uint32_t* h = lh + j * nbins;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    if (e < cnt) {
                        const uint32_t key = f2u(f[e] - b[e]) & 0x7fffffffu;
                        if (p.level == 1) {
                            if (key >= TIES_KEY_INF) bad |= 1u << i;
                            ex.lds_atomic_add(&h[key >> 20], 1u);
                        } else if (p.level == 2) {
                            if ((key >> 20) == prefix) ex.lds_atomic_add(&h[(key >> 10) & 1023u], 1u);
                        } else {
                            if ((key >> 10) == prefix) ex.lds_atomic_add(&h[key & 1023u], 1u);
                        }
                    }
                }
            }
        }
        if (bad) ex.global_atomic_or_u32(p.flags, bad);
    });
    ex.sync();
    ex.each(st, [&](int tid, EmptyState&) {
        for (int b = tid; b < nbins * p.count; b += nt) {
            const uint32_t v = lh[b];
            if (v) ex.global_atomic_add(&p.hist[(size_t)(p.first + b / nbins) * HIST1_BINS + (b % nbins)], (unsigned long long)v);
        }
    });
}

// one work-group of TIES_SELECT_THREADS per finetune; thread t owns TIES_SELECT_PER consecutive bins
constexpr int TIES_SELECT_THREADS = 256;
constexpr int TIES_SELECT_PER = HIST1_BINS / TIES_SELECT_THREADS;
struct TiesSelectParams {
    int level;                       // 1, 2 or 3
    unsigned long long k_keep;       // elements to keep per finetune (0: the threshold is +inf)
    const unsigned long long* hist;  // [k][HIST1_BINS] of this level
    TiesState* state;                // [k]
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
    const int nbins = p.level == 1 ? HIST1_BINS : HIST_LO_BINS;
    const unsigned long long* h = p.hist + (size_t)m * HIST1_BINS;
    TiesState* s = p.state + m;
    const unsigned long long rank = p.level == 1 ? p.k_keep : s->rank;
    const unsigned long long above0 = p.level == 1 ? 0ull : s->above;
    const uint32_t prefix0 = p.level == 1 ? 0u : s->prefix;
    ex.each(st, [&](int tid, TiesSelectState& t) {
        unsigned long long a = 0;
        for (int q = 0; q < TIES_SELECT_PER; ++q) {
            const int b = tid * TIES_SELECT_PER + q;
            if (b < nbins) a += h[b];
        }
        t.own = a;
        part[tid] = a;
    });
    ex.sync();
    ex.each(st, [&](int tid, TiesSelectState& t) {
        if (p.k_keep == 0) {          // nothing is kept: no finite magnitude reaches +inf
            if (tid == 0 && p.level == 3) { p.threshold[m] = u2f(TIES_KEY_INF); p.kept[m] = 0; }
            return;
        }
        unsigned long long higher = 0;                       // keys in the bins of the threads after this one
        for (int q = tid + 1; q < TIES_SELECT_THREADS; ++q) higher += part[q];
        if (!(higher < rank && rank <= higher + t.own)) return;
        // the bin that holds the rank-th largest key is one of this thread's
        for (int q = TIES_SELECT_PER - 1; q >= 0; --q) {
            const int b = tid * TIES_SELECT_PER + q;
            const unsigned long long c = b < nbins ? h[b] : 0ull;
            if (rank <= higher + c) {
                const uint32_t prefix = (prefix0 << (p.level == 1 ? 0 : 10)) | (uint32_t)b;
                s->prefix = prefix;
                s->rank = rank - higher;
                s->above = above0 + higher;
                if (p.level == 3) {                          // the bin is one key: the threshold; ties at it are all kept
                    p.threshold[m] = u2f(prefix);
                    p.kept[m] = above0 + higher + (prefix != 0u ? c : 0ull);     // a zero delta is never kept
                }
                return;
            }
            higher += c;
        }
    });
}

// the store tail of a fused merge pass (ties_merge, dare_merge): octet oi of out (r, rounded once to out_dtype) and of the
// optional fp32 delta_out (dl); cnt of the 8 elements exist, vec: one 16-byte store per 8 x 16 bit / two per 8 x fp32
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
    const int nt = ex.nthreads();
    const size_t noct = (p.in.n + 7) / 8;
    const float eps = 1e-8f;
    ex.each(st, [&](int tid, EmptyState&) {
        const size_t start = (size_t)ex.bid() * p.chunks * nt;
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
            // The sum over the agreeing entries equals the running sum of the positive (elected +1) or of the negative
            // (elected -1) weighted deltas: the skipped terms are +0 and x + 0 = x.  Both are kept, the election picks.
            for (int i = 0; i < p.in.k; ++i) {
                float f[8];
                ties_load8(p.in.ft[i], p.in.dtype, i0, cnt, vec, f);
                if (!p.in.shared_base) ties_load8(p.in.base[i], p.in.dtype, i0, cnt, vec, b);
                const uint32_t tau = f2u(p.threshold[i]);
                const float al = p.alpha[i];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float d = f[e] - b[e];
                    const uint32_t key = f2u(d) & 0x7fffffffu;
                    const bool kept = key >= tau && key != 0u;
                    const float tv = kept ? aten_fmul_(d, al) : 0.f;
                    S[e] = aten_fadd_(S[e], tv);
                    if (tv > 0.f) { P[e] = aten_fadd_(P[e], tv); DP[e] = aten_fadd_(DP[e], al); }
                    if (tv < 0.f) { N[e] = aten_fadd_(N[e], tv); DN[e] = aten_fadd_(DN[e], al); }
                }
            }
            float r[8], dl[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const bool pos = S[e] >= 0.f;
                float M = pos ? P[e] : N[e];
                if (p.normalize) {
                    float D = pos ? DP[e] : DN[e];
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
