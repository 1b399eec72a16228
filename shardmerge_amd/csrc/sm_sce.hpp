// sm_sce.hpp - SCE merge (Wan et al., FuseChat: select, calculate, erase), an operator the reference does not have.
// The function is stated in include/shardmerge_hip.h (smhip_sce_merge).  It is the first operator that needs both the
// exact radix select of sm_delta.hpp and the ordered fp64 accumulation of sm_geo.hpp in one call; every step of it is
// one correctly rounded operation or an exact order statistic in a stated order, so these kernels equal a plain
// restatement of it bit for bit.
//
//   sce_hist         one radix level of the selection of the k_keep-th largest score q, the sum of squared deviations of
//                    an element's k deltas from their mean.  q is formed on the fly from 16-byte loads of the k finetunes
//                    and their bases; q >= +0 and is not NaN for finite deltas, so it orders like its bits: levels of
//                    11 + 10 + 10 bits as in ties_hist.  ONE selection stream whatever k: one LDS histogram per
//                    work-group.  Level 1 also raises a flag bit per finetune whose delta holds a NaN or an Inf and
//                    counts the elements with q == 0, so that nz is known.
//   sce_select       the radix step of ties_select (sm_delta.hpp) on that stream; level 1 first turns nz into k_keep on the device.  After
//                    level 3 the threshold and the selected count are final and stay on the device.
//   sce_energy       E_i = sum of x_i^2 in fp64 over the selected elements, in the order of geo_gram: a work-group of
//                    256 per 32768-element segment, octet o to lane o % 256, the binary tree through LDS.
//   sce_energy_fold  the segments added in index order, a thread per finetune (k_geo_fold, sm_geo.hpp).
//   sce_merge        the fused streaming pass: the k finetunes, their bases and base_out are loaded once, q and the mask
//                    recomputed, sign election / weighted masked sums / division / add-back in registers; the weights
//                    arrive as kernel arguments.
// The kernels hold the k deltas of an octet in registers, KR of them: KR = 4 serves k <= 4, KR = 16 any k (same source).
#pragma once
#include "sm_geo.hpp"
#include "sm_ties.hpp"        // (TiesSelectState)

namespace smhip {

constexpr int SCE_REG_SMALL = 4;              // k <= 4: the instantiation with four deltas per octet in registers
constexpr uint32_t SCE_KEY_NONE = 0xffffffffu; // a threshold key that no score reaches (k_keep == 0)

// selection state and results (device memory, zeroed before a call)
struct SceState {
    RadixState sel;             // the one selection stream
    unsigned long long zeros;   // elements with q == 0 (level 1)
    unsigned long long k_keep;  // floor(select_topk * nz), from level 1 on
    unsigned long long selected;// elements with q >= tau and q > 0, after level 3
    uint32_t tau_key;           // after level 3: the bits of tau, SCE_KEY_NONE when k_keep == 0
    float threshold;            // after level 3: tau, +inf when k_keep == 0
};

// the deltas of octet o (the elements past its cnt are +0): d[i][e] for i < k <= KR; `bad` gains bit i where d_i holds
// a NaN or an Inf
template <int KR>
SM_HD void sce_delta8(const TiesInputs& in, const Octet& o, float (*d)[8], uint32_t& bad) {
    float b[8];
    delta_base8(in, o, b);
#pragma unroll
    for (int i = 0; i < KR; ++i) {
        if (i < in.k) {
            delta_load8(in, i, o, b, d[i]);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                d[i][e] = d[i][e] - b[e];
                if (delta_key(d[i][e]) >= TIES_KEY_INF) bad |= 1u << i;
            }
        }
    }
}
// step 2 of the definition: the key of q = sum_i fl32((d_i - mean)^2), mean = (sum_i d_i) / fp32(k), every operation one
// rounded fp32 operation.  (The sign bit is masked off: q has none for finite deltas, and a NaN from non-finite ones,
// where the call fails anyway, must still index inside the histogram.)
template <int KR>
SM_HD void sce_key8(int k, const float (*d)[8], uint32_t* key) {
    const float fk = (float)k;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < KR; ++i)
            if (i < k) s = aten_fadd_(s, d[i][e]);
        const float mean = s / fk;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < KR; ++i) {
            if (i < k) {
                const float dev = aten_fadd_(d[i][e], -mean);
                q = aten_fadd_(q, aten_fmul_(dev, dev));
            }
        }
        key[e] = f2u(q) & 0x7fffffffu;
    }
}

struct SceHistParams {
    TiesInputs in;
    int level;                  // 1, 2 or 3
    SceState* state;            // [1]
    unsigned long long* hist;   // [HIST1_BINS] of this level
    uint32_t* flags;            // [0]: bit i = finetune i has a non-finite delta
    int chunks;                 // octets per thread
};
template <int KR, class Ex>
SM_HD void k_sce_hist(Ex& ex, const SceHistParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    uint32_t* lh = (uint32_t*)(ex.lds() + LDS_SCRATCH_FLOATS);     // [nbins] and, level 1, the count of q == 0 after them
    const int nbins = radix_bins(p.level);
    const uint32_t prefix = p.level == 1 ? 0u : p.state->sel.prefix;
    hist_zero(ex, st, lh, nbins + 1);
    ex.each(st, [&](int tid, EmptyState&) {
        uint32_t bad = 0;
        for (int q = 0; q < p.chunks; ++q) {
            Octet o;
            if (!octet_at(p.in, ex.bid(), ex.nthreads(), p.chunks, tid, q, o)) break;
            float d[KR][8];
            uint32_t key[8];
            sce_delta8<KR>(p.in, o, d, bad);
            sce_key8<KR>(p.in.k, d, key);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                if (e < o.cnt) {
                    const int bin = radix_bin(p.level, key[e], prefix);
                    if (bin >= 0) ex.lds_atomic_add(&lh[bin], 1u);
                    if (p.level == 1 && key[e] == 0u) ex.lds_atomic_add(&lh[nbins], 1u);
                }
            }
        }
        if (bad && p.level == 1) ex.global_atomic_or_u32(p.flags, bad);
    });
    hist_flush(ex, st, lh, nbins, [&](int b) { return &p.hist[b]; });
    ex.each(st, [&](int tid, EmptyState&) {
        if (tid == 0 && p.level == 1 && lh[nbins]) ex.global_atomic_add(&p.state->zeros, (unsigned long long)lh[nbins]);
    });
}

// one work-group of TIES_SELECT_THREADS
struct SceSelectParams {
    int level;                       // 1, 2 or 3
    unsigned long long n;            // elements of the tensor
    double select_topk;              // in (0, 1)
    const unsigned long long* hist;  // [HIST1_BINS] of this level
    SceState* state;                 // [1]
};
template <class Ex>
SM_HD void k_sce_select(Ex& ex, const SceSelectParams& p) {
    typename Ex::template State<TiesSelectState> st;
    ex.init(st);
    unsigned long long* part = (unsigned long long*)(ex.lds() + LDS_SCRATCH_FLOATS);     // [TIES_SELECT_THREADS]
    const int nbins = radix_bins(p.level);
    const unsigned long long* h = p.hist;
    SceState* s = p.state;
    // level 1: k_keep = floor(select_topk * nz) - one fp64 multiply and a truncation; every thread reads the same state
    // before the barrier below, the one thread that owns the rank writes it after
    const unsigned long long k_keep = p.level == 1 ? (unsigned long long)geo_dmul(p.select_topk, (double)(p.n - s->zeros)) : s->k_keep;
    const RadixState s0 = radix_start(p.level, k_keep, s->sel);
    ex.each(st, [&](int tid, TiesSelectState& t) { part[tid] = t.own = radix_own_sum(h, nbins, tid); });
    ex.sync();
    ex.each(st, [&](int tid, TiesSelectState& t) {
        if (k_keep == 0) {            // nothing is selected: the threshold is +inf and no key reaches SCE_KEY_NONE
            if (tid == 0 && p.level == 1) s->k_keep = 0;
            if (tid == 0 && p.level == 3) { s->tau_key = SCE_KEY_NONE; s->threshold = u2f(TIES_KEY_INF); s->selected = 0; }
            return;
        }
        const RadixFound f = radix_select_step(h, nbins, part, t.own, s0.rank, tid);
        if (!f.found) return;
        const RadixState s1 = s->sel = radix_advance(p.level, s0, f);
        if (p.level == 1) s->k_keep = k_keep;
        if (p.level == 3) {                                  // the bin is one key: tau; ties at it are all selected
            s->tau_key = s1.prefix;
            s->threshold = u2f(s1.prefix);
            s->selected = s1.above + (s1.prefix != 0u ? f.c : 0ull);     // (k_keep <= nz: tau > 0 always)
        }
    });
}

struct SceEnergyParams {
    TiesInputs in;
    int select;                 // 1: x_i = d_i where q >= tau and q > 0, +0 elsewhere; 0: x_i = d_i (selection skipped)
    const SceState* state;      // [1]: tau_key
    size_t nseg;                // segments of GEO_SEG_ELEMS elements
    int seg_vec;                // the pointers are 16-byte aligned (a segment starts at an octet boundary)
    double* part;               // [nseg][k]: the sums of each segment
    uint32_t* flags;            // [0]: bit i = finetune i has a non-finite delta
};
template <int KR> SM_HD size_t sce_energy_lds_floats() { return LDS_SCRATCH_FLOATS + (size_t)2 * KR * GEO_THREADS; }

template <int KR, class Ex>
SM_HD void k_sce_energy(Ex& ex, const SceEnergyParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const int nt = ex.nthreads();                                  // GEO_THREADS
    const int k = p.in.k;
    const size_t seg = (size_t)ex.bid();
    double* red = (double*)(ex.lds() + LDS_SCRATCH_FLOATS);        // [KR][nt] (LDS_SCRATCH_FLOATS is even)
    const size_t start = seg * GEO_SEG_ELEMS;
    const size_t len = p.in.n - start < GEO_SEG_ELEMS ? p.in.n - start : GEO_SEG_ELEMS;
    const uint32_t tau = p.select ? p.state->tau_key : 0u;
    ex.each(st, [&](int tid, EmptyState&) {
        double acc[KR];
#pragma unroll
        for (int i = 0; i < KR; ++i) acc[i] = 0.0;
        uint32_t bad = 0;
        for (size_t q = tid; q < segment_octets(len); q += nt) {
            const Octet o = segment_octet(start, len, p.seg_vec, q);
            float d[KR][8];
            uint32_t key[8];
            sce_delta8<KR>(p.in, o, d, bad);
            if (p.select) sce_key8<KR>(k, d, key);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                // (an element that is not selected, or past the end, is x = +0: its product +0 leaves the lane as it is)
                if (!p.select || (key[e] >= tau && key[e] != 0u)) {
#pragma unroll
                    for (int i = 0; i < KR; ++i)
                        if (i < k) acc[i] = geo_dadd(acc[i], geo_dmul((double)d[i][e], (double)d[i][e]));
                }
            }
        }
#pragma unroll
        for (int i = 0; i < KR; ++i)
            if (i < k) red[i * nt + tid] = acc[i];
        if (bad) ex.global_atomic_or_u32(p.flags, bad);
    });
    ex.sync();
    // the fixed binary tree of geo_gram: p[t] = p[t] + p[t + s] for t < s, s = nt / 2, nt / 4, ..., 1
    for (int s = nt >> 1; s > 0; s >>= 1) {
        ex.each(st, [&](int tid, EmptyState&) {
            if (tid >= s) return;
            for (int i = 0; i < k; ++i) {
                double* v = red + i * nt;
                v[tid] = geo_dadd(v[tid], v[tid + s]);
            }
        });
        ex.sync();
    }
    ex.each(st, [&](int tid, EmptyState&) {
        if (tid < k) p.part[seg * k + tid] = red[tid * nt];
    });
}

struct SceMergeParams {
    TiesInputs in;
    float w[TIES_MAX_MODELS];   // the weights of step 3 (alpha acts through them only)
    const void* base_out; int base_out_dtype;
    int out_is_base0;           // base_out is base[0] in the same dtype and the bases are shared: loaded once
    float lambda;
    int select;                 // as in SceEnergyParams
    const SceState* state;      // [1]: tau_key
    void* out;                  // base_out_dtype, [n]
    float* delta_out;           // optional fp32 [n]: lambda * M
    int chunks;                 // octets per thread
};
template <int KR, class Ex>
SM_HD void k_sce_merge(Ex& ex, const SceMergeParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const int k = p.in.k;
    const float eps = 1e-8f;
    const uint32_t tau = p.select ? p.state->tau_key : 0u;
    ex.each(st, [&](int tid, EmptyState&) {
        for (int q = 0; q < p.chunks; ++q) {
            Octet o;
            if (!octet_at(p.in, ex.bid(), ex.nthreads(), p.chunks, tid, q, o)) break;
            float d[KR][8], bo[8];
            uint32_t key[8], bad = 0;
            sce_delta8<KR>(p.in, o, d, bad);
            if (p.select) sce_key8<KR>(k, d, key);
            // (base_out last and, where it is the shared base, loaded again - the line is still in cache from sce_delta8 -
            // instead of delta_base_out8's copy: the k deltas leave no registers to hold the base that long)
            ties_load8(p.out_is_base0 ? p.in.base[0] : p.base_out, p.out_is_base0 ? p.in.dtype : p.base_out_dtype, o.i0, o.cnt, o.vec, bo);
            float r[8], dl[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const bool sel = !p.select || (key[e] >= tau && key[e] != 0u);
                // SCE's own election (not sm_delta.hpp's Election): the sum S is unweighted, the weights act on P / N alone
                float S = 0.f, P = 0.f, N = 0.f, DP = 0.f, DN = 0.f;
#pragma unroll
                for (int i = 0; i < KR; ++i) {
                    if (i < k) {
                        const float x = sel ? d[i][e] : 0.f;
                        S = aten_fadd_(S, x);
                        if (x > 0.f) { P = aten_fadd_(P, aten_fmul_(x, p.w[i])); DP = aten_fadd_(DP, p.w[i]); }
                        if (x < 0.f) { N = aten_fadd_(N, aten_fmul_(x, p.w[i])); DN = aten_fadd_(DN, p.w[i]); }
                    }
                }
                const bool pos = S >= 0.f;
                float M = pos ? P : N;
                float D = pos ? DP : DN;
                if (fabsf(D) < eps) D = 1.f;
                M = M / D;
                dl[e] = aten_fmul_(p.lambda, M);
                r[e] = aten_fadd_(bo[e], dl[e]);
            }
            delta_store8(p, o, r, dl);
        }
    });
}

// ---- kernel tags (sm_tag.hpp) and this header's share of group 7 of smhip_side.hip (smhip_device.hpp) ----
// the one-stream radix level over the variance scores, its scan, the masked ordered fp64 energies and their fold (the
// fold of sm_geo.hpp under its own profile name), the fused merge pass; k <= 4 deltas per octet in registers, or up to 16
SM_KERNEL_TAG_LB(KSceHist, SceHistParams, "sce_hist", k_sce_hist<SCE_REG_SMALL>(ex, p), 256, 4)
SM_KERNEL_TAG_LB(KSceHistAny, SceHistParams, "sce_hist", k_sce_hist<TIES_MAX_MODELS>(ex, p), 256, 2)
SM_KERNEL_TAG_LB(KSceSelect, SceSelectParams, "sce_select", k_sce_select(ex, p), TIES_SELECT_THREADS, 4)
SM_KERNEL_TAG_LB(KSceEnergy, SceEnergyParams, "sce_energy", k_sce_energy<SCE_REG_SMALL>(ex, p), GEO_THREADS, 4)
SM_KERNEL_TAG_LB(KSceEnergyAny, SceEnergyParams, "sce_energy", k_sce_energy<TIES_MAX_MODELS>(ex, p), GEO_THREADS, 2)
SM_KERNEL_TAG_LB(KSceFold, GeoFoldParams, "sce_energy_fold", k_geo_fold(ex, p), 256, 4)
SM_KERNEL_TAG_LB(KSceMerge, SceMergeParams, "sce_merge", k_sce_merge<SCE_REG_SMALL>(ex, p), 256, 4)
SM_KERNEL_TAG_LB(KSceMergeAny, SceMergeParams, "sce_merge", k_sce_merge<TIES_MAX_MODELS>(ex, p), 256, 2)
#define SM_KERNELS_SCE(X) X(KSceHist) X(KSceHistAny) X(KSceSelect) X(KSceEnergy) X(KSceEnergyAny) X(KSceFold) X(KSceMerge) X(KSceMergeAny)

}  // namespace smhip
