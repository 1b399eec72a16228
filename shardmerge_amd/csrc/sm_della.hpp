// sm_della.hpp - DELLA merge (Deep et al. 2024, "DELLA-Merging"; mergekit's della / della_linear): DARE whose keep
// probability rises with the rank of each entry's magnitude within its row.  The function is stated in
// include/shardmerge_hip.h (smhip_della_merge).  The rank is exact and ties share a rank, the mask is the counter-based
// function of sm_dare.hpp, the threshold an fp64 chain of single rounded operations: the kernels equal a plain
// restatement bit for bit.
//
//   della_table  T as a function of the rank: c entries, fp64 in the kernel, once per call (with a constant instead of
//                the formula it fills threshold_out of a call that ranks nothing).
//   della_rank   one work-group per (finetune, row): the row's c magnitude keys go to LDS (4 c bytes, padded to a power
//                of two with all-ones keys), an in-place bitonic network sorts them, and each element's rank is the
//                lower bound of its key in the sorted row; T = table[rank] goes to the workspace as uint16.
//   della_merge  the fused streaming pass of dare_merge with a threshold and a rescale per element: per octet and
//                finetune one 16-byte load of eight T from the workspace, one Philox block, the fp32 chain.  The walk
//                (over the slab's octets of the flat index), the loader, the election, the kept counters: sm_delta.hpp.
// The sort: the strides 4, 2, 1 of every merge step run in registers (a thread owns 8 consecutive keys: two 16-byte LDS
// accesses each way), the strides from 8 up two at a time (4 keys per thread), so a 32768-key row is 55 passes over
// LDS instead of 120.
#pragma once
#include "sm_dare.hpp"

namespace smhip {

constexpr int DELLA_MAX_COLS = 32768;          // 4 bytes * 32768 = 128 KiB of the 160 KiB LDS, next to the scratch
constexpr uint32_t DELLA_PAD_KEY = 0xffffffffu;  // above every 31-bit magnitude

// step 4 of the definition: every operation rounded once, in this order
SM_HD uint32_t della_threshold(double p_lo, double w, uint32_t r, uint32_t c) {
    double p = p_lo;
    if (c > 1) {
        const double num = w * (double)r;
        const double q = num / (double)(c - 1);
        p = p_lo + q;
    }
    const double t = floor(p * 65536.0);
    const uint32_t T = (uint32_t)t;
    return T < 65535u ? T : 65535u;
}

struct DellaTableParams {
    uint16_t* out;              // [count]
    size_t count;
    uint32_t c;                 // row length: entry r is T of rank r
    double p_lo, w;             // density - epsilon, 2 * epsilon
    uint32_t fill;              // != 0: every entry is this value (the uniform threshold)
};
template <class Ex>
SM_HD void k_della_table(Ex& ex, const DellaTableParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    ex.each(st, [&](int tid, EmptyState&) {
        const size_t i = (size_t)ex.bid() * ex.nthreads() + tid;
        if (i < p.count) p.out[i] = (uint16_t)(p.fill ? p.fill : della_threshold(p.p_lo, p.w, (uint32_t)i, p.c));
    });
}

// the slab of whole rows that one rank / merge round works on.  Element j of the tensor (e0 <= j < e0 + rows * c) has its
// T at ws[i * stride + (j - (e0 & ~7))]: octets of the FLAT index stay 16-byte aligned in the workspace whatever e0.
struct DellaSlab {
    size_t e0;                  // first element
    size_t len;                 // rows * c
    size_t stride;              // uint16 entries per finetune, a multiple of 8
    uint16_t* ws;               // [k][stride]
};

struct DellaRankParams {
    TiesInputs in;              // the whole tensor
    DellaSlab slab;
    int c, rows;                // row length, rows of the slab
    int P;                      // c rounded up to a power of two, at least 8
    const uint16_t* table;      // [c]
    uint16_t* threshold_out;    // optional [k][n]
    uint32_t* flags;            // [0]: bit i = finetune i has a non-finite delta
};

SM_HD void della_cmpx(uint32_t& a, uint32_t& b, bool up) {
    const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
    a = up ? lo : hi;
    b = up ? hi : lo;
}

template <class Ex>
SM_HD void k_della_rank(Ex& ex, const DellaRankParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    uint32_t* keys = (uint32_t*)(ex.lds() + LDS_SCRATCH_FLOATS);      // [P]
    const int nt = ex.nthreads();
    const int i = ex.bid() % p.in.k;                                  // (the k work-groups of a row are neighbours: its base stays in L2)
    const size_t row0 = p.slab.e0 + (size_t)(ex.bid() / p.in.k) * p.c;
    const int c = p.c, P = p.P;
    const void* ft = p.in.ft[i];
    const void* bs = p.in.base[p.in.shared_base ? 0 : i];
    const bool vec = p.in.aligned && (c % 8 == 0) && (row0 % 8 == 0);
    // the keys of the row, the padding
    ex.each(st, [&](int tid, EmptyState&) {
        uint32_t bad = 0;
        if (vec) {
            for (int o = tid; o < P / 8; o += nt) {
                uint32_t kk[8];
                if (8 * o < c) {
                    float f[8], b[8];
                    load_elem8(ft, p.in.dtype, row0 + 8 * (size_t)o, f);
                    load_elem8(bs, p.in.dtype, row0 + 8 * (size_t)o, b);
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        kk[e] = f2u(f[e] - b[e]) & 0x7fffffffu;
                        if (kk[e] >= TIES_KEY_INF) bad = 1u;
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) kk[e] = DELLA_PAD_KEY;
                }
                u32x4 w0, w1;
                w0.x = kk[0]; w0.y = kk[1]; w0.z = kk[2]; w0.w = kk[3];
                w1.x = kk[4]; w1.y = kk[5]; w1.z = kk[6]; w1.w = kk[7];
                ((u32x4*)keys)[2 * o] = w0; ((u32x4*)keys)[2 * o + 1] = w1;
            }
        } else {
            for (int j = tid; j < P; j += nt) {
                uint32_t key = DELLA_PAD_KEY;
                if (j < c) {
                    key = f2u(load_elem(ft, p.in.dtype, row0 + j) - load_elem(bs, p.in.dtype, row0 + j)) & 0x7fffffffu;
                    if (key >= TIES_KEY_INF) bad = 1u;
                }
                keys[j] = key;
            }
        }
        if (bad) ex.global_atomic_or_u32(p.flags, 1u << i);
    });
    ex.sync();
    // the bitonic network, ascending.  A compare-exchange of positions a < b inside a merge step of size k2 sorts upwards
    // iff (a & k2) == 0.  First every block of 8 through its steps of size 2, 4 and 8 in registers ...
    auto tail8 = [&](int tid, int k2) {
        for (int g = tid; g < P / 8; g += nt) {
            const u32x4 w0 = ((const u32x4*)keys)[2 * g], w1 = ((const u32x4*)keys)[2 * g + 1];
            uint32_t v[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
            if (k2 == 8) {                                            // the first pass: steps 2, 4 and 8 of this block
#pragma unroll
                for (int e = 0; e < 8; e += 2) della_cmpx(v[e], v[e + 1], (e & 2) == 0);
#pragma unroll
                for (int e = 0; e < 8; ++e) if (!(e & 2)) della_cmpx(v[e], v[e + 2], (e & 4) == 0);
#pragma unroll
                for (int e = 0; e < 8; e += 2) della_cmpx(v[e], v[e + 1], (e & 4) == 0);
            }
            const bool up = ((8 * g) & k2) == 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) della_cmpx(v[e], v[e + 4], up);
#pragma unroll
            for (int e = 0; e < 8; ++e) if (!(e & 2)) della_cmpx(v[e], v[e + 2], up);
#pragma unroll
            for (int e = 0; e < 8; e += 2) della_cmpx(v[e], v[e + 1], up);
            u32x4 o0, o1;
            o0.x = v[0]; o0.y = v[1]; o0.z = v[2]; o0.w = v[3];
            o1.x = v[4]; o1.y = v[5]; o1.z = v[6]; o1.w = v[7];
            ((u32x4*)keys)[2 * g] = o0; ((u32x4*)keys)[2 * g + 1] = o1;
        }
    };
    ex.each(st, [&](int tid, EmptyState&) { tail8(tid, 8); });
    ex.sync();
    // ... then the steps of size 16 .. P: strides from k2 / 2 down to 8 through LDS, two at a time where two are left
    for (int k2 = 16; k2 <= P; k2 <<= 1) {
        int j = k2 >> 1;
        while (j >= 8) {
            if (j >= 16) {                                            // strides j and h = j / 2: positions a, a + h, a + j, a + j + h
                const int h = j >> 1;
                ex.each(st, [&](int tid, EmptyState&) {
                    for (int q = tid; q < P / 4; q += nt) {
                        const int a = ((q & ~(h - 1)) << 2) | (q & (h - 1));
                        const bool up = (a & k2) == 0;
                        uint32_t v0 = keys[a], v1 = keys[a + h], v2 = keys[a + j], v3 = keys[a + j + h];
                        della_cmpx(v0, v2, up); della_cmpx(v1, v3, up);
                        della_cmpx(v0, v1, up); della_cmpx(v2, v3, up);
                        keys[a] = v0; keys[a + h] = v1; keys[a + j] = v2; keys[a + j + h] = v3;
                    }
                });
                j >>= 2;
            } else {
                ex.each(st, [&](int tid, EmptyState&) {
                    for (int q = tid; q < P / 2; q += nt) {
                        const int a = ((q & ~(j - 1)) << 1) | (q & (j - 1));
                        uint32_t v0 = keys[a], v1 = keys[a + j];
                        della_cmpx(v0, v1, (a & k2) == 0);
                        keys[a] = v0; keys[a + j] = v1;
                    }
                });
                j >>= 1;
            }
            ex.sync();
        }
        ex.each(st, [&](int tid, EmptyState&) { tail8(tid, k2); });
        ex.sync();
    }
    // the rank of a key: how many keys of the sorted row are strictly smaller - its lower bound (P is a power of two)
    auto rank_of = [&](uint32_t key) {
        int pos = 0;
        for (int s = P >> 1; s >= 1; s >>= 1)
            if (keys[pos + s - 1] < key) pos += s;
        return pos;
    };
    uint16_t* ws = p.slab.ws + (size_t)i * p.slab.stride - (p.slab.e0 & ~(size_t)7);      // indexed by the flat element
    uint16_t* tout = p.threshold_out ? p.threshold_out + (size_t)i * p.in.n : nullptr;
    ex.each(st, [&](int tid, EmptyState&) {
        if (vec) {
            for (int o = tid; o < c / 8; o += nt) {
                const size_t j0 = row0 + 8 * (size_t)o;
                float f[8], b[8];
                load_elem8(ft, p.in.dtype, j0, f);
                load_elem8(bs, p.in.dtype, j0, b);
                uint32_t T[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) T[e] = p.table[rank_of(f2u(f[e] - b[e]) & 0x7fffffffu)];
                u32x4 w;
                w.x = T[0] | (T[1] << 16); w.y = T[2] | (T[3] << 16); w.z = T[4] | (T[5] << 16); w.w = T[6] | (T[7] << 16);
                *(u32x4*)(ws + j0) = w;
                if (tout) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) tout[j0 + e] = (uint16_t)T[e];
                }
            }
        } else {
            for (int j = tid; j < c; j += nt) {
                const uint32_t key = f2u(load_elem(ft, p.in.dtype, row0 + j) - load_elem(bs, p.in.dtype, row0 + j)) & 0x7fffffffu;
                const uint16_t T = p.table[rank_of(key)];
                ws[row0 + j] = T;
                if (tout) tout[row0 + j] = T;
            }
        }
    });
}

struct DellaMergeParams {
    TiesInputs in;              // the whole tensor
    DellaSlab slab;
    float alpha[TIES_MAX_MODELS];
    uint32_t stream_id[TIES_MAX_MODELS];
    uint64_t key;
    int rescale;                // 1: a kept entry times fp32(65536 / T) of ITS T, an fp64 division in the kernel
    const void* base_out; int base_out_dtype;
    int out_is_base0;
    float lambda;
    int normalize;
    int sign_election;          // 1: della, 0: della_linear
    void* out;
    float* delta_out;
    unsigned long long* kept;   // [k], device
    uint32_t* flags;
    int chunks;                 // octets per thread
};

template <class Ex>
SM_HD void k_della_merge(Ex& ex, const DellaMergeParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const int nt = ex.nthreads();
    const int k = p.in.k;
    uint32_t* lc = (uint32_t*)(ex.lds() + LDS_SCRATCH_FLOATS);     // [k][nt], then the totals (dare_lds_words)
    const size_t lo = p.slab.e0, hi = p.slab.e0 + p.slab.len;      // the slab's elements; its octets are those of the FLAT index
    const uint16_t* ws0 = p.slab.ws - (lo & ~(size_t)7);
    kept_zero(ex, st, lc, k);
    ex.each(st, [&](int tid, EmptyState&) {
        uint32_t bad = 0;
        const float Dall = delta_weight_sum(p.alpha, k);
        // (an octet cut by the slab's edge: its elements below o.lo are the slab's before - loaded, never kept or stored)
        for (int q = 0; q < p.chunks; ++q) {
            Octet o;
            if (!octet_at(lo, hi, p.in.aligned, ex.bid(), nt, p.chunks, tid, q, o)) break;
            float b[8], bo[8];
            delta_base8(p.in, o, b);
            delta_base_out8(p, o, b, bo);
            Election el;
            el.clear();
            for (int i = 0; i < k; ++i) {
                float f[8];
                delta_load8(p.in, i, o, b, f);
                const u32x4 tw = *(const u32x4*)(ws0 + (size_t)i * p.slab.stride + o.i0);   // eight T: one 16-byte load
                const uint32_t tws[4] = {tw.x, tw.y, tw.z, tw.w};
                uint32_t h[8];
                dare_draws8(p.key, p.stream_id[i], (uint64_t)o.i0, h);
                const float al = p.alpha[i];
                uint32_t nkept = 0;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const uint32_t T = (e & 1) ? (tws[e >> 1] >> 16) : (tws[e >> 1] & 0xffffu);
                    const float d = f[e] - b[e];
                    const uint32_t mag = delta_key(d);
                    if (mag >= TIES_KEY_INF) bad |= 1u << i;
                    const bool kept = e >= o.lo && h[e] < T && mag != 0u;
                    nkept += kept ? 1u : 0u;
                    float tv = 0.f;
                    if (kept) {
                        const float s = p.rescale ? (float)(65536.0 / (double)T) : 1.f;
                        tv = aten_fmul_(aten_fmul_(d, s), al);
                    }
                    el.add(e, tv, al, p.sign_election);
                }
                lc[i * nt + tid] += nkept;
            }
            float r[8], dl[8];
            el.finish(p.sign_election, p.normalize, Dall, p.lambda, bo, r, dl);
            delta_store8(p, o, r, dl);
        }
        if (bad) ex.global_atomic_or_u32(p.flags, bad);
    });
    kept_fold(ex, st, lc, k, p.kept);
}

// ---- kernel tags (sm_tag.hpp) and this header's share of group 7 of smhip_side.hip (smhip_device.hpp) ----
// T as a function of the rank, the whole-row sort in LDS (one work-group per finetune and row, up to 1024 threads), the
// fused pass with a threshold per element
SM_KERNEL_TAG_LB(KDellaTable, DellaTableParams, "della_table", k_della_table(ex, p), 256, 4)
SM_KERNEL_TAG_LB(KDellaRank, DellaRankParams, "della_rank", k_della_rank(ex, p), 1024, 4)
SM_KERNEL_TAG_LB(KDellaMerge, DellaMergeParams, "della_merge", k_della_merge(ex, p), 256, 4)
#define SM_KERNELS_DELLA(X) X(KDellaTable) X(KDellaRank) X(KDellaMerge)

}  // namespace smhip
