// sm_nv4.hpp - NVFP4: a model's 2-D weights as E2M1 codes, two to a byte, one E4M3 scale per block of 16 consecutive
// elements of a row and ONE fp32 scale for the whole tensor - the 4-bit form ModelOpt writes (as recalled: PAPERS.md).
// Not a merge operator: a DATA TYPE, a fourth representation of a model next to the delta pack, block-scaled FP8 and
// MXFP4, which every operator takes through nv4_dequant.  The functions are stated in include/shardmerge_hip.h
// (smhip_nv4_quant, smhip_nv4_dequant).  Unlike MXFP4 the scales are no powers of two: the tensor's maximum must exist
// before any block can be coded, and real fp32 divisions and products enter - each is ONE correctly rounded operation of
// its own, so the emulator and the device give the same bits.  The encodings are sm_minifloat.hpp's.
//
// C % 16 == 0, so the blocks of a tensor are its n / 16 consecutive runs of 16 elements.  A block is 32 bytes of a
// 16-bit type and its codes are 8 bytes - HALF a lane's natural 16-byte store.  So THE UNIT OF WORK IS A PAIR OF BLOCKS
// AND A LANE OWNS IT: 32 consecutive elements, code bytes 16 p .. and scale bytes 2 p, 2 p + 1 of pair p.  Consecutive
// lanes own consecutive pairs; a work-group of 256 lanes owns 512 consecutive blocks per round: 512 scale bytes.  The
// tensor's last pair is a lone block when n / 16 is odd: its second half is neither read nor written.
//
//   nv4_amax      the octet walk: 16 bytes per lane and round (32 of fp32), an integer maximum over the magnitude bits
//                 (the 15 of a 16-bit type compared packed, widened once at the end), folded across the wave by six
//                 shifts and across the four waves through four words of LDS; ONE global atomic maximum on a uint32 per
//                 work-group - exact and order-free, no floating-point atomic.  The same word shows a NaN or an Inf
//                 (>= 0x7f800000).  The host does not read it between the kernels.
//   nv4_quant     reads that word and forms g = max(A / 2688, 2^-126) itself.  Per lane four 16-byte loads (eight for
//                 fp32) back to back, two block maxima, two scale codes sc = e4m3((a / 6) / g), two block scales
//                 d = e4m3(sc) g, 32 divisions |x| / d rounded onto the E2M1 grid, the codes packed into four words,
//                 ONE 16-byte store.  The two scale bytes go to LDS; behind the round's one barrier 32 lanes store 16
//                 scale bytes each.  Two sets of 512 staged bytes alternate from round to round, so a round costs ONE
//                 barrier (a wave reaches the round after next only through the next barrier, behind every read of this
//                 one).  The counters are integers in the lane until the last round, where each wave folds them by six
//                 shifts into its own LDS words before that round's barrier; four lanes add the waves' words behind
//                 it: one global atomic per counter and work-group.
//   nv4_dequant   the mirror: 32 lanes load the round's 512 scale bytes into LDS by 16-byte loads, the barrier, then per
//                 lane one 16-byte load of codes, two block scales, 32 arithmetic decodes and products, four 16-byte
//                 stores (eight for fp32).
// A pointer that is not 16-byte aligned sends a call element by element through the same conversions; the last,
// partial round stores its scale bytes one by one where 16 do not fit.
#pragma once
#include "sm_minifloat.hpp"
#include "sm_tag.hpp"

namespace smhip {

constexpr int NV4_BLOCK = 16;                     // elements of a scale block
constexpr int NV4_THREADS = 256;                  // work-group: 256 lanes, 256 pairs of blocks per round
constexpr int NV4_LDS_FLOATS = 2 * 2 * NV4_THREADS / 4 + 16;   // beyond the scratch: [2][512] staged scale bytes, [4][4] wave counters
constexpr uint32_t NV4_MIN_GLOBAL = 0x00800000u;  // 2^-126, the smallest global scale
enum { NV4_ZERO_BLOCKS = 0, NV4_ZERO_SCALE = 1, NV4_SATURATED = 2, NV4_NONFINITE = 3, NV4_COUNTERS = 4 };
enum { NV4_FLAG_NAN_SCALE = 1u };

// ---- the function's steps, each one rounded fp32 operation ----
// the tensor's scale from its maximum's magnitude bits: max(A / 2688, 2^-126); 2688 = 6 * 448
SM_HD float nv4_global_of(uint32_t A) {
    const float g = u2f(A) / 2688.0f;
    return f2u(g) < NV4_MIN_GLOBAL ? u2f(NV4_MIN_GLOBAL) : g;
}
// a block's scale code from its maximum's magnitude bits: two divisions, then the E4M3 rounding (it saturates at 448)
SM_HD uint32_t nv4_scale_code(uint32_t a, float g) {
    const float sixth = u2f(a) / 6.0f;
    return f32_to_e4m3(sixth / g);
}
// what a block's elements are divided by, and multiplied by again: one product
SM_HD float nv4_block_scale(uint32_t sc, float g) { return aten_fmul_(e4m3_to_f32(sc), g); }
// one dequantised element: the product, then one rounding into the dtype; its raw bits (a 16-bit type in the low half)
SM_HD uint32_t nv4_dequant_elem(uint32_t code, float d, int dtype) {
    const float r = aten_fmul_(e2m1_to_f32(code), d);
    return dtype == DT_F32 ? f2u(r) : (uint32_t)(dtype == DT_BF16 ? f_to_bf16_any(r) : f_to_f16_any(r));
}
// the global maximum of a uint32 (the emulator runs the work-groups one after another)
SM_HD void nv4_atomic_max(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMax(p, v);
#else
    if (*p < v) *p = v;
#endif
}
// 16 bytes of LDS at a 16-byte aligned place
SM_HD u32x4 nv4_lds16(const uint8_t* p) {
    u32x4 v;
    memcpy(&v, __builtin_assume_aligned(p, 16), 16);
    return v;
}
SM_HD void nv4_put16(uint8_t* p, const u32x4& v) { memcpy(__builtin_assume_aligned(p, 16), &v, 16); }

// ---- nv4_amax ----
struct Nv4AmaxParams {
    const void* x; int dtype;   // [n]
    size_t n;                   // R C elements, a multiple of 16
    uint32_t* amax;             // one word, zeroed by the host: the maximum's magnitude bits as fp32
    int vec;                    // x is 16-byte aligned
    int chunks;                 // octets per lane
};
struct Nv4AmaxState { uint32_t m, r; };

template <class Ex>
SM_HD void k_nv4_amax(Ex& ex, const Nv4AmaxParams& p) {
    typedef Nv4AmaxState S;
    typename Ex::template State<S> st;
    ex.init(st);
    uint32_t* wmax = (uint32_t*)(ex.lds() + LDS_SCRATCH_FLOATS);    // [4]: the waves' maxima
    const size_t noct = p.n / 8;
    const int nt = ex.nthreads();
    ex.each(st, [&](int tid, S& s) {
        uint32_t m = 0;                                             // a 16-bit type: the packed 15 magnitude bits
        for (int q = 0; q < p.chunks; ++q) {
            const size_t u = ((size_t)ex.bid() * p.chunks + q) * nt + tid;
            if (u >= noct) break;
            if (p.dtype == DT_F32) {
                uint32_t w[8];
                if (p.vec) {
                    const u32x4 a = ((const u32x4*)p.x)[2 * u], b = ((const u32x4*)p.x)[2 * u + 1];
                    w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w; w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) w[e] = ((const uint32_t*)p.x)[8 * u + e];
                }
#pragma unroll
                for (int e = 0; e < 8; ++e) m = umax(m, w[e] & 0x7fffffffu);
            } else if (p.vec) {
                const u32x4 v = ((const u32x4*)p.x)[u];
                m = umax(m, umax(umax(v.x & 0x7fffu, (v.x >> 16) & 0x7fffu), umax(v.y & 0x7fffu, (v.y >> 16) & 0x7fffu)));
                m = umax(m, umax(umax(v.z & 0x7fffu, (v.z >> 16) & 0x7fffu), umax(v.w & 0x7fffu, (v.w >> 16) & 0x7fffu)));
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) m = umax(m, (uint32_t)((const uint16_t*)p.x)[8 * u + e] & 0x7fffu);
            }
        }
        // both 16-bit types order like their 15 magnitude bits: widened once
        s.m = p.dtype == DT_F32 ? m : (p.dtype == DT_BF16 ? m << 16 : f2u(f16_to_f(m)));
    });
    static_for<0, 6>([&](auto step_c) {
        constexpr int DELTA = 32 >> decltype(step_c)::value;
        ex.template wave_shift_down<DELTA, 1>(st, [](S& s) { return (const uint32_t*)&s.m; }, [](S& s) { return &s.r; });
        ex.each(st, [&](int, S& s) { s.m = umax(s.m, s.r); });
    });
    ex.each(st, [&](int tid, S& s) {
        if ((tid & 63) == 0) wmax[tid >> 6] = s.m;
    });
    ex.sync();
    ex.each(st, [&](int tid, S&) {
        if (tid != 0) return;
        const uint32_t a = umax(umax(wmax[0], wmax[1]), umax(wmax[2], wmax[3]));
        if (a) nv4_atomic_max(p.amax, a);
    });
}

// ---- nv4_quant ----
struct Nv4QuantParams {
    const void* x; int dtype;   // [nblk][16]
    size_t nblk;                // R C / 16 blocks
    uint8_t* codes;             // [nblk][8]
    uint8_t* scale;             // [nblk] E4M3 codes
    const uint32_t* amax;       // the word nv4_amax left
    float* global;              // where work-group 0 leaves g for the host
    unsigned long long* counts; // [NV4_COUNTERS], zeroed by the host
    int vec;                    // x, codes and scale are 16-byte aligned: pairs move in 16-byte accesses
    int chunks;                 // rounds per work-group
};
struct Nv4QuantState { uint32_t cnt[4], got[4]; };                  // the lane's counters and what a shift brings

// a lane's pair as 32 fp32 bit patterns (the second block zeros when nb == 1: it is not read) and the maxima of the
// blocks' magnitude bits
template <bool VEC>
SM_HD void nv4_load_pair(const Nv4QuantParams& p, size_t pair, int nb, uint32_t* w, uint32_t* a) {
    a[0] = a[1] = 0;
    if (p.dtype == DT_F32) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            u32x4 v = u32x4{0u, 0u, 0u, 0u};
            if (j < 4 || nb == 2) {
                if (VEC) {
                    v = ((const u32x4*)p.x)[pair * 8 + j];
                } else {
                    const uint32_t* s = (const uint32_t*)p.x + pair * 32 + 4 * j;
                    v = u32x4{s[0], s[1], s[2], s[3]};
                }
            }
            w[4 * j] = v.x; w[4 * j + 1] = v.y; w[4 * j + 2] = v.z; w[4 * j + 3] = v.w;
        }
#pragma unroll
        for (int i = 0; i < 32; ++i) a[i >> 4] = umax(a[i >> 4], w[i] & 0x7fffffffu);
        return;
    }
    uint32_t h[16];                                                 // packed as loaded: element 2 i in the low half
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        u32x4 v = u32x4{0u, 0u, 0u, 0u};
        if (j < 2 || nb == 2) {
            if (VEC) {
                v = ((const u32x4*)p.x)[pair * 4 + j];
            } else {
                const uint16_t* s = (const uint16_t*)p.x + pair * 32 + 8 * j;
                v = u32x4{(uint32_t)s[0] | ((uint32_t)s[1] << 16), (uint32_t)s[2] | ((uint32_t)s[3] << 16),
                          (uint32_t)s[4] | ((uint32_t)s[5] << 16), (uint32_t)s[6] | ((uint32_t)s[7] << 16)};
            }
        }
        h[4 * j] = v.x; h[4 * j + 1] = v.y; h[4 * j + 2] = v.z; h[4 * j + 3] = v.w;
    }
    // both 16-bit types order like their 15 magnitude bits: the maximum of the halves, widened once
#pragma unroll
    for (int i = 0; i < 16; ++i) a[i >> 3] = umax(a[i >> 3], umax(h[i] & 0x7fffu, (h[i] >> 16) & 0x7fffu));
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        if (p.dtype == DT_BF16) { w[2 * i] = h[i] << 16; w[2 * i + 1] = h[i] & 0xffff0000u; }
        else { w[2 * i] = f2u(f16_to_f(h[i] & 0xffffu)); w[2 * i + 1] = f2u(f16_to_f(h[i] >> 16)); }
    }
#pragma unroll
    for (int b = 0; b < 2; ++b) a[b] = p.dtype == DT_BF16 ? a[b] << 16 : f2u(f16_to_f(a[b]));
}

// one lane, one pair of nb blocks: the two scale codes; the codes are stored, the counters counted
template <bool VEC>
SM_HD void nv4_quant_pair(const Nv4QuantParams& p, size_t pair, int nb, float g, uint32_t* cnt, uint32_t* sc) {
    uint32_t w[32], a[2], q[4];
    nv4_load_pair<VEC>(p, pair, nb, w, a);
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        sc[b] = nv4_scale_code(a[b], g);
        const float d = nv4_block_scale(sc[b], g);
        const bool dead = d == 0.0f;                                // every code is its sign bit alone
        const uint32_t live = b < nb ? 1u : 0u;
        cnt[NV4_ZERO_BLOCKS] += (a[b] == 0u ? 1u : 0u) & live;
        cnt[NV4_ZERO_SCALE] += (a[b] != 0u && dead ? 1u : 0u) & live;
        cnt[NV4_NONFINITE] += (a[b] >= 0x7f800000u ? 1u : 0u) & live;   // (the call fails: the outputs are unspecified)
        uint32_t nsat = 0;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            uint32_t word = 0;
#pragma unroll
            for (int e = 0; e < 8; ++e) {                           // element 2 j' in the low nibble of byte j'
                const uint32_t u = w[16 * b + 8 * j + e];
                uint32_t sat;
                const float quot = u2f(u & 0x7fffffffu) / d;
                const uint32_t c = e2m1_of_bits(f2u(quot) & 0x7fffffffu, &sat);
                word |= (((u >> 28) & 8u) | (dead ? 0u : c)) << (4 * e);
                nsat += dead ? 0u : sat;
            }
            q[2 * b + j] = word;
        }
        cnt[NV4_SATURATED] += nsat;                                 // (a block that is not there is all zeros: dead)
    }
    if (VEC) {
        if (nb == 2) {
            ((u32x4*)p.codes)[pair] = u32x4{q[0], q[1], q[2], q[3]};
        } else {
            ((uint32_t*)p.codes)[4 * pair] = q[0];
            ((uint32_t*)p.codes)[4 * pair + 1] = q[1];
        }
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i)
            if (i < 8 * nb) p.codes[pair * 16 + i] = (uint8_t)(q[i >> 2] >> (8 * (i & 3)));
    }
}

template <class Ex>
SM_HD void k_nv4_quant(Ex& ex, const Nv4QuantParams& p) {
    typedef Nv4QuantState S;
    typename Ex::template State<S> st;
    ex.init(st);
    uint8_t* stage = (uint8_t*)(ex.lds() + LDS_SCRATCH_FLOATS);     // [2][512]: the round's scale bytes, the sets alternate
    uint32_t* wcnt = (uint32_t*)(stage + 4 * NV4_THREADS);          // [4][4]: the waves' counters
    const size_t npair = (p.nblk + 1) / 2;
    const float g = nv4_global_of(*p.amax);                         // every lane forms it itself: no readback before this kernel
    ex.each(st, [&](int tid, S& s) {
        s.cnt[0] = s.cnt[1] = s.cnt[2] = s.cnt[3] = 0u;
        if (ex.bid() == 0 && tid == 0) *p.global = g;
    });
    for (int q = 0; q < p.chunks; ++q) {
        const size_t b0 = ((size_t)ex.bid() * p.chunks + q) * NV4_THREADS;      // the round's first pair
        uint8_t* set = stage + (q & 1) * 2 * NV4_THREADS;
        ex.each(st, [&](int tid, S& s) {
            const size_t pair = b0 + tid;
            if (pair >= npair) return;
            const int nb = 2 * pair + 1 < p.nblk ? 2 : 1;
            uint32_t sc[2];
            if (p.vec) {
                nv4_quant_pair<true>(p, pair, nb, g, s.cnt, sc);
                set[2 * tid] = (uint8_t)sc[0];
                set[2 * tid + 1] = (uint8_t)sc[1];
            } else {
                nv4_quant_pair<false>(p, pair, nb, g, s.cnt, sc);
                p.scale[2 * pair] = (uint8_t)sc[0];
                if (nb == 2) p.scale[2 * pair + 1] = (uint8_t)sc[1];
            }
        });
        if (q == p.chunks - 1) {                                    // the counters ride the last round's barrier
            static_for<0, 6>([&](auto step_c) {
                constexpr int DELTA = 32 >> decltype(step_c)::value;
                ex.template wave_shift_down<DELTA, 4>(st, [](S& s) { return (const uint32_t*)s.cnt; }, [](S& s) { return s.got; });
                ex.each(st, [&](int, S& s) { s.cnt[0] += s.got[0]; s.cnt[1] += s.got[1]; s.cnt[2] += s.got[2]; s.cnt[3] += s.got[3]; });
            });
            ex.each(st, [&](int tid, S& s) {
                if ((tid & 63) == 0) {
                    uint32_t* mine = wcnt + 4 * (tid >> 6);
                    mine[0] = s.cnt[0]; mine[1] = s.cnt[1]; mine[2] = s.cnt[2]; mine[3] = s.cnt[3];
                }
            });
        }
        ex.sync();
        ex.each(st, [&](int tid, S&) {
            const size_t B = 2 * b0 + 16 * (size_t)tid;             // 16 blocks: 16 staged scale bytes
            if (p.vec && tid < 32 && B < p.nblk) {
                if (B + 16 <= p.nblk) {
                    ((u32x4*)p.scale)[B / 16] = nv4_lds16(set + 16 * tid);
                } else {                                            // the tensor ends inside these 16 blocks
                    for (size_t b = B; b < p.nblk; ++b) p.scale[b] = set[b - 2 * b0];
                }
            }
            if (q == p.chunks - 1 && tid >= 64 && tid < 64 + NV4_COUNTERS) {    // (a wave the scale bytes leave idle)
                const int c = tid - 64;
                const uint32_t v = wcnt[c] + wcnt[4 + c] + wcnt[8 + c] + wcnt[12 + c];
                if (v) ex.global_atomic_add(&p.counts[c], (unsigned long long)v);
            }
        });
    }
}

// ---- nv4_dequant ----
struct Nv4DequantParams {
    const uint8_t* codes;       // [nblk][8]
    const uint8_t* scale;       // [nblk] E4M3 codes
    float global;               // g: finite and positive (checked by the host)
    size_t nblk;
    void* out; int out_dtype;   // [nblk][16]
    int vec;                    // codes, scale and out are 16-byte aligned
    int chunks;                 // rounds per work-group
    uint32_t* flags;            // [0]: NV4_FLAG_NAN_SCALE
};
template <class Ex>
SM_HD void k_nv4_dequant(Ex& ex, const Nv4DequantParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    uint8_t* stage = (uint8_t*)(ex.lds() + LDS_SCRATCH_FLOATS);     // [2][512]: the round's scale bytes, the sets alternate
    const size_t npair = (p.nblk + 1) / 2;
    for (int q = 0; q < p.chunks; ++q) {
        const size_t b0 = ((size_t)ex.bid() * p.chunks + q) * NV4_THREADS;
        uint8_t* set = stage + (q & 1) * 2 * NV4_THREADS;
        ex.each(st, [&](int tid, EmptyState&) {
            const size_t B = 2 * b0 + 16 * (size_t)tid;
            if (!(p.vec && tid < 32 && B < p.nblk)) return;
            if (B + 16 <= p.nblk) {
                nv4_put16(set + 16 * tid, ((const u32x4*)p.scale)[B / 16]);
            } else {
                for (size_t b = B; b < p.nblk; ++b) set[b - 2 * b0] = p.scale[b];
            }
        });
        ex.sync();
        ex.each(st, [&](int tid, EmptyState&) {
            const size_t pair = b0 + tid;
            if (pair >= npair) return;
            const int nb = 2 * pair + 1 < p.nblk ? 2 : 1;
            uint32_t s[2];
            s[0] = p.vec ? set[2 * tid] : p.scale[2 * pair];
            s[1] = nb == 2 ? (p.vec ? set[2 * tid + 1] : p.scale[2 * pair + 1]) : 0u;
            if ((s[0] & 0x7fu) == 0x7fu || (s[1] & 0x7fu) == 0x7fu) ex.global_atomic_or_u32(p.flags, NV4_FLAG_NAN_SCALE);
            const float d[2] = {nv4_block_scale(s[0], p.global), nv4_block_scale(s[1], p.global)};
            uint32_t c[4] = {0u, 0u, 0u, 0u};
            if (p.vec) {
                if (nb == 2) {
                    const u32x4 v = ((const u32x4*)p.codes)[pair];
                    c[0] = v.x; c[1] = v.y; c[2] = v.z; c[3] = v.w;
                } else {
                    c[0] = ((const uint32_t*)p.codes)[4 * pair];
                    c[1] = ((const uint32_t*)p.codes)[4 * pair + 1];
                }
            } else {
#pragma unroll
                for (int i = 0; i < 16; ++i)
                    if (i < 8 * nb) c[i >> 2] |= (uint32_t)p.codes[pair * 16 + i] << (8 * (i & 3));
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {                           // eight elements: one word of codes, block j / 2
                if ((j >> 1) >= nb) continue;
                uint32_t w[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) w[e] = nv4_dequant_elem((c[j] >> (4 * e)) & 15u, d[j >> 1], p.out_dtype);
                const size_t i0 = pair * 32 + 8 * j;
                if (!p.vec) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        if (p.out_dtype == DT_F32) ((uint32_t*)p.out)[i0 + e] = w[e];
                        else ((uint16_t*)p.out)[i0 + e] = (uint16_t)w[e];
                    }
                } else if (p.out_dtype == DT_F32) {
                    ((u32x4*)p.out)[i0 / 4] = u32x4{w[0], w[1], w[2], w[3]};
                    ((u32x4*)p.out)[i0 / 4 + 1] = u32x4{w[4], w[5], w[6], w[7]};
                } else {
                    ((u32x4*)p.out)[i0 / 8] = u32x4{w[0] | (w[1] << 16), w[2] | (w[3] << 16), w[4] | (w[5] << 16), w[6] | (w[7] << 16)};
                }
            }
        });
    }
}

// ---- kernel tags (sm_tag.hpp) and group 27 of smhip_side.hip (smhip_device.hpp) ----
// the tensor's maximum (the octet walk, one atomic per work-group), the quantiser and the dequantiser (a pair of blocks
// per lane, the scale bytes staged in LDS)
SM_KERNEL_TAG_LB(KNv4Amax, Nv4AmaxParams, "nv4_amax", k_nv4_amax(ex, p), NV4_THREADS, 4)
SM_KERNEL_TAG_LB(KNv4Quant, Nv4QuantParams, "nv4_quant", k_nv4_quant(ex, p), NV4_THREADS, 4)
SM_KERNEL_TAG_LB(KNv4Dequant, Nv4DequantParams, "nv4_dequant", k_nv4_dequant(ex, p), NV4_THREADS, 4)
#define SM_SIDE_KERNELS_27(X) X(KNv4Amax) X(KNv4Quant) X(KNv4Dequant)

}  // namespace smhip
