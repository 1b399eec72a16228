// sm_mx4.hpp - MXFP4: a model's 2-D weights as E2M1 codes, two to a byte, and one E8M0 power-of-two scale per block of
// 32 consecutive elements of a row - the OCP micro-scaling form of the 4-bit checkpoints (as recalled: PAPERS.md).  Not a
// merge operator: a DATA TYPE, a third representation of a model next to the delta pack and block-scaled FP8, which
// every operator takes through mx4_dequant.  The functions are stated in include/shardmerge_hip.h (smhip_mx4_quant,
// smhip_mx4_dequant, smhip_mx4_fn); every step of them is an integer function of the fp32 bit patterns, or one fp32
// product that is exact short of overflow, so the emulator and the device give the same bits.
//
// C % 32 == 0, so the blocks of a tensor are simply its n / 32 consecutive runs of 32 elements: block b owns elements
// 32 b .., code bytes 16 b .. and scale byte b.  THE UNIT OF WORK IS A BLOCK AND A LANE OWNS IT for its whole life;
// consecutive lanes own consecutive blocks, so a wave reads 4 KiB (8 KiB of fp32) and writes 1 KiB contiguously, and a
// work-group of 256 lanes owns 256 consecutive blocks per round: 256 scale bytes.
//
//   mx4_quant     four 16-byte loads (eight for fp32) back to back; the maximum over the 31 magnitude bits as integers
//                 (the 15 of a 16-bit type, widened once), which also shows a NaN or an Inf; the scale code from the
//                 maximum's exponent field; each element moved onto the E2M1 grid by an integer subtraction in its
//                 exponent field and rounded by an integer addition; the 32 codes packed into four words; ONE 16-byte
//                 store.  The scale byte goes to LDS; after the round's one barrier 16 lanes store 16 scale bytes each.
//                 The two sets of 256 staged bytes alternate from round to round, so a round costs ONE barrier (a wave
//                 reaches the round after next only through the next barrier, behind every read of this one).  The
//                 counters (zero blocks, saturated elements, non-finite blocks) are integers in the lane until the last
//                 round, where each wave folds them by six shifts and leaves them in its own LDS words before that
//                 round's barrier; three lanes add the four waves' words behind it: one global atomic per counter and
//                 work-group, no zeroing, no barrier of its own.
//   mx4_dequant   the mirror: 16 lanes load the round's 256 scale bytes into LDS by 16-byte loads, the barrier, then per
//                 lane one 16-byte load of codes, its scale byte, 32 arithmetic decodes (the fp32 bits are built from
//                 the three fields; no table) times the scale, and four 16-byte stores (eight for fp32).
//   mx4_fn        the probe behind smhip_mx4_fn: the four conversions alone over a flat array.
// A pointer that is not 16-byte aligned sends a call element by element through the same conversions; the last,
// partial round stores its scale bytes one by one where 16 do not fit.
#pragma once
#include "sm_minifloat.hpp"
#include "sm_tag.hpp"

namespace smhip {

constexpr int MX4_BLOCK = 32;                     // elements of a scale block
constexpr int MX4_THREADS = 256;                  // work-group: 256 lanes, 256 consecutive blocks per round
constexpr int MX4_LDS_FLOATS = 2 * MX4_THREADS / 4 + 16;   // beyond the scratch: [2][256] staged scale bytes, [4][4] wave counters
enum { MX4_F32_TO_E2M1 = 0, MX4_E2M1_TO_F32 = 1, MX4_AMAX_TO_E8M0 = 2, MX4_E8M0_TO_F32 = 3 };
enum { MX4_ZERO_BLOCKS = 0, MX4_SATURATED = 1, MX4_NONFINITE = 2, MX4_COUNTERS = 3 };
enum { MX4_FLAG_NAN_SCALE = 1u };

// ---- the encodings ----
// E2M1 (e2m1_bits, e2m1_to_f32, e2m1_of_bits, f32_to_e2m1) is sm_minifloat.hpp's: NVFP4's elements share it.
// E8M0: 2^(code - 127); 0xFF is NaN.  Code 0 is 2^-127, an fp32 denormal
SM_HD float e8m0_to_f32(uint32_t s) { return u2f(s == 0xffu ? 0x7fc00000u : (s ? s << 23 : 0x00400000u)); }
// the scale code of a block from its maximum's magnitude bits: max(E - 2, 0) with E the biased exponent field, that is
// 2^(floor(log2 a) - 2) wherever that is at least 2^-127; a zero or a denormal maximum gives code 0
SM_HD uint32_t amax_to_e8m0(uint32_t a) {
    const uint32_t e = a >> 23;
    return e > 2u ? e - 2u : 0u;
}
// |x| 2^(127 - s) as non-negative fp32 bits, from the magnitude bits m of x: exact - the subtraction is in the exponent
// field.  A result below 2^-126 (it rounds to code 0 in any case) is given as 0.  A denormal x is first written as the
// fp32 value of its mantissa (an exact conversion) times 2^-149; it matters for s <= 2 alone
SM_HD uint32_t mx4_scaled_bits(uint32_t m, uint32_t s) {
    int32_t t = (int32_t)m + (127 - (int32_t)s) * 0x00800000;
    if (m < 0x00800000u) t = (int32_t)f2u((float)(int32_t)m) - (22 + (int32_t)(s < 64u ? s : 64u)) * 0x00800000;
    return t < 0x00800000 ? 0u : (uint32_t)t;
}
// the code (sign included) of one element of a block with scale code s, from its fp32 bits
SM_HD uint32_t mx4_code_of(uint32_t u, uint32_t s, uint32_t* sat) {
    return ((u >> 28) & 8u) | e2m1_of_bits(mx4_scaled_bits(u & 0x7fffffffu, s), sat);
}
// one dequantised element: the product (exact short of overflow: two significant bits times a power of two), then one
// rounding into the dtype; its raw bits (a 16-bit type in the low half)
SM_HD uint32_t mx4_dequant_elem(uint32_t code, float scale, int dtype) {
    const float r = aten_fmul_(e2m1_to_f32(code), scale);
    return dtype == DT_F32 ? f2u(r) : (uint32_t)(dtype == DT_BF16 ? f_to_bf16_any(r) : f_to_f16_any(r));
}
// 16 bytes of LDS at a 16-byte aligned place
SM_HD u32x4 mx4_lds16(const uint8_t* p) {
    u32x4 v;
    memcpy(&v, __builtin_assume_aligned(p, 16), 16);
    return v;
}
SM_HD void mx4_put16(uint8_t* p, const u32x4& v) { memcpy(__builtin_assume_aligned(p, 16), &v, 16); }

struct Mx4QuantParams {
    const void* x; int dtype;   // [nblk][32]
    size_t nblk;                // R C / 32 blocks
    uint8_t* codes;             // [nblk][16]
    uint8_t* scale;             // [nblk]
    unsigned long long* counts; // [MX4_COUNTERS], zeroed by the host
    int vec;                    // x, codes and scale are 16-byte aligned: blocks move in 16-byte accesses
    int chunks;                 // rounds per work-group
};
struct Mx4QuantState { uint32_t cnt[4], got[4]; };   // the lane's counters (cnt[3] unused) and what a shift brings

// a lane's block as 32 fp32 bit patterns, and the maximum of their magnitude bits
template <bool VEC>
SM_HD uint32_t mx4_load_block(const Mx4QuantParams& p, size_t blk, uint32_t* w) {
    uint32_t a = 0;
    if (p.dtype == DT_F32) {
        if (VEC) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const u32x4 v = ((const u32x4*)p.x)[blk * 8 + j];
                w[4 * j] = v.x; w[4 * j + 1] = v.y; w[4 * j + 2] = v.z; w[4 * j + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 32; ++i) w[i] = ((const uint32_t*)p.x)[blk * 32 + i];
        }
#pragma unroll
        for (int i = 0; i < 32; ++i) a = umax(a, w[i] & 0x7fffffffu);
        return a;
    }
    uint32_t h[16];                                                 // packed as loaded: element 2 i in the low half
    if (VEC) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const u32x4 v = ((const u32x4*)p.x)[blk * 4 + j];
            h[4 * j] = v.x; h[4 * j + 1] = v.y; h[4 * j + 2] = v.z; h[4 * j + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i)
            h[i] = (uint32_t)((const uint16_t*)p.x)[blk * 32 + 2 * i] | ((uint32_t)((const uint16_t*)p.x)[blk * 32 + 2 * i + 1] << 16);
    }
    // both 16-bit types order like their 15 magnitude bits: the maximum of the halves, widened once
#pragma unroll
    for (int i = 0; i < 16; ++i) a = umax(a, umax(h[i] & 0x7fffu, (h[i] >> 16) & 0x7fffu));
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        if (p.dtype == DT_BF16) { w[2 * i] = h[i] << 16; w[2 * i + 1] = h[i] & 0xffff0000u; }
        else { w[2 * i] = f2u(f16_to_f(h[i] & 0xffffu)); w[2 * i + 1] = f2u(f16_to_f(h[i] >> 16)); }
    }
    return p.dtype == DT_BF16 ? a << 16 : f2u(f16_to_f(a));
}

// one lane, one block: the scale code; the codes are stored, the counters counted
template <bool VEC>
SM_HD uint32_t mx4_quant_block(const Mx4QuantParams& p, size_t blk, uint32_t* cnt) {
    uint32_t w[32];
    const uint32_t a = mx4_load_block<VEC>(p, blk, w);
    const uint32_t s = amax_to_e8m0(a);
    cnt[MX4_ZERO_BLOCKS] += a == 0u ? 1u : 0u;
    cnt[MX4_NONFINITE] += a >= 0x7f800000u ? 1u : 0u;               // (the call fails: the outputs are unspecified)
    uint32_t q[4], nsat = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        uint32_t word = 0;
#pragma unroll
        for (int e = 0; e < 8; ++e) {                               // element 2 j' in the low nibble of byte j'
            uint32_t sat;
            word |= mx4_code_of(w[8 * j + e], s, &sat) << (4 * e);
            nsat += sat;
        }
        q[j] = word;
    }
    cnt[MX4_SATURATED] += nsat;
    if (VEC) {
        ((u32x4*)p.codes)[blk] = u32x4{q[0], q[1], q[2], q[3]};
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) p.codes[blk * 16 + i] = (uint8_t)(q[i >> 2] >> (8 * (i & 3)));
    }
    return s;
}

template <class Ex>
SM_HD void k_mx4_quant(Ex& ex, const Mx4QuantParams& p) {
    typedef Mx4QuantState S;
    typename Ex::template State<S> st;
    ex.init(st);
    uint8_t* stage = (uint8_t*)(ex.lds() + LDS_SCRATCH_FLOATS);     // [2][256]: the round's scale bytes, the sets alternate
    uint32_t* wcnt = (uint32_t*)(stage + 2 * MX4_THREADS);          // [4][4]: the waves' counters
    ex.each(st, [&](int, S& s) { s.cnt[0] = s.cnt[1] = s.cnt[2] = s.cnt[3] = 0u; });
    for (int q = 0; q < p.chunks; ++q) {
        const size_t b0 = ((size_t)ex.bid() * p.chunks + q) * MX4_THREADS;
        uint8_t* set = stage + (q & 1) * MX4_THREADS;
        ex.each(st, [&](int tid, S& s) {
            const size_t blk = b0 + tid;
            if (blk >= p.nblk) return;
            if (p.vec) set[tid] = (uint8_t)mx4_quant_block<true>(p, blk, s.cnt);
            else p.scale[blk] = (uint8_t)mx4_quant_block<false>(p, blk, s.cnt);
        });
        if (q == p.chunks - 1) {                                    // the counters ride the last round's barrier
            static_for<0, 6>([&](auto step_c) {
                constexpr int DELTA = 32 >> decltype(step_c)::value;
                ex.template wave_shift_down<DELTA, 3>(st, [](S& s) { return (const uint32_t*)s.cnt; }, [](S& s) { return s.got; });
                ex.each(st, [&](int, S& s) { s.cnt[0] += s.got[0]; s.cnt[1] += s.got[1]; s.cnt[2] += s.got[2]; });
            });
            ex.each(st, [&](int tid, S& s) {
                if ((tid & 63) == 0) { wcnt[4 * (tid >> 6)] = s.cnt[0]; wcnt[4 * (tid >> 6) + 1] = s.cnt[1]; wcnt[4 * (tid >> 6) + 2] = s.cnt[2]; }
            });
        }
        ex.sync();
        ex.each(st, [&](int tid, S&) {
            if (p.vec && tid < 16 && b0 + 16 * tid < p.nblk) {
                if (b0 + 16 * tid + 16 <= p.nblk) {
                    ((u32x4*)p.scale)[b0 / 16 + tid] = mx4_lds16(set + 16 * tid);
                } else {                                            // the tensor ends inside these 16 blocks
                    for (size_t b = b0 + 16 * tid; b < p.nblk; ++b) p.scale[b] = set[b - b0];
                }
            }
            if (q == p.chunks - 1 && tid >= 64 && tid < 64 + MX4_COUNTERS) {    // (a wave the scale bytes leave idle)
                const int c = tid - 64;
                const uint32_t v = wcnt[c] + wcnt[4 + c] + wcnt[8 + c] + wcnt[12 + c];
                if (v) ex.global_atomic_add(&p.counts[c], (unsigned long long)v);
            }
        });
    }
}

struct Mx4DequantParams {
    const uint8_t* codes;       // [nblk][16]
    const uint8_t* scale;       // [nblk]
    size_t nblk;
    void* out; int out_dtype;   // [nblk][32]
    int vec;                    // codes, scale and out are 16-byte aligned
    int chunks;                 // rounds per work-group
    uint32_t* flags;            // [0]: MX4_FLAG_NAN_SCALE
};
template <class Ex>
SM_HD void k_mx4_dequant(Ex& ex, const Mx4DequantParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    uint8_t* stage = (uint8_t*)(ex.lds() + LDS_SCRATCH_FLOATS);     // [2][256]: the round's scale bytes, the sets alternate
    for (int q = 0; q < p.chunks; ++q) {
        const size_t b0 = ((size_t)ex.bid() * p.chunks + q) * MX4_THREADS;
        uint8_t* set = stage + (q & 1) * MX4_THREADS;
        ex.each(st, [&](int tid, EmptyState&) {
            if (!(p.vec && tid < 16 && b0 + 16 * tid < p.nblk)) return;
            if (b0 + 16 * tid + 16 <= p.nblk) {
                mx4_put16(set + 16 * tid, ((const u32x4*)p.scale)[b0 / 16 + tid]);
            } else {
                for (size_t b = b0 + 16 * tid; b < p.nblk; ++b) set[b - b0] = p.scale[b];
            }
        });
        ex.sync();
        ex.each(st, [&](int tid, EmptyState&) {
            const size_t blk = b0 + tid;
            if (blk >= p.nblk) return;
            const uint32_t s = p.vec ? set[tid] : p.scale[blk];
            if (s == 0xffu) ex.global_atomic_or_u32(p.flags, MX4_FLAG_NAN_SCALE);
            const float sc = e8m0_to_f32(s);
            uint32_t c[4];
            if (p.vec) {
                const u32x4 v = ((const u32x4*)p.codes)[blk];
                c[0] = v.x; c[1] = v.y; c[2] = v.z; c[3] = v.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    c[j] = (uint32_t)p.codes[blk * 16 + 4 * j] | ((uint32_t)p.codes[blk * 16 + 4 * j + 1] << 8) |
                           ((uint32_t)p.codes[blk * 16 + 4 * j + 2] << 16) | ((uint32_t)p.codes[blk * 16 + 4 * j + 3] << 24);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {                           // eight elements: one word of codes
                uint32_t w[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) w[e] = mx4_dequant_elem((c[j] >> (4 * e)) & 15u, sc, p.out_dtype);
                const size_t i0 = blk * 32 + 8 * j;
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

struct Mx4FnParams { int op; size_t n; const void* x; void* y; };   // float -> uint8 (ops 0, 2), uint8 -> float (ops 1, 3)
SM_HD void mx4_fn_elem(const Mx4FnParams& p, size_t i) {
    if (p.op == MX4_F32_TO_E2M1) ((uint8_t*)p.y)[i] = (uint8_t)f32_to_e2m1(((const float*)p.x)[i]);
    else if (p.op == MX4_AMAX_TO_E8M0) ((uint8_t*)p.y)[i] = (uint8_t)amax_to_e8m0(f2u(((const float*)p.x)[i]) & 0x7fffffffu);
    else if (p.op == MX4_E2M1_TO_F32) ((float*)p.y)[i] = e2m1_to_f32(((const uint8_t*)p.x)[i] & 15u);
    else ((float*)p.y)[i] = e8m0_to_f32(((const uint8_t*)p.x)[i]);
}
template <class Ex>
SM_HD void k_mx4_fn(Ex& ex, const Mx4FnParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    ex.each(st, [&](int tid, EmptyState&) {
        const size_t i = (size_t)ex.bid() * ex.nthreads() + tid;
        if (i < p.n) mx4_fn_elem(p, i);
    });
}

// ---- kernel tags (sm_tag.hpp) and group 25 of smhip_side.hip (smhip_device.hpp) ----
// the quantiser and the dequantiser (a block per lane, the scale bytes staged in LDS), the conversions' probe
SM_KERNEL_TAG_LB(KMx4Quant, Mx4QuantParams, "mx4_quant", k_mx4_quant(ex, p), MX4_THREADS, 4)
SM_KERNEL_TAG_LB(KMx4Dequant, Mx4DequantParams, "mx4_dequant", k_mx4_dequant(ex, p), MX4_THREADS, 4)
SM_KERNEL_TAG_LB(KMx4Fn, Mx4FnParams, "mx4_fn", k_mx4_fn(ex, p), 256, 4)
#define SM_SIDE_KERNELS_25(X) X(KMx4Quant) X(KMx4Dequant) X(KMx4Fn)

}  // namespace smhip
