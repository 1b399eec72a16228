// sm_fp8.hpp - block-scaled FP8: a model's 2-D weights as OCP E4M3 codes and one fp32 scale per 128 x 128 block, the
// form of the `quant_method: "fp8"` checkpoints (as recalled: PAPERS.md).  Not a merge operator: a DATA TYPE, a second
// representation of a model next to the delta pack, which every operator takes through fp8_dequant.  The functions are
// stated in include/shardmerge_hip.h (smhip_fp8_quant, smhip_fp8_dequant, smhip_fp8_fn); every step of them is an exact
// maximum, an integer function or one correctly rounded fp32 operation, so the kernels equal three lines of torch on the
// CPU bit for bit.
//
//   fp8_quant     ONE pass with the block in registers.  A work-group of 256 lanes takes one 128 x 128 block; lane t owns
//                 octet column t % 16 and rows t / 16 + 16 j, j = 0..7: eight 16-byte loads back to back (two per octet
//                 for fp32), one wave load instruction covers four whole row segments.  The 64 values stay in registers,
//                 packed as loaded for the 16-bit types.  The maximum is taken on the magnitude bits as integers (which
//                 also shows a NaN or an Inf): per lane, across the wave by six shifts, across the four waves through
//                 four words of LDS that alternate between two sets from block to block - ONE barrier per block.  Then
//                 the scale, the 64 divisions and conversions, one 8-byte store per octet: 16 lanes write the 128
//                 contiguous bytes of a block row.  Lane 0 writes the scale and the block's maximum; the report is the
//                 host's, from the blocks' maxima (no atomic, no counter).  Edge blocks, C % 8 != 0 and unaligned views
//                 go through ties_load8 with its cnt and byte stores.
//   fp8_dequant   the octet walk of the streaming passes: 8 bytes of codes, one scale (an octet never straddles a block
//                 column when C % 8 == 0), a 16-byte store (two for fp32).  The decode is arithmetic: two shifts and an
//                 add for a normal code, one integer conversion and a product for a subnormal one - no table, no LDS.
//   fp8_fn        the probe behind smhip_fp8_fn: the two conversions alone over a flat array.
#pragma once
#include "sm_delta.hpp"
#include "sm_minifloat.hpp"

namespace smhip {

constexpr int FP8_BLOCK = 128;                    // rows and columns of a scale block
constexpr int FP8_THREADS = 256;                  // work-group of fp8_quant: 16 octet columns x 16 rows, 8 times
constexpr uint32_t FP8_MIN_SCALE = 0x00800000u;   // 2^-126, the smallest normal fp32 value
enum { FP8_ENCODE = 0, FP8_DECODE = 1 };
enum { FP8_FLAG_NONFINITE = 1u, FP8_FLAG_NAN_CODE = 2u };

// (the encoding - e4m3_to_f32, f32_to_e4m3, FP8_MAX_KEY - is sm_minifloat.hpp's: NVFP4's block scales share it)

// the scale of a block from its maximum's key a (a finite magnitude): max(a / 448, 2^-126), one rounded fp32 division
SM_HD float fp8_scale_of(uint32_t a) {
    const float s = u2f(a) / 448.0f;
    return f2u(s) < FP8_MIN_SCALE ? u2f(FP8_MIN_SCALE) : s;
}
// the code of one element: one rounded fp32 division, then the conversion
SM_HD uint32_t fp8_code_of(float x, float s) { return f32_to_e4m3(x / s); }
SM_HD uint32_t fp8_pack4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return a | (b << 8) | (c << 16) | (d << 24); }

struct u32x2 { uint32_t x, y; };

struct Fp8QuantParams {
    const void* x; int dtype;   // [R][C]
    size_t R, C, BR, BC;        // BR = ceil(R / 128), BC = ceil(C / 128) blocks
    uint8_t* codes;             // [R][C]
    float* scale;               // [BR][BC]
    uint32_t* amax;             // [BR][BC], workspace: the key of each block's maximum (>= 0x7f800000: a NaN or an Inf)
    int vec;                    // C % 8 == 0, x 16-byte aligned, codes 8-byte aligned: whole blocks move in vector accesses
};
// the lane's 64 values: a whole block of a 16-bit type packed as loaded in w[0..31] (row j: w[4 j .. 4 j + 3]), anything
// else as fp32 bits (row j: w[8 j .. 8 j + 7]); m the running maximum's key, r what a shift brings
struct Fp8QuantState { uint32_t w[64]; uint32_t m, r; };

template <class Ex>
SM_HD void k_fp8_quant(Ex& ex, const Fp8QuantParams& p) {
    typedef Fp8QuantState S;
    typename Ex::template State<S> st;
    ex.init(st);
    uint32_t* wmax = (uint32_t*)(ex.lds() + LDS_SCRATCH_FLOATS);   // [2][4]: the waves' maxima, the sets alternate
    const size_t nblk = p.BR * p.BC;
    int set = 0;
    for (size_t blk = (size_t)ex.bid(); blk < nblk; blk += (size_t)ex.nblocks(), set ^= 4) {
        const size_t bi = blk / p.BC, bj = blk - bi * p.BC, r0 = bi * FP8_BLOCK, c0 = bj * FP8_BLOCK;
        const int rows = (int)((p.R - r0) < (size_t)FP8_BLOCK ? (p.R - r0) : (size_t)FP8_BLOCK);
        const int cols = (int)((p.C - c0) < (size_t)FP8_BLOCK ? (p.C - c0) : (size_t)FP8_BLOCK);
        const bool whole = p.vec && rows == FP8_BLOCK && cols == FP8_BLOCK;
        const bool packed = whole && p.dtype != DT_F32;
        ex.each(st, [&](int tid, S& s) {
            const int oc = tid & 15, rr = tid >> 4;
            uint32_t m = 0;
            if (packed) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const u32x4 v = ((const u32x4*)p.x)[((r0 + rr + 16 * j) * p.C + c0) / 8 + oc];
                    s.w[4 * j] = v.x; s.w[4 * j + 1] = v.y; s.w[4 * j + 2] = v.z; s.w[4 * j + 3] = v.w;
                }
                // both 16-bit types order like their 15 magnitude bits: the maximum of the halves, widened once
#pragma unroll
                for (int i = 0; i < 32; ++i) m = umax(m, umax(s.w[i] & 0x7fffu, (s.w[i] >> 16) & 0x7fffu));
                m = p.dtype == DT_BF16 ? m << 16 : f2u(f16_to_f(m));
            } else if (whole) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const size_t q = ((r0 + rr + 16 * j) * p.C + c0) / 4 + 2 * oc;
                    const u32x4 a = ((const u32x4*)p.x)[q], b = ((const u32x4*)p.x)[q + 1];
                    s.w[8 * j] = a.x; s.w[8 * j + 1] = a.y; s.w[8 * j + 2] = a.z; s.w[8 * j + 3] = a.w;
                    s.w[8 * j + 4] = b.x; s.w[8 * j + 5] = b.y; s.w[8 * j + 6] = b.z; s.w[8 * j + 7] = b.w;
                }
#pragma unroll
                for (int i = 0; i < 64; ++i) m = umax(m, s.w[i] & 0x7fffffffu);
            } else {                                                // an edge block, or a view that no vector access fits
                const int cnt = cols - 8 * oc < 0 ? 0 : (cols - 8 * oc < 8 ? cols - 8 * oc : 8);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    float f[8];
                    const int r = rr + 16 * j;
                    ties_load8(p.x, p.dtype, (r0 + r) * p.C + c0 + 8 * oc, r < rows ? cnt : 0, false, f);
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        s.w[8 * j + e] = f2u(f[e]);
                        m = umax(m, f2u(f[e]) & 0x7fffffffu);
                    }
                }
            }
            s.m = m;
        });
        static_for<0, 6>([&](auto step_c) {
            constexpr int DELTA = 32 >> decltype(step_c)::value;
            ex.template wave_shift_down<DELTA, 1>(st, [](S& s) { return (const uint32_t*)&s.m; }, [](S& s) { return &s.r; });
            ex.each(st, [&](int, S& s) { s.m = umax(s.m, s.r); });
        });
        ex.each(st, [&](int tid, S& s) {
            if ((tid & 63) == 0) wmax[set + (tid >> 6)] = s.m;
        });
        ex.sync();
        ex.each(st, [&](int tid, S& s) {
            const int oc = tid & 15, rr = tid >> 4;
            const uint32_t a = umax(umax(wmax[set], wmax[set + 1]), umax(wmax[set + 2], wmax[set + 3]));
            if (tid == 0) p.amax[blk] = a;
            if (a >= TIES_KEY_INF) return;                          // the call fails: the outputs are unspecified
            const float sc = fp8_scale_of(a);
            if (tid == 0) p.scale[blk] = sc;
            if (packed) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    float f[8];
                    decode16x8(u32x4{s.w[4 * j], s.w[4 * j + 1], s.w[4 * j + 2], s.w[4 * j + 3]}, p.dtype, f);
                    uint32_t c[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) c[e] = fp8_code_of(f[e], sc);
                    ((u32x2*)p.codes)[((r0 + rr + 16 * j) * p.C + c0) / 8 + oc] =
                        u32x2{fp8_pack4(c[0], c[1], c[2], c[3]), fp8_pack4(c[4], c[5], c[6], c[7])};
                }
            } else if (whole) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    uint32_t c[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) c[e] = fp8_code_of(u2f(s.w[8 * j + e]), sc);
                    ((u32x2*)p.codes)[((r0 + rr + 16 * j) * p.C + c0) / 8 + oc] =
                        u32x2{fp8_pack4(c[0], c[1], c[2], c[3]), fp8_pack4(c[4], c[5], c[6], c[7])};
                }
            } else {
                const int cnt = cols - 8 * oc < 0 ? 0 : (cols - 8 * oc < 8 ? cols - 8 * oc : 8);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int r = rr + 16 * j;
                    if (r >= rows) continue;
                    uint8_t* dst = p.codes + (r0 + r) * p.C + c0 + 8 * oc;
#pragma unroll
                    for (int e = 0; e < 8; ++e)
                        if (e < cnt) dst[e] = (uint8_t)fp8_code_of(u2f(s.w[8 * j + e]), sc);
                }
            }
        });
        // (no second barrier: the next block's maxima go to the other set, and a wave reaches the block after that only
        //  through the next barrier, behind every read of this one)
    }
}

struct Fp8DequantParams {
    const uint8_t* codes;       // [R][C]
    const float* scale;         // [ceil(R / 128)][BC]
    size_t R, C, PB, BC;        // PB = ceil(C / 8) octets per row, BC = ceil(C / 128)
    size_t units;               // R * PB row octets
    void* out; int out_dtype;   // [R][C]
    int row_vec;                // C % 8 == 0, codes 8-byte and out 16-byte aligned
    int chunks;                 // row octets per thread
    uint32_t* flags;            // [0]: FP8_FLAG_NAN_CODE
};
// one element: the product rounded once in fp32, then once into the dtype; its raw bits (a 16-bit type in the low half)
SM_HD uint32_t fp8_dequant_elem(uint32_t code, float s, int dtype) {
    const float r = aten_fmul_(e4m3_to_f32(code), s);
    return dtype == DT_F32 ? f2u(r) : (uint32_t)(dtype == DT_BF16 ? f_to_bf16_any(r) : f_to_f16_any(r));
}
template <class Ex>
SM_HD void k_fp8_dequant(Ex& ex, const Fp8DequantParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const int nt = ex.nthreads();
    ex.each(st, [&](int tid, EmptyState&) {
        uint32_t bad = 0;
        for (int q = 0; q < p.chunks; ++q) {
            const size_t u = ((size_t)ex.bid() * p.chunks + q) * nt + tid;
            if (u >= p.units) break;
            const size_t r = p.units <= 0xffffffffull ? (size_t)((uint32_t)u / (uint32_t)p.PB) : u / p.PB, o = u - r * p.PB;
            const size_t c0 = 8 * o, i0 = r * p.C + c0;
            const int cnt = (int)((p.C - c0) < 8 ? (p.C - c0) : 8);
            const float s = p.scale[(r / FP8_BLOCK) * p.BC + c0 / FP8_BLOCK];
            if (p.row_vec) {
                const u32x2 cw = ((const u32x2*)p.codes)[i0 / 8];
                uint32_t w[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const uint32_t c = ((e < 4 ? cw.x : cw.y) >> (8 * (e & 3))) & 0xffu;
                    if ((c & 0x7fu) == 0x7fu) bad = FP8_FLAG_NAN_CODE;
                    w[e] = fp8_dequant_elem(c, s, p.out_dtype);
                }
                if (p.out_dtype == DT_F32) {
                    ((u32x4*)p.out)[i0 / 4] = u32x4{w[0], w[1], w[2], w[3]};
                    ((u32x4*)p.out)[i0 / 4 + 1] = u32x4{w[4], w[5], w[6], w[7]};
                } else {
                    ((u32x4*)p.out)[i0 / 8] = u32x4{w[0] | (w[1] << 16), w[2] | (w[3] << 16), w[4] | (w[5] << 16), w[6] | (w[7] << 16)};
                }
            } else {                                                // a row octet that starts anywhere: element by element
                for (int e = 0; e < cnt; ++e) {
                    const uint32_t c = p.codes[i0 + e];
                    if ((c & 0x7fu) == 0x7fu) bad = FP8_FLAG_NAN_CODE;
                    const uint32_t w = fp8_dequant_elem(c, s, p.out_dtype);
                    if (p.out_dtype == DT_F32) ((uint32_t*)p.out)[i0 + e] = w;
                    else ((uint16_t*)p.out)[i0 + e] = (uint16_t)w;
                }
            }
        }
        if (bad) ex.global_atomic_or_u32(p.flags, bad);
    });
}

struct Fp8FnParams { int op; size_t n; const void* x; void* y; };   // ENCODE: float -> uint8; DECODE: uint8 -> float
template <class Ex>
SM_HD void k_fp8_fn(Ex& ex, const Fp8FnParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    ex.each(st, [&](int tid, EmptyState&) {
        const size_t i = (size_t)ex.bid() * ex.nthreads() + tid;
        if (i >= p.n) return;
        if (p.op == FP8_ENCODE) ((uint8_t*)p.y)[i] = (uint8_t)f32_to_e4m3(((const float*)p.x)[i]);
        else ((float*)p.y)[i] = e4m3_to_f32(((const uint8_t*)p.x)[i]);
    });
}

// ---- kernel tags (sm_tag.hpp) and group 24 of smhip_side.hip (smhip_device.hpp) ----
// the one-pass quantiser (a block per work-group, in registers), the streaming dequantiser, the conversions' probe
SM_KERNEL_TAG_LB(KFp8Quant, Fp8QuantParams, "fp8_quant", k_fp8_quant(ex, p), FP8_THREADS, 4)
SM_KERNEL_TAG_LB(KFp8Dequant, Fp8DequantParams, "fp8_dequant", k_fp8_dequant(ex, p), 256, 4)
SM_KERNEL_TAG_LB(KFp8Fn, Fp8FnParams, "fp8_fn", k_fp8_fn(ex, p), 256, 4)
#define SM_SIDE_KERNELS_24(X) X(KFp8Quant) X(KFp8Dequant) X(KFp8Fn)

}  // namespace smhip
