// sm_common.hpp - what every kernel header uses: the vector structs, the dtype codes and SigDesc, the conversions and
// loaders, WeightRanges, the small per-thread State structs and the LDS / histogram constants.
#pragma once
#include <cmath>
#include <cstring>

#include "fft_engine.hpp"

namespace smhip {

struct cf4 { float x, y, z, w; };
struct u32x4 { uint32_t x, y, z, w; };

enum { DT_BF16 = 0, DT_F16 = 1, DT_F32 = 2 };
enum { OUT_BF16 = 0, OUT_F32 = 1 };

// value = (load(x) - (base ? load(base) : 0)) * prescale
struct SigDesc {
    const void* x;
    const void* base;
    int dtype;
    float prescale;
};

SM_HD uint32_t umax(uint32_t a, uint32_t b) { return a > b ? a : b; }
SM_HD float u2f(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
SM_HD uint32_t f2u(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
SM_HD float bf16_to_f(uint32_t h) { return u2f(h << 16); }
SM_HD float f16_to_f(uint32_t h) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint16_t h16 = (uint16_t)h;                 // v_cvt_f32_f16
    _Float16 hv;
    memcpy(&hv, &h16, 2);
    return (float)hv;
#endif
    const uint32_t s = (h & 0x8000u) << 16, e = (h >> 10) & 0x1f, m = h & 0x3ff;
    if (e == 0) {
        if (m == 0) return u2f(s);
        float v = (float)m * 5.9604644775390625e-08f;   // m * 2^-24
        return (s ? -v : v);
    }
    if (e == 31) return u2f(s | 0x7f800000u | (m << 13));
    return u2f(s | ((e + 112) << 23) | (m << 13));
}
// round-to-nearest-even; caller guarantees v is not NaN
SM_HD uint16_t f_to_bf16(float v) {
    uint32_t u = f2u(v);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
// two floats -> packed bf16 pair (lo = a), round-to-nearest-even; neither is NaN
SM_HD uint32_t pack_bf16x2(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    const f32x2 v = {a, b};
    const bf16x2 h = __builtin_convertvector(v, bf16x2);      // v_cvt_pk_bf16_f32
    uint32_t u;
    memcpy(&u, &h, 4);
    return u;
#else
    return (uint32_t)f_to_bf16(a) | ((uint32_t)f_to_bf16(b) << 16);
#endif
}
// a ROUNDED fp32 product / sum (the device compiler contracts a * b + c into an fma otherwise)
SM_HD float aten_fmul_(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    float r = a * b; asm volatile("" : "+v"(r)); return r;
#else
    volatile float r = a * b; return r;
#endif
}
SM_HD float aten_fadd_(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    float r = a + b; asm volatile("" : "+v"(r)); return r;
#else
    volatile float r = a + b; return r;
#endif
}
SM_HD bool is_nan(float v) { return v != v; }
SM_HD bool is_inf(float v) { return (f2u(v) & 0x7fffffffu) == 0x7f800000u; }

SM_HD float load_elem(const void* p, int dtype, size_t i) {
    if (dtype == DT_F32) return ((const float*)p)[i];
    const uint32_t h = ((const uint16_t*)p)[i];
    return dtype == DT_BF16 ? bf16_to_f(h) : f16_to_f(h);
}
// 8 consecutive elements starting at i (i % 8 == 0, pointer 16-byte aligned)
SM_HD void load_elem8(const void* p, int dtype, size_t i, float* out) {
    if (dtype == DT_F32) {
        const cf4 a = ((const cf4*)p)[i / 4], b = ((const cf4*)p)[i / 4 + 1];
        out[0] = a.x; out[1] = a.y; out[2] = a.z; out[3] = a.w;
        out[4] = b.x; out[5] = b.y; out[6] = b.z; out[7] = b.w;
    } else {
        const u32x4 v = ((const u32x4*)p)[i / 8];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (dtype == DT_BF16) {
                out[2 * c] = u2f(w[c] << 16);
                out[2 * c + 1] = u2f(w[c] & 0xffff0000u);
            } else {
                out[2 * c] = f16_to_f(w[c] & 0xffffu);
                out[2 * c + 1] = f16_to_f(w[c] >> 16);
            }
        }
    }
}
// 8 packed 16-bit values (bf16 or f16) -> float
SM_HD void decode16x8(const u32x4& v, int dtype, float* out) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (dtype == DT_BF16) {
            out[2 * c] = u2f(w[c] << 16);
            out[2 * c + 1] = u2f(w[c] & 0xffff0000u);
        } else {
            out[2 * c] = f16_to_f(w[c] & 0xffffu);
            out[2 * c + 1] = f16_to_f(w[c] >> 16);
        }
    }
}
SM_HD void load_sig8(const SigDesc& s, size_t i, float* out) {
    if (!s.x) {
#pragma unroll
        for (int c = 0; c < 8; ++c) out[c] = 0.f;
        return;
    }
    load_elem8(s.x, s.dtype, i, out);
    if (s.base) {
        float b[8];
        load_elem8(s.base, s.dtype, i, b);
#pragma unroll
        for (int c = 0; c < 8; ++c) out[c] -= b[c];
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) out[c] *= s.prescale;
}
SM_HD float load_sig1(const SigDesc& s, size_t i) {
    if (!s.x) return 0.f;
    float v = load_elem(s.x, s.dtype, i);
    if (s.base) v -= load_elem(s.base, s.dtype, i);
    return v * s.prescale;
}

// weight of a half-spectrum bin column: columns 0 and C/2 (C even) hold all of
// their full-spectrum bins, every other column stands for itself and its
// conjugate twin (multiplicities for the order statistics).
// C < 0: the planes hold a full spectrum, every bin counts once.
SM_HD int bin_weight(int k2, int C) { return (C < 0 || k2 == 0 || (2 * k2 == C)) ? 1 : 2; }

// XCD-aware placement for the strided (column) passes.  Work-groups are dealt
// round-robin over the 8 XCDs (blocks b and b+8 share an L2): the G work-groups
// that touch the same 128-byte lines get block ids that are equal mod 8 and
// adjacent in dispatch order, so a line is fetched from HBM once per XCD-L2 and
// partial-line writes merge in that L2.  Speed only, never correctness.
// Returns the logical index for block id `bid`; the grid must be padded to a
// multiple of 8*G and logical indices >= count do nothing.
SM_HD int xcd_remap(int bid, int G) {
    const int per = 8 * G;
    const int y = bid / per, i = (bid % per) / 8, x = bid % 8;
    return (y * 8 + x) * G + i;
}

// multiplicity of plane element i (planes are [Cb][R]): 1 inside column 0 and
// column C/2, else 2 - two range tests instead of a division per element
struct WeightRanges {
    size_t hi0, loN, hiN;
    size_t period;      // > 0: the planes hold a BATCH of half spectra one after the other ((C/2+1)*R elements each)
    int full;
};
// Cb_total: bin columns in the planes; more than C/2 + 1 of them means a batch (rank > 2 tensors:
// the reference transforms the last two dims and takes every statistic over the whole tensor)
SM_HD WeightRanges weight_ranges(int R, int C, int Cb_total = 0) {
    WeightRanges w;
    w.full = C < 0;
    w.hi0 = (size_t)R;
    if (C >= 0 && (C % 2) == 0 && C > 0) { w.loN = (size_t)(C / 2) * R; w.hiN = w.loN + R; }
    else { w.loN = w.hiN = 0; }
    w.period = (C >= 0 && Cb_total > C / 2 + 1) ? (size_t)(C / 2 + 1) * R : 0;
    return w;
}
SM_HD uint32_t weight_at(const WeightRanges& w, size_t i) {
    if (w.period) i %= w.period;
    return (w.full || i < w.hi0 || (i >= w.loN && i < w.hiN)) ? 1u : 2u;
}

struct EmptyStateF { double red[2]; };
struct NormsState { double red[16]; };

struct FftState {
    float xr[EREG];
    float xi[EREG];
    double red[4];
    uint32_t fd[4], fr[4];     // the row pass's fused torch.norm summaries (aten_fused_rows); dead everywhere else
    int fep[2];                // ... and the predicted binades of this thread's group (per component)
};

constexpr int LDS_SCRATCH_FLOATS = 64 * 4;   // reduction scratch at the start of LDS
constexpr int HIST1_BINS = 2048;             // level 1: key >> 20
constexpr int HIST_LO_BINS = 1024;           // levels 2, 3: 10 bits each

struct EmptyState { double red[8]; unsigned long long keep[8]; };

SM_HD int sgn(float v) { return (v > 0.f) - (v < 0.f); }
// torch.sign(NaN) = NaN and NaN == NaN is False: NaNs never "agree"
// (on the bit patterns: |x| > inf is a NaN, |x| == 0 is a zero of either sign)
SM_HD bool same_sign(float a, float b) {
    const uint32_t ua = f2u(a), ub = f2u(b);
    const uint32_t ka = ua & 0x7fffffffu, kb = ub & 0x7fffffffu;
    const bool not_nan = ka <= 0x7f800000u && kb <= 0x7f800000u;
    const bool za = ka == 0u, zb = kb == 0u;
    const bool both_nonzero_same = !za && !zb && ((ua ^ ub) >> 31) == 0u;
    return not_nan && ((za && zb) || both_nonzero_same);
}

// rounding to a tensor's own dtype as torch does on CPU (a 16-bit elementwise op is an fp32 op rounded to the dtype)
SM_HD uint16_t f_to_bf16_any(float v) {            // RNE, NaN stays NaN
    const uint32_t u = f2u(v);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x0040u);
    return f_to_bf16(v);
}
SM_HD uint16_t f_to_f16_any(float v) {
#if defined(__HIP_DEVICE_COMPILE__)
    const _Float16 h = (_Float16)v;                   // v_cvt_f16_f32 (RNE)
    uint16_t r;
    memcpy(&r, &h, 2);
    return r;
#else
    const uint32_t u = f2u(v), sign = (u >> 16) & 0x8000u, a = u & 0x7fffffffu;
    if (a > 0x7f800000u) return (uint16_t)(sign | 0x7e00u);
    if (a >= 0x47800000u) return (uint16_t)(sign | 0x7c00u);              // >= 65536: Inf (65520 rounds up below)
    if (a < 0x33000000u) return (uint16_t)sign;                             // < 2^-25: zero
    int e = (int)(a >> 23) - 127;
    uint32_t m = (a & 0x7fffffu) | 0x800000u;
    int shift = (e < -14) ? (13 + (-14 - e)) : 13;                         // subnormal halves lose more bits
    uint32_t half = m >> shift, rem = m & ((1u << shift) - 1u), mid = 1u << (shift - 1);
    if (rem > mid || (rem == mid && (half & 1u))) ++half;
    uint32_t out = (e < -14) ? half : (((uint32_t)(e + 15) << 10) + (half - 0x400u));
    return (uint16_t)(sign | out);
#endif
}
SM_HD float round_to_dtype(float v, int dtype) {
    if (dtype == DT_F32) return v;
    if (dtype == DT_BF16) return bf16_to_f(f_to_bf16_any(v));
    return f16_to_f(f_to_f16_any(v));
}
SM_HD float sign_of(float v) { return is_nan(v) ? v : (float)sgn(v); }      // torch.sign(NaN) = NaN

// the constants of a pair's class blend (the slerp reduction writes them: sm_select.hpp) and the blend of one bin
struct BlendConsts {
    float thr;        // cutoff threshold (0 when cutoff_pct == 0)
    float dot;        // clamped cosine between the slerp-class vectors
    float cos_t, sin_t;
    float inv_rel;    // 1 / max(||v1 - dot v0||, 1e-12)
    float pad[3];
    double s00, s01, s11;
    unsigned long long n_slerp;
};

SM_HD float blend_slerp_one(const BlendConsts& c, float t_sum, float a, float b) {      // = blend_one(), BLEND_SLERP
    if (same_sign(a, b)) {
        if (fabsf(b) < c.thr) return a + t_sum * b;
        return a * c.cos_t + ((b - a * c.dot) * c.inv_rel) * c.sin_t;
    }
    return (fabsf(a) > fabsf(b)) ? a : b;
}

}  // namespace smhip
