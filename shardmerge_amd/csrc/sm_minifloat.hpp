// sm_minifloat.hpp - the two small float encodings the on-disk data types share: OCP E4M3 "fn" (sm_fp8.hpp's elements,
// sm_nv4.hpp's block scales) and E2M1 (the elements of sm_mx4.hpp and sm_nv4.hpp).  Plain integer arithmetic on the
// fp32 bit patterns and one rounded fp32 addition: the emulator and the device give the same bits.  The functions are
// stated in include/shardmerge_hip.h (smhip_fp8_fn, smhip_mx4_fn).
#pragma once
#include "sm_common.hpp"

namespace smhip {

constexpr uint32_t FP8_MAX_KEY = 0x43e00000u;     // 448.0f, the largest finite E4M3 value

// ---- OCP E4M3 "fn" - bias 7, no infinities, NaN is S.1111.111, largest finite value 448 ----
// exact.  A NaN code gives the quiet NaN torch's conversion gives (sign | 0x7ff00000)
SM_HD float e4m3_to_f32(uint32_t code) {
    const uint32_t s = (code & 0x80u) << 24, a = code & 0x7fu;
    if (a == 0x7fu) return u2f(s | 0x7ff00000u);
    if (a < 8u) {                                                   // subnormal: m 2^-9 (and the zeros)
        const float v = (float)(int)a * 0.001953125f;
        return u2f(s | f2u(v));
    }
    return u2f(s | ((a << 20) + 0x3c000000u));                      // exponent e - 7 + 127, three mantissa bits on top
}
// round to nearest even on the E4M3 grid, subnormals included; saturating: a |v| that rounds above 448 gives +-448, an
// Inf too; NaN gives 0x7F
SM_HD uint32_t f32_to_e4m3(float v) {
    const uint32_t u = f2u(v), s = (u >> 24) & 0x80u;
    uint32_t a = u & 0x7fffffffu;
    if (a > 0x7f800000u) return 0x7fu;
    if (a >= FP8_MAX_KEY) return s | 0x7eu;                         // [448, 464] rounds to 448; beyond it the clamp
    if (a < 0x3c800000u) {                                          // |v| < 2^-6: the subnormal grid of step 2^-9.
        // 2^14 has an ulp of 2^-9: ONE rounded addition leaves RNE(|v| 2^9) in the low mantissa bits (8: 2^-6 itself)
        return s | (f2u(aten_fadd_(u2f(a), 16384.0f)) - 0x46800000u);
    }
    a += 0x7ffffu + ((a >> 20) & 1u);                               // RNE to three mantissa bits; a carry moves the exponent
    return s | ((a >> 20) - 960u);                                  // (127 - 7) << 3
}

// ---- E2M1: sign, two exponent bits of bias 1, one mantissa bit: +-{0, 0.5, 1, 1.5, 2, 3, 4, 6}; no NaN, no infinity ----
// exact; the bits are built from the three fields
SM_HD uint32_t e2m1_bits(uint32_t code) {
    const uint32_t s = (code & 8u) << 28, e = (code >> 1) & 3u, m = code & 1u;
    return s | (e ? ((e + 126u) << 23) | (m << 22) : m * 0x3f000000u);
}
SM_HD float e2m1_to_f32(uint32_t code) { return u2f(e2m1_bits(code)); }
// the code (0..7) of a magnitude given as non-negative fp32 bits, and whether it rounds above 6: round to nearest, ties
// to the even mantissa.  From 1 up one integer addition rounds to one mantissa bit (a carry moves the exponent); below
// 1 the grid is {0, 0.5, 1}: a tie at 0.25 goes to 0 and one at 0.75 to 1.  Everything from 7 up, Inf and NaN included,
// is saturated to 6
SM_HD uint32_t e2m1_of_bits(uint32_t a, uint32_t* sat) {
    const uint32_t r = ((a + 0x1fffffu + ((a >> 22) & 1u)) >> 22) - 252u;        // (a >= 1.0: r >= 2)
    const uint32_t low = (a > 0x3e800000u ? 1u : 0u) + (a >= 0x3f400000u ? 1u : 0u);
    const uint32_t c = a < 0x3f800000u ? low : r;
    *sat = c > 7u ? 1u : 0u;
    return c > 7u ? 7u : c;
}
SM_HD uint32_t f32_to_e2m1(float v) {
    uint32_t sat;
    const uint32_t u = f2u(v);
    return ((u >> 28) & 8u) | e2m1_of_bits(u & 0x7fffffffu, &sat);
}

}  // namespace smhip
