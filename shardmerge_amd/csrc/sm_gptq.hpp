// sm_gptq.hpp - group-quantised INT4 in the GPTQ tensor layout: a Linear's W [R = out][C = in] as X.qweight I32 [C / 8][R]
// (eight 4-bit codes of consecutive INPUT columns to a word), X.scales F16 [C / g][R], X.qzeros I32 [C / g][R / 8] (eight
// zero-points of consecutive OUTPUT rows to a word, stored minus one) and X.g_idx I32 [C] (as recalled: PAPERS.md).  Not
// a merge operator: a DATA TYPE, a fifth representation of a model next to the delta pack, block-scaled FP8, MXFP4 and
// NVFP4, which every operator takes through gptq_dequant.  The functions are stated in include/shardmerge_hip.h
// (smhip_gptq_quant, smhip_gptq_dequant): plain fp32 operations, each rounded once, so the emulator and the device give
// the same bits.
//
// The other three formats pack along a row of W and a lane owns a block.  Here the weight is stored TRANSPOSED: the
// eight elements a lane loads with one 16-byte read become ONE word that belongs in a column of qweight, and the
// minimum and maximum of a group lie across lanes.  THE UNIT OF WORK IS A TILE: 64 rows by one group of g = 32, 64 or
// 128 columns, g / 8 = OPR = 4, 8 or 16 octets per row.  A work-group of 256 lanes covers it in NP = g / 32 = 1, 2 or 4
// passes of 256 / OPR = 64, 32 or 16 rows: OPR consecutive lanes run along C and read one row's g elements as one run of
// 2 g (fp32: 4 g) bytes, a 16-byte load each (two for fp32).  Tile u of the tensor is row tile u / (C / g), group
// u % (C / g); a work-group takes `chunks` consecutive tiles, one per round.
//
//   gptq_quant    A  every lane folds its octets (kept in registers) to a minimum and a maximum and leaves them in the
//                    LDS planes pmn / pmx [OPR][S]; a NaN or an Inf makes the maximum a NaN.        -- barrier 1
//                 B  64 lanes, one per row, fold the row's OPR partials (min and max are exact: no order), form s16 and
//                    z and leave s16 (fp32 and its fp16 code) and z in LDS; they count the group.     -- barrier 2
//                 C  every lane quantises its octets into one word each and writes it to the LDS tile [OPR][S] - the
//                    transpose; it counts the clipped elements.                                      -- barrier 3
//                 D  the tile leaves as OPR rows of 64 consecutive words, 256-byte runs; eight lanes pack the 64
//                    zero-points into eight words and store the 64 scales as eight 16-byte pieces, one 128-byte run;
//                    the first row tile writes the group's g_idx.
//                 Three barriers a tile and nothing staged twice: round q + 1 writes pmn / pmx behind barrier 3 of round
//                 q, whose readers (B) stood before barrier 2; s16 / z are rewritten behind barrier 1 of q + 1, the tile
//                 behind barrier 2 of q + 1, and D of round q ends before a wave reaches either.  The counters are
//                 integers in LDS (lds_atomic_add), flushed in D of the work-group's last round: one global atomic per
//                 counter and work-group.
//   gptq_dequant  the mirror, ONE barrier a round on two alternating LDS sets: the tile's OPR x 64 words are read along
//                 o (256-byte runs) into the LDS tile, wave 1 reads the 64 scales, wave 2 the eight zero words, wave 3
//                 checks the group's g_idx (first row tile only); behind the barrier every lane takes its word out of
//                 the tile - the transpose -, decodes the eight nibbles arithmetically ((q - z) * s16, no table) and
//                 stores them along C, 16 bytes (fp32: 32).
// THE PADDING.  In A, C and the decode a wave's 64 lanes touch tile[j][r] for OPR values of j and 64 / OPR consecutive
// r; with a row stride S = 64 + 64 / OPR (68, 72, 80 words) the word addresses j S + r are 64 different residues modulo
// 64: no two lanes of a wave meet in a bank, whether the LDS has 32 or 64 of them.  The accesses along o (B, D, the
// dequantiser's loads) are 64 consecutive words.
// Rows past R (a partial tile; R % 8 == 0) are neither read nor written.  x / out that are not 16-byte aligned go
// element by element, scales that are not go half by half; qweight, qzeros and g_idx are words.
#pragma once
#include "sm_common.hpp"
#include "sm_tag.hpp"

namespace smhip {

constexpr int GPTQ_THREADS = 256;                 // work-group
constexpr int GPTQ_ROWS = 64;                     // rows of a tile
constexpr int GPTQ_PLANE = 16 * (GPTQ_ROWS + 4);  // words of an LDS plane [OPR][S] at its largest (g = 128: 16 x 68)
// beyond the scratch - quant: pmn, pmx, the tile; s16 [64]; z [64]; the fp16 codes [64 halves]; the counters [4]
constexpr int GPTQ_QUANT_LDS_FLOATS = 3 * GPTQ_PLANE + 64 + 64 + 32 + 4;
// dequant: two sets of the tile, s16 [64], z [64]
constexpr int GPTQ_DEQUANT_SET = GPTQ_PLANE + 64 + 64;
constexpr int GPTQ_DEQUANT_LDS_FLOATS = 2 * GPTQ_DEQUANT_SET;
enum { GPTQ_ZERO_GROUPS = 0, GPTQ_SCALE_CLAMPED = 1, GPTQ_CLIPPED = 2, GPTQ_NONFINITE = 3, GPTQ_COUNTERS = 4 };
enum { GPTQ_FLAG_ACT_ORDER = 1u, GPTQ_FLAG_NONFINITE_SCALE = 2u };

// ---- the function's steps, each one rounded fp32 operation ----
// the fp16 code of a group's scale from its clamped extremes mn <= 0 <= mx: (mx - mn) / 15 rounded to fp16 and clamped
// into [2^-24, 65504] (codes 0x0001 .. 0x7bff); *moved: a clamp changed it
SM_HD uint32_t gptq_scale_code(float mn, float mx, uint32_t* moved) {
    const float r = mx - mn;
    const float s = r / 15.0f;
    const uint32_t h = f_to_f16_any(s);                             // (s >= 0, +Inf or a NaN)
    *moved = (h == 0u || h > 0x7bffu) ? 1u : 0u;
    return h == 0u ? 1u : (h > 0x7bffu ? 0x7bffu : h);
}
// the zero-point: -mn / s16 rounded to the nearest integer, ties to even, clamped into 0 .. 15 (a NaN gives 0)
SM_HD uint32_t gptq_zero_of(float mn, float s16) {
    const float z = rintf((0.0f - mn) / s16);
    return (uint32_t)(int)fminf(fmaxf(z, 0.0f), 15.0f);
}
// one code: rint(x / s16) + z clamped into 0 .. 15; *clip: it left that range
SM_HD uint32_t gptq_code_of(float x, float s16, float z, uint32_t* clip) {
    const float t = rintf(x / s16) + z;
    *clip += (t < 0.0f || t > 15.0f) ? 1u : 0u;
    return (uint32_t)(int)fminf(fmaxf(t, 0.0f), 15.0f);
}
// one dequantised element: (q - z) as an exact integer, one product, one rounding into the dtype; its raw bits
SM_HD uint32_t gptq_dequant_elem(uint32_t q, uint32_t z, float s16, int dtype) {
    const float r = aten_fmul_((float)((int)q - (int)z), s16);
    return dtype == DT_F32 ? f2u(r) : (uint32_t)(dtype == DT_BF16 ? f_to_bf16_any(r) : f_to_f16_any(r));
}
// eight consecutive elements from element i on (i % 8 == 0), promoted exactly
SM_HD void gptq_load8(const void* x, int dtype, size_t i, int vec, float* out) {
    if (vec) { load_elem8(x, dtype, i, out); return; }
#pragma unroll
    for (int e = 0; e < 8; ++e) out[e] = load_elem(x, dtype, i + e);
}
// 16 bytes of LDS at a 16-byte aligned place
SM_HD u32x4 gptq_lds16(const uint32_t* p) {
    u32x4 v;
    memcpy(&v, __builtin_assume_aligned(p, 16), 16);
    return v;
}

// ---- gptq_quant ----
struct GptqQuantParams {
    const void* x; int dtype;   // [R][C]
    size_t R, C;                // R % 8 == 0, C % g == 0
    int g;                      // 32, 64 or 128
    uint32_t* qweight;          // [C / 8][R]
    uint32_t* qzeros;           // [C / g][R / 8]
    uint16_t* scales;           // [C / g][R] fp16 codes
    uint32_t* g_idx;            // [C]
    unsigned long long* counts; // [GPTQ_COUNTERS], zeroed by the host
    int vec_x, vec_s;           // x / scales are 16-byte aligned
    int chunks;                 // rounds (tiles) per work-group
};
template <int NP> struct GptqQuantState { float x[NP][8]; };

template <int NP, class Ex>
SM_HD void gptq_quant_body(Ex& ex, const GptqQuantParams& p) {
    typedef GptqQuantState<NP> St;
    constexpr int OPR = 4 * NP, RPP = GPTQ_THREADS / OPR, S = GPTQ_ROWS + GPTQ_ROWS / OPR;
    typename Ex::template State<St> st;
    ex.init(st);
    float* pmn = ex.lds() + LDS_SCRATCH_FLOATS;                     // [OPR][S]: the octets' minima
    float* pmx = pmn + GPTQ_PLANE;                                  // [OPR][S]: their maxima (a NaN: the octet is not finite)
    uint32_t* tile = (uint32_t*)(pmx + GPTQ_PLANE);                 // [OPR][S]: the transposed words
    float* sf = (float*)(tile + GPTQ_PLANE);                        // [64]: s16
    uint32_t* zz = (uint32_t*)(sf + 64);                            // [64]: z
    uint16_t* sh = (uint16_t*)(zz + 64);                            // [64]: the fp16 codes of s16
    uint32_t* cnt = (uint32_t*)(sh + 64);                           // [GPTQ_COUNTERS]
    const size_t NG = p.C / (size_t)p.g, RT = (p.R + GPTQ_ROWS - 1) / GPTQ_ROWS, ntiles = NG * RT;
    ex.each(st, [&](int tid, St&) {
        if (tid < GPTQ_COUNTERS) cnt[tid] = 0u;                     // (first added to behind barrier 1)
    });
    for (int q = 0; q < p.chunks; ++q) {
        const size_t u = (size_t)ex.bid() * p.chunks + q;
        if (u >= ntiles) break;                                     // (the same for every lane of the work-group)
        const bool last = q == p.chunks - 1 || u + 1 >= ntiles;
        const size_t G = u % NG, o0 = (u / NG) * GPTQ_ROWS;
        // A: the loads, the octets' extremes
        ex.each(st, [&](int tid, St& s) {
            const int j = tid % OPR;
#pragma unroll
            for (int k = 0; k < NP; ++k) {
                const int row = k * RPP + tid / OPR;
                if (o0 + row >= p.R) continue;
                float* v = s.x[k];
                gptq_load8(p.x, p.dtype, (o0 + row) * p.C + G * p.g + 8 * (size_t)j, p.vec_x, v);
                float mn = v[0], mx = v[0];
                uint32_t am = 0u;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    mn = v[e] < mn ? v[e] : mn;
                    mx = v[e] > mx ? v[e] : mx;
                    am = umax(am, f2u(v[e]) & 0x7fffffffu);
                }
                pmn[j * S + row] = mn;
                pmx[j * S + row] = am >= 0x7f800000u ? u2f(0x7fc00000u) : mx;
            }
        });
        ex.sync();
        // B: a lane per row: the group's extremes, s16 and z
        ex.each(st, [&](int tid, St&) {
            if (tid >= GPTQ_ROWS || o0 + tid >= p.R) return;
            float mn = 0.0f, mx = 0.0f;
            uint32_t bad = 0u;
#pragma unroll
            for (int j = 0; j < OPR; ++j) {
                const float a = pmn[j * S + tid], b = pmx[j * S + tid];
                mn = a < mn ? a : mn;
                mx = b > mx ? b : mx;
                bad |= (f2u(b) & 0x7fffffffu) >= 0x7f800000u ? 1u : 0u;
            }
            uint32_t moved;
            const uint32_t h = gptq_scale_code(mn, mx, &moved);
            const float s16 = f16_to_f(h);
            sf[tid] = s16;
            sh[tid] = (uint16_t)h;
            zz[tid] = gptq_zero_of(mn, s16);
            const bool zero = mn == 0.0f && mx == 0.0f;
            if (bad) ex.lds_atomic_add(&cnt[GPTQ_NONFINITE], 1u);   // (the call fails: the outputs are unspecified)
            else if (zero) ex.lds_atomic_add(&cnt[GPTQ_ZERO_GROUPS], 1u);
            else if (moved) ex.lds_atomic_add(&cnt[GPTQ_SCALE_CLAMPED], 1u);
        });
        ex.sync();
        // C: the codes, eight to a word, into the transposed tile
        ex.each(st, [&](int tid, St& s) {
            const int j = tid % OPR;
            uint32_t clip = 0u;
#pragma unroll
            for (int k = 0; k < NP; ++k) {
                const int row = k * RPP + tid / OPR;
                if (o0 + row >= p.R) continue;
                const float s16 = sf[row], z = (float)(int)zz[row];
                uint32_t word = 0u;
#pragma unroll
                for (int e = 0; e < 8; ++e) word |= gptq_code_of(s.x[k][e], s16, z, &clip) << (4 * e);
                tile[j * S + row] = word;
            }
            if (clip) ex.lds_atomic_add(&cnt[GPTQ_CLIPPED], clip);
        });
        ex.sync();
        // D: everything leaves along o
        ex.each(st, [&](int tid, St&) {
            const int r = tid & 63;
            if (o0 + r < p.R) {
#pragma unroll
                for (int k = 0; k < NP; ++k) {
                    const int j = (tid >> 6) + 4 * k;
                    p.qweight[(G * OPR + j) * p.R + o0 + r] = tile[j * S + r];
                }
            }
            const int w = tid - 128;                                // wave 2: eight lanes, eight rows each
            if (w >= 0 && w < 8 && o0 + 8 * w < p.R) {
                uint32_t word = 0u;
#pragma unroll
                for (int e = 0; e < 8; ++e) word |= ((zz[8 * w + e] - 1u) & 15u) << (4 * e);
                p.qzeros[G * (p.R / 8) + o0 / 8 + w] = word;
                const size_t at = G * p.R + o0 + 8 * (size_t)w;
                if (p.vec_s) {
                    ((u32x4*)p.scales)[at / 8] = gptq_lds16((const uint32_t*)sh + 4 * w);
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) p.scales[at + e] = sh[8 * w + e];
                }
            }
            if (o0 == 0 && tid >= 192)                              // wave 3 of the first row tile: the group's g_idx
                for (int c = tid - 192; c < p.g; c += 64) p.g_idx[G * p.g + c] = (uint32_t)G;
            if (last && tid >= 64 && tid < 64 + GPTQ_COUNTERS) {    // wave 1: one global atomic per counter and work-group
                const uint32_t v = cnt[tid - 64];
                if (v) ex.global_atomic_add(&p.counts[tid - 64], (unsigned long long)v);
            }
        });
    }
}

template <class Ex>
SM_HD void k_gptq_quant(Ex& ex, const GptqQuantParams& p) {
    if (p.g == 128) gptq_quant_body<4>(ex, p);
    else if (p.g == 64) gptq_quant_body<2>(ex, p);
    else gptq_quant_body<1>(ex, p);
}

// ---- gptq_dequant ----
struct GptqDequantParams {
    const uint32_t* qweight;    // [C / 8][R]
    const uint32_t* qzeros;     // [C / g][R / 8]
    const uint16_t* scales;     // [C / g][R] fp16 codes
    const uint32_t* g_idx;      // [C]
    size_t R, C;
    int g;
    void* out; int out_dtype;   // [R][C]
    int vec;                    // out is 16-byte aligned
    int chunks;                 // rounds (tiles) per work-group
    uint32_t* flags;            // [0]: GPTQ_FLAG_*
};

template <int NP, class Ex>
SM_HD void gptq_dequant_body(Ex& ex, const GptqDequantParams& p) {
    constexpr int OPR = 4 * NP, RPP = GPTQ_THREADS / OPR, S = GPTQ_ROWS + GPTQ_ROWS / OPR;
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const size_t NG = p.C / (size_t)p.g, RT = (p.R + GPTQ_ROWS - 1) / GPTQ_ROWS, ntiles = NG * RT;
    for (int q = 0; q < p.chunks; ++q) {
        const size_t u = (size_t)ex.bid() * p.chunks + q;
        if (u >= ntiles) break;                                     // (the same for every lane of the work-group)
        const size_t G = u % NG, o0 = (u / NG) * GPTQ_ROWS;
        uint32_t* tile = (uint32_t*)(ex.lds() + LDS_SCRATCH_FLOATS) + (q & 1) * GPTQ_DEQUANT_SET;   // the sets alternate
        float* sf = (float*)(tile + GPTQ_PLANE);
        uint32_t* zz = (uint32_t*)(sf + 64);
        ex.each(st, [&](int tid, EmptyState&) {
            const int r = tid & 63, wave = tid >> 6;
            uint32_t flag = 0u;
            if (o0 + r < p.R) {
#pragma unroll
                for (int k = 0; k < NP; ++k) {
                    const int j = wave + 4 * k;
                    tile[j * S + r] = p.qweight[(G * OPR + j) * p.R + o0 + r];
                }
                if (wave == 1) {
                    const uint32_t h = p.scales[G * p.R + o0 + r];
                    if ((h & 0x7c00u) == 0x7c00u) flag |= GPTQ_FLAG_NONFINITE_SCALE;
                    sf[r] = f16_to_f(h);
                }
                if (wave == 2) {
                    const uint32_t word = p.qzeros[G * (p.R / 8) + (o0 + r) / 8];
                    zz[r] = (((word >> (4 * (r & 7))) & 15u) + 1u) & 15u;
                }
            }
            if (wave == 3 && o0 == 0)
                for (int c = r; c < p.g; c += 64)
                    if (p.g_idx[G * p.g + c] != (uint32_t)G) flag |= GPTQ_FLAG_ACT_ORDER;
            if (flag) ex.global_atomic_or_u32(p.flags, flag);
        });
        ex.sync();
        ex.each(st, [&](int tid, EmptyState&) {
            const int j = tid % OPR;
#pragma unroll
            for (int k = 0; k < NP; ++k) {
                const int row = k * RPP + tid / OPR;
                if (o0 + row >= p.R) continue;
                const uint32_t word = tile[j * S + row], z = zz[row];
                const float s16 = sf[row];
                uint32_t w[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) w[e] = gptq_dequant_elem((word >> (4 * e)) & 15u, z, s16, p.out_dtype);
                const size_t i0 = (o0 + row) * p.C + G * p.g + 8 * (size_t)j;
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

template <class Ex>
SM_HD void k_gptq_dequant(Ex& ex, const GptqDequantParams& p) {
    if (p.g == 128) gptq_dequant_body<4>(ex, p);
    else if (p.g == 64) gptq_dequant_body<2>(ex, p);
    else gptq_dequant_body<1>(ex, p);
}

// ---- kernel tags (sm_tag.hpp) and group 28 of smhip_side.hip (smhip_device.hpp) ----
// the quantiser (a tile of 64 rows by one group, three barriers, the transpose through LDS) and the dequantiser (its
// mirror, one barrier a round)
SM_KERNEL_TAG_LB(KGptqQuant, GptqQuantParams, "gptq_quant", k_gptq_quant(ex, p), GPTQ_THREADS, 4)
SM_KERNEL_TAG_LB(KGptqDequant, GptqDequantParams, "gptq_dequant", k_gptq_dequant(ex, p), GPTQ_THREADS, 4)
#define SM_SIDE_KERNELS_28(X) X(KGptqQuant) X(KGptqDequant)

}  // namespace smhip
