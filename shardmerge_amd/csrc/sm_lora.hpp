// sm_lora.hpp - the low-rank update of a LoRA adapter applied to its base weight (smhip_lora_apply):
//
//   out[i][j] = round_dtype(fma(scale, sum_k B[i][k] A[k][j], base[i][j]))
//
// base / out [rows x cols] of the base's dtype, A = lora_a [rank x cols], B = lora_b [rows x rank] of the factors'
// dtype.  The sum is accumulated in fp32 (16-bit factor products are exact in fp32) and rounded once into the dtype.
//
// Two kernels.  k_lora_pack copies the factors into the workspace, both k-contiguous - Bp [rows_pad x rp] = B and
// Ap [cols_pad x rp] = A^T - zero padded to whole output tiles and whole rank chunks (rp = rank rounded up to
// LORA_KSTEP), so that the product kernel reads its fragments as aligned 16-byte loads with no bounds checks and
// any alignment of the caller's factors works.  The factors are ~1 % of the base's bytes.
// k_lora_apply streams the base once: one work-group per 128 x 128 output tile, four waves of 64 x 64, each a 4 x 4
// grid of 16 x 16 MFMA tiles computing D[j][i] = sum_k Ap[j][k] Bp[i][k] - the transposed product, so that a lane's
// four accumulator registers are four consecutive COLUMNS of one output row (C/D map: col = lane & 15 -> row i,
// row = 4 (lane >> 4) + reg -> column j) and the epilogue reads the base and writes the output 4 elements at a time.
// 16-bit factors: v_mfma_f32_16x16x32_{bf16,f16}, one per tile per rank chunk (the products are exact in fp32).
// fp32 factors: a k-ordered fp64 fma chain on the VALU in the same lane layout, bit for bit the emulator's result
// (with an fp32 sum, results that cancel against the base miss the 16-bit dtypes' 1-ulp bar by up to hundreds of
// ulps).  The factor fragments come from L2 (the packed factors
// of a layer are a few MB and every tile row / column of tiles re-reads them).  A 16-bit base on the 4-element path
// is loaded before the product so that its latency hides behind it.
// The CPU work-group emulator runs a scalar body of the same per-element definition (k-ordered fma chain).
//
// Embedding LoRA (lora_embedding_A [rank x rows], lora_embedding_B [cols x rank]) is the same product with the
// factors in transposed roles: k_lora_pack with `trans` packs Bp = A^T and Ap = B^T, and k_lora_apply runs unchanged.
//
// DoRA (smhip_adapter_apply with a magnitude m [rows]):  out[i][j] = round_dtype(v[i][j] * f[i]),
//   v = the value the apply epilogue forms before its rounding (fp32 fma(scale, sum, base) for 16-bit factors, the fp64
//   fma for fp32 factors), f[i] = m[i] / sqrt(sum_j v[i][j]^2), fp64, v * f in fp64 rounded once into the dtype
//   (through fp32 for the 16-bit dtypes).  Three passes after the packing:
//   k_dora_norm   the product of k_lora_apply (same code, same order) and, per (row, column tile), the fp64 sum of v^2
//                 over the tile's columns: lane, then two DPP/shuffle steps over the lane groups, then LDS across the
//                 two column waves - a fixed order, so the partials are bit-reproducible.  Writes [tiles_j x rows].
//   k_dora_scale  one thread per row: the row's partials in tile order -> f[i]; the rows whose factor is not finite
//                 (a zero or non-finite norm, a non-finite magnitude) are counted per work-group with the first of
//                 them, for the host to fail on.  A separate launch: the kernel boundary makes the norm pass's
//                 partials, written from every XCD, visible here.
//   k_dora_apply  the product again (v bit-identical to the norm pass's) and the scaled store; V is recomputed, not
//                 stored (one more read of the base instead of an fp32 round trip of V).
#pragma once
#include <cmath>

#include "sm_common.hpp"
#include "sm_tag.hpp"

namespace smhip {

constexpr int LORA_KSTEP = 32;      // rank chunk: one 16x16x32 MFMA (16-bit factors)
constexpr int LORA_TILE = 128;      // output tile of a work-group (rows and columns); 256 threads
constexpr int LORA_PACK_O = 64;     // pack tile: 64 rows of B / columns of A x LORA_KSTEP ranks
constexpr int LORA_MAX_RANK = 512;

struct LoraPackParams {
    const void* a;                  // lora_a [rank x cols]; trans: lora_embedding_A [rank x rows]
    const void* b;                  // lora_b [rows x rank]; trans: lora_embedding_B [cols x rank]
    void* ap;                       // [cols_pad x rp] = A^T, zero padded
    void* bp;                       // [rows_pad x rp] = B, zero padded
    int rows, cols, rank, rp;
    int esize;                      // factor element bytes: 2 or 4
    int b_tiles;                    // work-groups [0, b_tiles) pack B, the rest A
    int trans;                      // embedding layout: Bp = a^T (a read with rows contiguous), Ap = b^T (ranks contiguous)
};
template <class Ex>
SM_HD void k_lora_pack(Ex& ex, const LoraPackParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const int nkt = p.rp / LORA_KSTEP;
    int bid = ex.bid();
    const bool isb = bid < p.b_tiles;
    if (!isb) bid -= p.b_tiles;
    const int o0 = (bid / nkt) * LORA_PACK_O, k0 = (bid % nkt) * LORA_KSTEP;
    const int nouter = isb ? p.rows : p.cols;
    const bool rk = isb != (p.trans != 0);                 // the source has its ranks contiguous in memory
    const void* src = rk ? p.b : p.a;
    void* dst = isb ? p.bp : p.ap;
    uint32_t* tile = (uint32_t*)ex.lds();                  // [LORA_PACK_O][LORA_KSTEP + 1] raw element bits
    const int nt = ex.nthreads();
    ex.each(st, [&](int tid, EmptyState&) {
        for (int e = tid; e < LORA_PACK_O * LORA_KSTEP; e += nt) {
            int o, k;
            if (rk) { o = e / LORA_KSTEP; k = e % LORA_KSTEP; }      // ranks contiguous in memory
            else { k = e / LORA_PACK_O; o = e % LORA_PACK_O; }      // rows / columns contiguous in memory
            const int go = o0 + o, gk = k0 + k;
            uint32_t v = 0;
            if (go < nouter && gk < p.rank) {
                const size_t idx = rk ? (size_t)go * p.rank + gk : (size_t)gk * nouter + go;
                v = p.esize == 4 ? ((const uint32_t*)src)[idx] : (uint32_t)((const uint16_t*)src)[idx];
            }
            tile[o * (LORA_KSTEP + 1) + k] = v;
        }
    });
    ex.sync();
    ex.each(st, [&](int tid, EmptyState&) {
        for (int e = tid; e < LORA_PACK_O * LORA_KSTEP; e += nt) {
            const int o = e / LORA_KSTEP, k = e % LORA_KSTEP;
            const uint32_t v = tile[o * (LORA_KSTEP + 1) + k];
            const size_t idx = (size_t)(o0 + o) * p.rp + k0 + k;
            if (p.esize == 4) ((uint32_t*)dst)[idx] = v;
            else ((uint16_t*)dst)[idx] = (uint16_t)v;
        }
    });
}

struct LoraApplyParams {
    const void* base;
    void* out;
    int dtype;                      // of base / out
    const void* ap;                 // packed factors (k_lora_pack)
    const void* bp;
    int rows, cols, rp;
    int tiles_j;                    // column tiles: ceil(cols / LORA_TILE)
    float scale;
    int vec;                        // cols % 4 == 0 and base / out aligned to 4 elements: 4-element loads and stores
    double* part;                   // k_dora_norm: the row partials [tiles_j x rows]
    const double* fac;              // k_dora_apply: the row factors f [rows]
};

SM_HD void lora_put(void* out, int dtype, size_t i, float v) {
    if (dtype == DT_F32) ((float*)out)[i] = v;
    else if (dtype == DT_BF16) ((uint16_t*)out)[i] = f_to_bf16_any(v);
    else ((uint16_t*)out)[i] = f_to_f16_any(v);
}
// 4-element path, 16-bit base: out[i][j .. j+3] from the base's two words w0, w1 (already loaded)
SM_HD void lora_store4_16(const LoraApplyParams& p, size_t off, const float* acc, uint32_t w0, uint32_t w1) {
    const uint32_t h[4] = {w0 & 0xffffu, w0 >> 16, w1 & 0xffffu, w1 >> 16};
    uint32_t r[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float b = p.dtype == DT_BF16 ? bf16_to_f(h[q]) : f16_to_f(h[q]);
        const float v = fmaf(p.scale, acc[q], b);
        r[q] = p.dtype == DT_BF16 ? f_to_bf16_any(v) : f_to_f16_any(v);
    }
    uint32_t* ow = (uint32_t*)((uint16_t*)p.out + off);
    ow[0] = r[0] | (r[1] << 16);
    ow[1] = r[2] | (r[3] << 16);
}
// out[i][j .. j+3] = round(fma(scale, acc[q], base[i][j + q])), the columns past `cols` skipped
SM_HD void lora_store4(const LoraApplyParams& p, int i, int j, const float* acc) {
    if (i >= p.rows || j >= p.cols) return;
    const size_t off = (size_t)i * p.cols + j;
    if (p.vec) {
        if (p.dtype == DT_F32) {
            const cf4 b = *(const cf4*)((const float*)p.base + off);
            cf4 o;
            o.x = fmaf(p.scale, acc[0], b.x); o.y = fmaf(p.scale, acc[1], b.y);
            o.z = fmaf(p.scale, acc[2], b.z); o.w = fmaf(p.scale, acc[3], b.w);
            *(cf4*)((float*)p.out + off) = o;
        } else {
            const uint32_t* bw = (const uint32_t*)((const uint16_t*)p.base + off);
            lora_store4_16(p, off, acc, bw[0], bw[1]);
        }
        return;
    }
    for (int q = 0; q < 4 && j + q < p.cols; ++q)
        lora_put(p.out, p.dtype, off + q, fmaf(p.scale, acc[q], load_elem(p.base, p.dtype, off + q)));
}

// fp32 factors: out[i][j .. j+3] = round(base + scale * acc[q]) evaluated in fp64 (the products and their sum are
// fp64 too: an fp32 sum loses the bits a result that cancels against the base needs for the 16-bit dtypes)
SM_HD void lora_store4d(const LoraApplyParams& p, int i, int j, const double* acc) {
    if (i >= p.rows || j >= p.cols) return;
    const size_t off = (size_t)i * p.cols + j;
    for (int q = 0; q < 4 && j + q < p.cols; ++q)
        lora_put(p.out, p.dtype, off + q, (float)((double)load_elem(p.base, p.dtype, off + q) + (double)p.scale * acc[q]));
}

// ---- DoRA: v of out[i][j .. j+3] (n < 4 of them inside the tensor) and the scaled store ----
// 16-bit factors: v = fma(scale, acc, base) in fp32, as lora_store4 / lora_store4_16 form it; base words w0, w1 when
// the caller loaded them (pre), else read here
SM_HD void dora_v4(const LoraApplyParams& p, size_t off, int n, bool pre, uint32_t w0, uint32_t w1, const float* acc,
                   double* v) {
    float b[4] = {0.f, 0.f, 0.f, 0.f};
    if (pre) {
        const uint32_t h[4] = {w0 & 0xffffu, w0 >> 16, w1 & 0xffffu, w1 >> 16};
        for (int q = 0; q < 4; ++q) b[q] = p.dtype == DT_BF16 ? bf16_to_f(h[q]) : f16_to_f(h[q]);
    } else if (p.vec && n == 4 && p.dtype == DT_F32) {
        const cf4 c = *(const cf4*)((const float*)p.base + off);
        b[0] = c.x; b[1] = c.y; b[2] = c.z; b[3] = c.w;
    } else {
        for (int q = 0; q < 4; ++q) if (q < n) b[q] = load_elem(p.base, p.dtype, off + q);
    }
    for (int q = 0; q < 4; ++q) v[q] = q < n ? (double)fmaf(p.scale, acc[q], b[q]) : 0.0;
}
// fp32 factors: v = fma(scale, acc, base) in fp64
SM_HD void dora_v4d(const LoraApplyParams& p, size_t off, int n, const double* acc, double* v) {
    for (int q = 0; q < 4; ++q) v[q] = q < n ? fma((double)p.scale, acc[q], (double)load_elem(p.base, p.dtype, off + q)) : 0.0;
}
// out[i][j .. j+3] = round(v[q] * f), the first n
SM_HD void dora_store4(const LoraApplyParams& p, size_t off, int n, const double* v, double f) {
    if (p.vec && n == 4) {
        if (p.dtype == DT_F32) {
            cf4 o;
            o.x = (float)(v[0] * f); o.y = (float)(v[1] * f); o.z = (float)(v[2] * f); o.w = (float)(v[3] * f);
            *(cf4*)((float*)p.out + off) = o;
        } else {
            uint32_t r[4];
            for (int q = 0; q < 4; ++q) {
                const float y = (float)(v[q] * f);
                r[q] = p.dtype == DT_BF16 ? f_to_bf16_any(y) : f_to_f16_any(y);
            }
            uint32_t* ow = (uint32_t*)((uint16_t*)p.out + off);
            ow[0] = r[0] | (r[1] << 16);
            ow[1] = r[2] | (r[3] << 16);
        }
        return;
    }
    for (int q = 0; q < 4; ++q) if (q < n) lora_put(p.out, p.dtype, off + q, (float)(v[q] * f));
}

#if defined(__HIP_DEVICE_COMPILE__)
typedef float lora_f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 lora_bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 lora_f16x8 __attribute__((ext_vector_type(8)));
#endif

enum { LORA_PLAIN = 0, DORA_NORM = 1, DORA_APPLY = 2 };

// FT: the factors' dtype (DT_BF16 / DT_F16 / DT_F32); MODE: what the epilogue does with the product (above)
template <int FT, int MODE, class Ex>
SM_HD void k_lora_tile(Ex& ex, const LoraApplyParams& p) {
    const int bid = ex.bid();
    const int i0 = (bid / p.tiles_j) * LORA_TILE, j0 = (bid % p.tiles_j) * LORA_TILE;
#if defined(__HIP_DEVICE_COMPILE__)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wi = i0 + (wave >> 1) * 64, wj = j0 + (wave & 1) * 64;
    const int l16 = lane & 15, g = lane >> 4;
    lora_f32x4 acc[4][4];                                   // [column tile a][row tile b]
    double dacc[FT == DT_F32 ? 4 : 1][4][4];                // fp32 factors: fp64 accumulators instead
#pragma unroll
    for (int a = 0; a < (FT == DT_F32 ? 4 : 1); ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int q = 0; q < 4; ++q) dacc[a][b][q] = 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = lora_f32x4{0.f, 0.f, 0.f, 0.f};
    // lane (l16, g) reads ranks k0 + 8 g .. k0 + 8 g + 7 of row wj + 16 a + l16 of Ap and of row wi + 16 b + l16 of Bp
    // 16-bit base on the 4-element path: the tile's base words are loaded before the product, which hides them
    const bool pre = FT != DT_F32 && p.vec && p.dtype != DT_F32;
    uint32_t braw[4][4][2];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int i = wi + 16 * b + l16, j = wj + 16 * a + 4 * g;
            braw[a][b][0] = braw[a][b][1] = 0;
            if (pre && i < p.rows && j < p.cols) {
                const uint32_t* bw = (const uint32_t*)((const uint16_t*)p.base + (size_t)i * p.cols + j);
                braw[a][b][0] = bw[0];
                braw[a][b][1] = bw[1];
            }
        }
    const size_t es = FT == DT_F32 ? 4 : 2;
    const char* pa = (const char*)p.ap + ((size_t)(wj + l16) * p.rp + 8 * g) * es;
    const char* pb = (const char*)p.bp + ((size_t)(wi + l16) * p.rp + 8 * g) * es;
    const size_t tstride = (size_t)16 * p.rp * es;          // 16 rows of a packed factor
    for (int k0 = 0; k0 < p.rp; k0 += LORA_KSTEP) {
        const size_t koff = (size_t)k0 * es;
        if constexpr (FT == DT_F32) {
            // fp32 factors: a k-ordered fp64 fma chain on the VALU per output element (the emulator's definition,
            // bit for bit); the lane's outputs are rows wi + 16 b + l16 and columns wj + 16 a + 4 g + q
            const float* fb = (const float*)p.bp + (size_t)(wi + l16) * p.rp + k0;
            const float* fa = (const float*)p.ap + (size_t)(wj + 4 * g) * p.rp + k0;
            for (int k4 = 0; k4 < LORA_KSTEP; k4 += 4) {
                cf4 bv[4];
#pragma unroll
                for (int b = 0; b < 4; ++b) bv[b] = *(const cf4*)(fb + (size_t)16 * b * p.rp + k4);
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const cf4 av = *(const cf4*)(fa + (size_t)(16 * a + q) * p.rp + k4);
#pragma unroll
                        for (int b = 0; b < 4; ++b) {
                            double v = dacc[a][b][q];
                            v = fma((double)bv[b].x, (double)av.x, v);
                            v = fma((double)bv[b].y, (double)av.y, v);
                            v = fma((double)bv[b].z, (double)av.z, v);
                            v = fma((double)bv[b].w, (double)av.w, v);
                            dacc[a][b][q] = v;
                        }
                    }
            }
        } else {
            u32x4 af[4], bf[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                af[t] = *(const u32x4*)(pa + t * tstride + koff);
                bf[t] = *(const u32x4*)(pb + t * tstride + koff);
            }
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    if constexpr (FT == DT_BF16)
                        acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(lora_bf16x8, af[a]),
                                                                            __builtin_bit_cast(lora_bf16x8, bf[b]), acc[a][b], 0, 0, 0);
                    else
                        acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(lora_f16x8, af[a]),
                                                                           __builtin_bit_cast(lora_f16x8, bf[b]), acc[a][b], 0, 0, 0);
                }
        }
    }
    if constexpr (MODE == LORA_PLAIN) {
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const float v[4] = {acc[a][b].x, acc[a][b].y, acc[a][b].z, acc[a][b].w};
            const int i = wi + 16 * b + l16, j = wj + 16 * a + 4 * g;
            if constexpr (FT == DT_F32) lora_store4d(p, i, j, dacc[a < (FT == DT_F32 ? 4 : 1) ? a : 0][b]);
            else if (!pre) lora_store4(p, i, j, v);
            else if (i < p.rows && j < p.cols) lora_store4_16(p, (size_t)i * p.cols + j, v, braw[a][b][0], braw[a][b][1]);
        }
    } else {
        // DORA_NORM: per row tile b, the lane's sum of v^2, then the four lane groups g of a row (two shuffles), into
        // LDS [wave][64 rows]; then each even (column) wave adds its odd partner's sums
        double* red = (double*)ex.lds();
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            double rs = 0.0;
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const int i = wi + 16 * b + l16, j = wj + 16 * a + 4 * g;
                const int n = i < p.rows ? (p.cols - j < 0 ? 0 : (p.cols - j > 4 ? 4 : p.cols - j)) : 0;
                const size_t off = (size_t)(i < p.rows ? i : 0) * p.cols + (n ? j : 0);
                double v[4];
                if constexpr (FT == DT_F32) {
                    dora_v4d(p, off, n, dacc[a < (FT == DT_F32 ? 4 : 1) ? a : 0][b], v);
                } else {
                    const float f4[4] = {acc[a][b].x, acc[a][b].y, acc[a][b].z, acc[a][b].w};
                    dora_v4(p, off, n, pre && n == 4, braw[a][b][0], braw[a][b][1], f4, v);
                }
                if constexpr (MODE == DORA_NORM) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) rs = fma(v[q], v[q], rs);         // (v = 0 past the tensor)
                } else if (n) {
                    dora_store4(p, off, n, v, p.fac[i]);
                }
            }
            if constexpr (MODE == DORA_NORM) {
                rs += __shfl_xor(rs, 16, 64);
                rs += __shfl_xor(rs, 32, 64);
                if (g == 0) red[wave * 64 + 16 * b + l16] = rs;
            }
        }
        if constexpr (MODE == DORA_NORM) {
            __syncthreads();
            if (!(wave & 1) && g == 0) {
                const int tj = bid % p.tiles_j;
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int r = 16 * b + l16, i = wi + r;
                    if (i < p.rows) p.part[(size_t)tj * p.rows + i] = red[wave * 64 + r] + red[(wave + 1) * 64 + r];
                }
            }
        }
    }
#else
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const int nt = ex.nthreads();
    auto ld = [&](const void* q, size_t idx) {
        if (FT == DT_F32) return ((const float*)q)[idx];
        const uint32_t h = ((const uint16_t*)q)[idx];
        return FT == DT_BF16 ? bf16_to_f(h) : f16_to_f(h);
    };
    if constexpr (MODE != LORA_PLAIN) {
        // DoRA: per element the same k-ordered chain and v as the LoRA body; DORA_NORM sums v^2 along each row
        auto v4 = [&](int i, int j, int n, double* v) {
            const size_t off = (size_t)i * p.cols + j;
            if (FT == DT_F32) {
                double acc[4];
                for (int q = 0; q < 4; ++q) {
                    acc[q] = 0.0;
                    if (q < n)
                        for (int k = 0; k < p.rp; ++k)
                            acc[q] = fma((double)ld(p.bp, (size_t)i * p.rp + k), (double)ld(p.ap, (size_t)(j + q) * p.rp + k), acc[q]);
                }
                dora_v4d(p, off, n, acc, v);
            } else {
                float acc[4];
                for (int q = 0; q < 4; ++q) {
                    acc[q] = 0.f;
                    if (q < n)
                        for (int k = 0; k < p.rp; ++k)
                            acc[q] = fmaf(ld(p.bp, (size_t)i * p.rp + k), ld(p.ap, (size_t)(j + q) * p.rp + k), acc[q]);
                }
                dora_v4(p, off, n, false, 0u, 0u, acc, v);
            }
        };
        ex.each(st, [&](int tid, EmptyState&) {
            for (int r = tid; r < LORA_TILE; r += nt) {
                const int i = i0 + r;
                if (i >= p.rows) continue;
                double rs = 0.0;
                for (int j = j0; j < j0 + LORA_TILE && j < p.cols; j += 4) {
                    const int n = p.cols - j > 4 ? 4 : p.cols - j;
                    double v[4];
                    v4(i, j, n, v);
                    if (MODE == DORA_NORM) for (int q = 0; q < n; ++q) rs = fma(v[q], v[q], rs);
                    else dora_store4(p, (size_t)i * p.cols + j, n, v, p.fac[i]);
                }
                if (MODE == DORA_NORM) p.part[(size_t)(bid % p.tiles_j) * p.rows + i] = rs;
            }
        });
        return;
    }
    ex.each(st, [&](int tid, EmptyState&) {
        for (int e = tid; e < LORA_TILE * LORA_TILE / 4; e += nt) {
            const int i = i0 + e / (LORA_TILE / 4), j = j0 + 4 * (e % (LORA_TILE / 4));
            if (i >= p.rows || j >= p.cols) continue;
            if (FT == DT_F32) {
                double acc[4];
                for (int q = 0; q < 4; ++q) {
                    acc[q] = 0.0;
                    for (int k = 0; k < p.rp; ++k)
                        acc[q] = fma((double)ld(p.bp, (size_t)i * p.rp + k), (double)ld(p.ap, (size_t)(j + q) * p.rp + k), acc[q]);
                }
                lora_store4d(p, i, j, acc);
                continue;
            }
            float acc[4];
            for (int q = 0; q < 4; ++q) {
                acc[q] = 0.f;
                for (int k = 0; k < p.rp; ++k)
                    acc[q] = fmaf(ld(p.bp, (size_t)i * p.rp + k), ld(p.ap, (size_t)(j + q) * p.rp + k), acc[q]);
            }
            lora_store4(p, i, j, acc);
        }
    });
#endif
}

template <int FT, class Ex>
SM_HD void k_lora_apply(Ex& ex, const LoraApplyParams& p) { k_lora_tile<FT, LORA_PLAIN>(ex, p); }
template <int FT, class Ex>
SM_HD void k_dora_norm(Ex& ex, const LoraApplyParams& p) { k_lora_tile<FT, DORA_NORM>(ex, p); }
template <int FT, class Ex>
SM_HD void k_dora_apply(Ex& ex, const LoraApplyParams& p) { k_lora_tile<FT, DORA_APPLY>(ex, p); }

// ---- DoRA row factors: f[i] = m[i] / sqrt(sum_t part[t][i]), the partials summed in tile order (fp64) ----
constexpr int DORA_SCALE_THREADS = 64;      // one wave per work-group: 128 of them for 8192 rows
struct DoraScaleParams {
    const double* part;             // [tiles_j x rows] (k_dora_norm)
    const void* mag;                // the magnitude m [rows]
    int mdtype;
    double* fac;                    // f [rows]
    uint32_t* bad;                  // [grid][2]: the work-group's rows whose f is not finite, the first of them
    int rows, tiles_j;
};
template <class Ex>
SM_HD void k_dora_scale(Ex& ex, const DoraScaleParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    uint32_t* flag = (uint32_t*)ex.lds();                   // [DORA_SCALE_THREADS]: the row, or ~0u when it is fine
    const int r0 = ex.bid() * DORA_SCALE_THREADS;
    ex.each(st, [&](int tid, EmptyState&) {
        const int i = r0 + tid;
        uint32_t bad = ~0u;
        if (i < p.rows) {
            double sum = 0.0;
#pragma unroll 8
            for (int t = 0; t < p.tiles_j; ++t) sum += p.part[(size_t)t * p.rows + i];     // (8 loads in flight)
            const double m = (double)load_elem(p.mag, p.mdtype, i);
            const double f = m / sqrt(sum);
            // a zero, NaN or infinite norm, a NaN or infinite magnitude
            if (!(sum > 0.0 && sum <= 1.7976931348623157e308) || !(f - f == 0.0)) bad = (uint32_t)i;
            p.fac[i] = f;
        }
        flag[tid] = bad;
    });
    ex.sync();
    ex.each(st, [&](int tid, EmptyState&) {
        if (tid != 0) return;
        uint32_t n = 0, first = ~0u;
        for (int t = 0; t < DORA_SCALE_THREADS; ++t) {
            const uint32_t r = flag[t];
            n += r != ~0u;
            first = r < first ? r : first;
        }
        p.bad[2 * ex.bid()] = n;
        p.bad[2 * ex.bid() + 1] = first;
    });
}

// ---- kernel tags (sm_tag.hpp) and this header's share of group 2 of smhip_side.hip (smhip_device.hpp) ----
// LoRA low-rank update: the factor packing and the MFMA product, one per factor dtype
SM_KERNEL_TAG_LB(KLoraPack, LoraPackParams, "lora_pack", k_lora_pack(ex, p), 256, 4)
SM_KERNEL_TAG_LB(KLoraBf16, LoraApplyParams, "lora_apply", k_lora_apply<DT_BF16>(ex, p), 256, 2)
SM_KERNEL_TAG_LB(KLoraF16, LoraApplyParams, "lora_apply", k_lora_apply<DT_F16>(ex, p), 256, 2)
SM_KERNEL_TAG_LB(KLoraF32, LoraApplyParams, "lora_apply", k_lora_apply<DT_F32>(ex, p), 256, 2)
// DoRA: the row-norm pass, the row factors and the scaled apply pass
SM_KERNEL_TAG_LB(KDoraNormBf16, LoraApplyParams, "dora_norm", k_dora_norm<DT_BF16>(ex, p), 256, 2)
SM_KERNEL_TAG_LB(KDoraNormF16, LoraApplyParams, "dora_norm", k_dora_norm<DT_F16>(ex, p), 256, 2)
SM_KERNEL_TAG_LB(KDoraNormF32, LoraApplyParams, "dora_norm", k_dora_norm<DT_F32>(ex, p), 256, 2)
SM_KERNEL_TAG_LB(KDoraScale, DoraScaleParams, "dora_scale", k_dora_scale(ex, p), DORA_SCALE_THREADS, 4)
SM_KERNEL_TAG_LB(KDoraApplyBf16, LoraApplyParams, "dora_apply", k_dora_apply<DT_BF16>(ex, p), 256, 2)
SM_KERNEL_TAG_LB(KDoraApplyF16, LoraApplyParams, "dora_apply", k_dora_apply<DT_F16>(ex, p), 256, 2)
SM_KERNEL_TAG_LB(KDoraApplyF32, LoraApplyParams, "dora_apply", k_dora_apply<DT_F32>(ex, p), 256, 2)
#define SM_KERNELS_LORA(X) X(KLoraPack) X(KLoraBf16) X(KLoraF16) X(KLoraF32) \
    X(KDoraNormBf16) X(KDoraNormF16) X(KDoraNormF32) X(KDoraScale) X(KDoraApplyBf16) X(KDoraApplyF16) X(KDoraApplyF32)

}  // namespace smhip
