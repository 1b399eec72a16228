// sm_geo.hpp - the geometric merge operators (Model Stock, Jang et al. 2024; SLERP and NuSLERP), operators the
// reference does not have: their coefficients come from the norms of the task vectors and the angles between them.
// The function is stated in include/shardmerge_hip.h (smhip_geo_merge).  What the operators share is the Gram matrix
// G[i][j] = sum_e x_i[e] x_j[e] of the k vectors in fp64, with a summation order that is a function of the element
// count alone - fixed segments, a fixed stride inside a segment, a fixed binary tree, segments added in index order -
// so G, the coefficients and the output are defined bit for bit and do not depend on the grid or the device.
//
//   geo_gram       one streaming pass: per octet the base (once when shared) and the finetunes of one TILE of pairs
//                  (GEO_TILE x GEO_TILE models; k <= 4 is one tile, larger k re-reads), the deltas in registers, one
//                  fp64 accumulator per pair and thread (a product of two fp32 values is exact in fp64), the 256
//                  partials of a work-group reduced by a binary tree in LDS.  One work-group per segment (whole tensor)
//                  or per row (row-wise); the tile index is part of the grid: ONE launch.
//   geo_gram_fold  whole tensor: the segments' results added in index order, a thread per pair.
//   geo_coef       row-wise Model Stock: a thread per row turns its Gram into t and the k coefficients.
//   geo_combine    one streaming pass: out = base_out + sum_i c_i x_i (delta space) or sum_i c_i x_i (weight space),
//                  the coefficients from the kernel arguments or from the [R][k] array of geo_coef.
#pragma once
#include "sm_delta.hpp"

namespace smhip {

constexpr int GEO_THREADS = 256;                  // work-group of geo_gram: the tree below needs a power of two
constexpr size_t GEO_SEG_ELEMS = 32768;           // whole tensor: elements per segment (16 octets per thread)
constexpr int GEO_TILE = 4;                       // models per side of a tile of pairs
enum { GEO_MODEL_STOCK = 0, GEO_NUSLERP = 1, GEO_SLERP = 2 };

// ONE correctly rounded fp64 operation each (the device compiler contracts a * b + c into an fma otherwise)
SM_HD double geo_dmul(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
    double r = a * b; asm volatile("" : "+v"(r)); return r;
#else
    volatile double r = a * b; return r;
#endif
}
SM_HD double geo_dadd(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
    double r = a + b; asm volatile("" : "+v"(r)); return r;
#else
    volatile double r = a + b; return r;
#endif
}
SM_HD double geo_ddiv(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __ddiv_rn(a, b);
#else
    volatile double r = a / b; return r;
#endif
}
SM_HD double geo_dsqrt(double a) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __dsqrt_rn(a);
#else
    return std::sqrt(a);
#endif
}
SM_HD bool geo_finite(double v) { return v - v == 0.0; }

// position of G[i][j], i <= j, in the packed upper triangle of a k x k matrix (row after row)
SM_HD int geo_pair_index(int i, int j, int k) { return i * k - i * (i - 1) / 2 + (j - i); }
SM_HD int geo_pairs(int k) { return k * (k + 1) / 2; }
// tiles of pairs: blocks of GEO_TILE models, block pairs (A, B) with A <= B, row after row
SM_HD int geo_blocks(int k) { return (k + GEO_TILE - 1) / GEO_TILE; }
SM_HD int geo_tiles(int k) { return geo_pairs(geo_blocks(k)); }

// cos_ij of the definition: clamp(G_ij / (n_i n_j), -1, 1), 0 when the product of the norms is 0 or not finite
SM_HD double geo_cos(double gij, double ni, double nj) {
    const double p = geo_dmul(ni, nj);
    if (p == 0.0 || !geo_finite(p)) return 0.0;
    const double c = geo_ddiv(gij, p);
    return c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);
}
// Model Stock's t from the packed Gram g[geo_pairs(k)]; *cos_out: the mean cosine
SM_HD double geo_stock_t(const double* g, int k, double* cos_out) {
    if (k == 1) { if (cos_out) *cos_out = 0.0; return 1.0; }
    double sum = 0.0;
    for (int i = 0; i < k; ++i) {
        const double ni = geo_dsqrt(g[geo_pair_index(i, i, k)]);
        for (int j = i + 1; j < k; ++j)
            sum = geo_dadd(sum, geo_cos(g[geo_pair_index(i, j, k)], ni, geo_dsqrt(g[geo_pair_index(j, j, k)])));
    }
    const double c = geo_ddiv(sum, (double)(k * (k - 1) / 2));
    if (cos_out) *cos_out = c;
    const double den = geo_dadd(1.0, geo_dmul((double)(k - 1), c));
    if (!(den > 0.0)) return 0.0;
    const double t = geo_ddiv(geo_dmul((double)k, c), den);
    return geo_finite(t) ? t : 0.0;
}
// c_i = fp32((t * alpha_i) / A)
SM_HD float geo_stock_coef(double t, double alpha, double A) { return (float)geo_ddiv(geo_dmul(t, alpha), A); }

struct GeoGramParams {
    TiesInputs in;
    int weight_space;           // 1: x_i = finetune_i (the bases are not read), 0: x_i = finetune_i - base_i
    size_t seg_len;             // elements per segment: GEO_SEG_ELEMS (whole tensor) or C (row-wise)
    size_t nseg;                // segments: ceil(n / seg_len)
    int seg_vec;                // every segment starts at an octet boundary and the pointers are 16-byte aligned
    double* part;               // [nseg][geo_pairs(k)]: the Gram of each segment
    uint32_t* flags;            // [0]: bit i = x_i holds a NaN or an Inf
};
SM_HD size_t geo_gram_lds_floats() { return LDS_SCRATCH_FLOATS + (size_t)2 * GEO_TILE * GEO_TILE * GEO_THREADS; }

// TILED = false: k <= GEO_TILE, the one (diagonal) tile - the tuned case, half the registers; true: any k
template <bool TILED, class Ex>
SM_HD void k_geo_gram(Ex& ex, const GeoGramParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const int nt = ex.nthreads();                                  // GEO_THREADS
    const int k = p.in.k;
    const int ntiles = TILED ? geo_tiles(k) : 1;
    const size_t seg = (size_t)ex.bid() / ntiles;
    int tile = ex.bid() % ntiles, A = 0;
    for (int rowlen = geo_blocks(k); tile >= rowlen; tile -= rowlen, --rowlen) ++A;
    const int B = A + tile;
    const bool diag = !TILED || A == B;
    const int a0 = A * GEO_TILE, b0 = B * GEO_TILE;
    const int na = k - a0 < GEO_TILE ? k - a0 : GEO_TILE, nb = k - b0 < GEO_TILE ? k - b0 : GEO_TILE;
    double* red = (double*)(ex.lds() + LDS_SCRATCH_FLOATS);        // [GEO_TILE * GEO_TILE][nt] (LDS_SCRATCH_FLOATS is even)
    const size_t start = seg * p.seg_len;
    const size_t len = p.in.n - start < p.seg_len ? p.in.n - start : p.seg_len;
    ex.each(st, [&](int tid, EmptyState&) {
        double acc[GEO_TILE][GEO_TILE];
#pragma unroll
        for (int ia = 0; ia < GEO_TILE; ++ia)
#pragma unroll
            for (int jb = 0; jb < GEO_TILE; ++jb) acc[ia][jb] = 0.0;
        uint32_t bad = 0;
        for (size_t q = tid; q < segment_octets(len); q += nt) {
            const Octet o = segment_octet(start, len, p.seg_vec, q);
            float b[8], xa[GEO_TILE][8], xb[TILED ? GEO_TILE : 1][8];
            if (!p.weight_space) delta_base8(p.in, o, b);
            // the vectors of one side of the tile: 8 elements each (elements past the segment's end load as +0)
            auto load_side = [&](int m0, int nm, float (*x)[8]) {
#pragma unroll
                for (int m = 0; m < GEO_TILE; ++m) {
                    if (m < nm) {
                        const int i = m0 + m;
                        if (p.weight_space) ties_load8(p.in.ft[i], p.in.dtype, o.i0, o.cnt, o.vec, x[m]);
                        else delta_load8(p.in, i, o, b, x[m]);
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            if (!p.weight_space) x[m][e] = x[m][e] - b[e];
                            if (delta_key(x[m][e]) >= TIES_KEY_INF) bad |= 1u << i;
                        }
                    }
                }
            };
            load_side(a0, na, xa);
            if constexpr (TILED) { if (!diag) load_side(b0, nb, xb); }
#pragma unroll
            for (int e = 0; e < 8; ++e) {
#pragma unroll
                for (int ia = 0; ia < GEO_TILE; ++ia) {
#pragma unroll
                    for (int jb = 0; jb < GEO_TILE; ++jb) {
                        // (the product of two fp32 values is exact in fp64: fused or not, this is ONE rounded addition)
                        if (ia < na && jb < nb && (!diag || ia <= jb)) {
                            float y = xa[jb][e];
                            if constexpr (TILED) { if (!diag) y = xb[jb][e]; }
                            acc[ia][jb] = acc[ia][jb] + (double)xa[ia][e] * (double)y;
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int ia = 0; ia < GEO_TILE; ++ia)
#pragma unroll
            for (int jb = 0; jb < GEO_TILE; ++jb)
                if (ia < na && jb < nb && (!diag || ia <= jb)) red[(ia * GEO_TILE + jb) * nt + tid] = acc[ia][jb];
        if (bad) ex.global_atomic_or_u32(p.flags, bad);
    });
    ex.sync();
    // the fixed binary tree: p[t] = p[t] + p[t + s] for t < s, s = nt / 2, nt / 4, ..., 1
    for (int s = nt >> 1; s > 0; s >>= 1) {
        ex.each(st, [&](int tid, EmptyState&) {
            if (tid >= s) return;
            for (int ia = 0; ia < na; ++ia)
                for (int jb = diag ? ia : 0; jb < nb; ++jb) {
                    double* v = red + (ia * GEO_TILE + jb) * nt;
                    v[tid] = v[tid] + v[tid + s];
                }
        });
        ex.sync();
    }
    ex.each(st, [&](int tid, EmptyState&) {
        const int ia = tid / GEO_TILE, jb = tid % GEO_TILE;
        if (tid < GEO_TILE * GEO_TILE && ia < na && jb < nb && (!diag || ia <= jb))
            p.part[seg * geo_pairs(k) + geo_pair_index(a0 + ia, b0 + jb, k)] = red[tid * nt];
    });
}

// The ordered fp64 fold over the segments, one work-group of at least np threads: the Gram's (geo_gram_fold), and under
// their own tags SCE's energies (sce_energy_fold, sm_sce.hpp) and the statistics' (stats_fold, sm_stats.hpp).
struct GeoFoldParams {
    int np;                     // values per segment: geo_pairs(k)
    int row, pitch;             // value t lands at out[(t / row) * pitch + t % row]; row = pitch = np: at out[t]
    size_t nseg;
    const double* part;         // [nseg][np]
    double* out;                // out = (((0 + part[0]) + part[1]) + ...)
};
template <class Ex>
SM_HD void k_geo_fold(Ex& ex, const GeoFoldParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    ex.each(st, [&](int tid, EmptyState&) {
        if (tid >= p.np) return;
        double s = 0.0;
        for (size_t q = 0; q < p.nseg; ++q) s = geo_dadd(s, p.part[q * p.np + tid]);
        p.out[(tid / p.row) * p.pitch + tid % p.row] = s;
    });
}

struct GeoCoefParams {
    int k;
    size_t rows;
    double alpha[TIES_MAX_MODELS];
    double A;                   // the sum of the alphas in order, 1 where |A| < 1e-8
    const double* G;            // [rows][geo_pairs(k)]
    float* coef;                // [rows][k]
    double* t;                  // [rows]
};
template <class Ex>
SM_HD void k_geo_coef(Ex& ex, const GeoCoefParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    ex.each(st, [&](int tid, EmptyState&) {
        const size_t r = (size_t)ex.bid() * ex.nthreads() + tid;
        if (r >= p.rows) return;
        const double t = geo_stock_t(p.G + r * geo_pairs(p.k), p.k, nullptr);
        p.t[r] = t;
        for (int i = 0; i < p.k; ++i) p.coef[r * p.k + i] = geo_stock_coef(t, p.alpha[i], p.A);
    });
}

struct GeoCombineParams {
    TiesInputs in;
    int weight_space;
    float c[TIES_MAX_MODELS];   // whole tensor: the coefficients
    const float* rowcoef;       // row-wise: [R][k], else null
    size_t C;                   // row length (row-wise)
    const void* base_out; int base_out_dtype;
    int out_is_base0;           // base_out is base[0] in the same dtype and the bases are shared: loaded once
    void* out;                  // base_out_dtype, [n]
    float* delta_out;           // optional fp32 [n]: M
    int chunks;                 // octets per thread
};
template <class Ex>
SM_HD void k_geo_combine(Ex& ex, const GeoCombineParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const int k = p.in.k;
    ex.each(st, [&](int tid, EmptyState&) {
        for (int q = 0; q < p.chunks; ++q) {
            Octet o;
            if (!octet_at(p.in, ex.bid(), ex.nthreads(), p.chunks, tid, q, o)) break;
            float b[8], bo[8], M[8];
            if (!p.weight_space) {
                delta_base8(p.in, o, b);
                delta_base_out8(p, o, b, bo);
            }
            // row-wise: the row of element i0, and whether the whole octet lies in it (always when C % 8 == 0)
            size_t row = 0;
            bool one_row = true;
            if (p.rowcoef) {
                row = o.i0 / p.C;
                one_row = o.i0 - row * p.C + 8 <= p.C;
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) M[e] = 0.f;
            for (int i = 0; i < k; ++i) {
                float f[8];
                if (p.weight_space) ties_load8(p.in.ft[i], p.in.dtype, o.i0, o.cnt, o.vec, f);
                else delta_load8(p.in, i, o, b, f);
                const float ci = p.rowcoef ? p.rowcoef[row * k + i] : p.c[i];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float x = p.weight_space ? f[e] : f[e] - b[e];
                    float ce = ci;
                    if (!one_row && e < o.cnt) ce = p.rowcoef[((o.i0 + e) / p.C) * k + i];
                    M[e] = aten_fadd_(M[e], aten_fmul_(ce, x));
                }
            }
            float r[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) r[e] = p.weight_space ? M[e] : aten_fadd_(bo[e], M[e]);
            delta_store8(p, o, r, M);
        }
    });
}

// ---- kernel tags (sm_tag.hpp) and this header's share of group 7 of smhip_side.hip (smhip_device.hpp) ----
// the ordered fp64 Gram pass, its fold over the segments, the row-wise coefficients, the combine pass
SM_KERNEL_TAG_LB(KGeoGram, GeoGramParams, "geo_gram", k_geo_gram<false>(ex, p), GEO_THREADS, 4)       // k <= 4: one tile of pairs
SM_KERNEL_TAG_LB(KGeoGramTiled, GeoGramParams, "geo_gram", k_geo_gram<true>(ex, p), GEO_THREADS, 2)
SM_KERNEL_TAG_LB(KGeoFold, GeoFoldParams, "geo_gram_fold", k_geo_fold(ex, p), 256, 4)
SM_KERNEL_TAG_LB(KGeoCoef, GeoCoefParams, "geo_coef", k_geo_coef(ex, p), 256, 4)
SM_KERNEL_TAG_LB(KGeoCombine, GeoCombineParams, "geo_combine", k_geo_combine(ex, p), 256, 4)
#define SM_KERNELS_GEO(X) X(KGeoGram) X(KGeoGramTiled) X(KGeoFold) X(KGeoCoef) X(KGeoCombine)

}  // namespace smhip
