// sm_extract.hpp - the device primitives and the host eigensolver of smhip_lora_extract: a low-rank adapter (A, B) from
// a finetune and its base by a randomized subspace iteration whose small algebra runs on L x L matrices.  The function
// is stated step by step in include/shardmerge_hip.h; every value below is defined bit for bit.
//
//   xl_fill        the Rademacher panel, a function of (key, flat index): one Philox4x32-10 block per 128 entries.
//   xl_delta_mm    THE hot path, on v_mfma_f32_16x16x4_f32: Y = D X (trans = 0) or Y = D^T X (trans = 1) with
//                  D = fp32(finetune) - fp32(base) formed in registers and never written, X an fp32 panel of L columns.
//                  The reduction dimension is cut into segments of XL_SEG; one wave per work-group owns one tile of output
//                  rows, one segment and one chunk of up to XL_CT column tiles of 16, and writes its partial sums to the
//                  workspace.  The instruction is a k-ordered fp32 fmaf chain (one rounding per product), so within a
//                  segment every output element is ONE fmaf chain from +0:
//                    trans = 1  lanes run along the contiguous columns of D (16 bytes = 8 / 4 output rows per lane, eight
//                               row tiles per wave: output row m0 + 8 r + t is row r of tile t) and an instruction takes
//                               the four consecutive k: the chain runs in the natural order, the segment padded with zero
//                               products to a multiple of 4.
//                    trans = 0  a lane loads 8 elements along k (k0 + 8 g + j of its row, g = lane >> 4) and instruction
//                               j takes element j of the four lane groups: inside every block of 32 the chain visits
//                               k0 + 8 g + j in the order j = 0..7 outside, g = 0..3 inside; the segment is padded with
//                               zero products to a multiple of 32.
//                  An element past an edge enters as a product of two +0 (no out-of-bounds read; 16-byte loads only where
//                  the whole group lies inside and the pointers and the row pitch allow them).
//   xl_fold        Y = ((0 + part_0) + part_1) + ... in segment order, fp32, a thread per element; flags a NaN / Inf.
//   xl_gram        P^T P of an fp32 panel in fp64 (a product of two fp32 values is exact in fp64): segments of XL_GSEG
//                  rows, an 8 x 8 tile of pairs per work-group, four threads per pair that take the segment's rows
//                  q, q + 4, ... in order, a two-step binary tree through LDS ((s0 + s2) + (s1 + s3)).
//   xl_gram_fold   the segments added in index order, both triangles written.
//   xl_panel_mm    panel [m x L] . T [L x L2], per element one fp32 fmaf chain over k = 0..L-1 from +0 (VALU), stored as
//                  an fp32 panel or rounded once into a factor dtype, optionally transposed; the panel may be the leading
//                  columns of a wider one and the result a block of columns of a wider one (row pitches, a column offset).
//   xl_sym_eig     host: cyclic Jacobi on a symmetric L x L fp64 matrix over geo_dmul / geo_dadd / geo_ddiv / geo_dsqrt,
//                  each ONE rounded operation, so the hipcc build, the g++ emulator and a numpy restatement agree.
#pragma once
#include <vector>

#include "sm_dare.hpp"
#include "sm_geo.hpp"
#include "sm_lora.hpp"

namespace smhip {

constexpr int XL_MAX_RANK = 256;
constexpr int XL_MAX_L = 272;                 // ceil16(256 + 8)
constexpr int XL_OVERSAMPLE = 8;
constexpr int XL_MAX_POWER = 4;
constexpr int XL_SEG = 512;                   // reduction segment of xl_delta_mm: 8192 rows -> 16 segments per row tile
constexpr int XL_CT = 5;                      // column tiles of 16 per work-group (80 columns: r = 64 in one chunk)
constexpr int XL_MT0 = 32;                    // output rows per work-group, trans = 0 (two row tiles)
constexpr int XL_MT1 = 128;                   // ... trans = 1 (eight row tiles, interleaved)
constexpr int XL_GSEG = 256;                  // rows per segment of xl_gram
constexpr int XL_EIG_SWEEPS = 60;

SM_HD int xl_ceil16(int v) { return (v + 15) / 16 * 16; }
SM_HD int xl_panel_width(int rows, int cols, int rank) {
    const int a = xl_ceil16(rank + XL_OVERSAMPLE), b = xl_ceil16(rows < cols ? rows : cols);
    return a < b ? a : b;
}

// ---- the Rademacher panel: entry e (flat, row-major) is +1 when bit (e & 31) of word ((e >> 5) & 3) of the Philox block
//      with counter (e >> 7, 0, 0) is 0, else -1 ----
struct XlFillParams {
    float* out;
    size_t n;                   // entries
    uint64_t key;
};
template <class Ex>
SM_HD void k_xl_fill(Ex& ex, const XlFillParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    ex.each(st, [&](int tid, EmptyState&) {
        const size_t w = (size_t)ex.bid() * ex.nthreads() + tid;          // word index: 32 entries
        const size_t e0 = w * 32;
        if (e0 >= p.n) return;
        const uint64_t blk = w >> 2;
        uint32_t c[4] = {(uint32_t)blk, (uint32_t)(blk >> 32), 0u, 0u};
        philox4x32_10(c, (uint32_t)p.key, (uint32_t)(p.key >> 32));
        const uint32_t bits = c[w & 3];
        const int cnt = p.n - e0 < 32 ? (int)(p.n - e0) : 32;
        for (int b = 0; b < cnt; ++b) p.out[e0 + b] = ((bits >> b) & 1u) ? -1.f : 1.f;
    });
}

// ---- the delta product ----
struct XlMmParams {
    const void* ft;
    const void* base;
    int dtype;
    int rows, cols;             // of the delta
    int trans;                  // 0: [rows x L] = D X, X [cols x L]; 1: [cols x L] = D^T X, X [rows x L]
    int L;
    const float* x;
    float* part;                // [nseg][M][L]
    int nseg, nchunk;           // grid = row tiles x nseg x nchunk
    int vec;                    // ft and base 16-byte aligned and cols % 8 == 0: 16-byte loads of whole groups of 8
};
SM_HD float xl_delta(const XlMmParams& p, size_t idx) {
    return load_elem(p.ft, p.dtype, idx) - load_elem(p.base, p.dtype, idx);
}
// the 8 deltas from flat index idx on, `cnt` of them inside (the others +0); vec: idx % 8 == 0, one aligned group
SM_HD void xl_delta8(const XlMmParams& p, size_t idx, int cnt, bool vec, float* d) {
    float f[8], b[8];
    ties_load8(p.ft, p.dtype, idx, cnt, vec, f);
    ties_load8(p.base, p.dtype, idx, cnt, vec, b);
#pragma unroll
    for (int e = 0; e < 8; ++e) d[e] = f[e] - b[e];
}

#if defined(__HIP_DEVICE_COMPILE__)
typedef float xl_f32x4 __attribute__((ext_vector_type(4)));
#endif

template <class Ex>
SM_HD void k_xl_delta_mm(Ex& ex, const XlMmParams& p) {
    const int M = p.trans ? p.cols : p.rows, K = p.trans ? p.rows : p.cols;
    const int chunk = ex.bid() % p.nchunk, seg = (ex.bid() / p.nchunk) % p.nseg, mt = ex.bid() / (p.nchunk * p.nseg);
    const int l0 = chunk * XL_CT * 16;
    const int nt = (p.L - l0) / 16 < XL_CT ? (p.L - l0) / 16 : XL_CT;      // column tiles of this chunk
    const int ks = seg * XL_SEG, ke = ks + XL_SEG < K ? ks + XL_SEG : K;   // the segment [ks, ke)
    float* part = p.part + (size_t)seg * M * p.L;
#if defined(__HIP_DEVICE_COMPILE__)
    const int lane = threadIdx.x & 63, i16 = lane & 15, g = lane >> 4;
    if (!p.trans) {
        const int m0 = mt * XL_MT0;
        xl_f32x4 acc[2][XL_CT];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int t = 0; t < XL_CT; ++t) acc[a][t] = xl_f32x4{0.f, 0.f, 0.f, 0.f};
        for (int k0 = ks; k0 < ke; k0 += 32) {
            const int kl = k0 + 8 * g;                      // the lane's 8 k
            const int cnt = ke - kl < 0 ? 0 : (ke - kl > 8 ? 8 : ke - kl);
            float d[2][8];
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                const int m = m0 + 16 * a + i16;
                const int c = m < M ? cnt : 0;
                xl_delta8(p, c ? (size_t)m * p.cols + kl : 0, c, p.vec && c == 8, d[a]);
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = kl + j;
                float xv[XL_CT];
#pragma unroll
                for (int t = 0; t < XL_CT; ++t) xv[t] = (t < nt && k < ke) ? p.x[(size_t)k * p.L + l0 + 16 * t + i16] : 0.f;
#pragma unroll
                for (int t = 0; t < XL_CT; ++t) {
                    if (t < nt) {
                        acc[0][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(d[0][j], xv[t], acc[0][t], 0, 0, 0);
                        acc[1][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(d[1][j], xv[t], acc[1][t], 0, 0, 0);
                    }
                }
            }
        }
        // C/D map: column = lane & 15, row = 4 (lane >> 4) + reg
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int t = 0; t < XL_CT; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int m = m0 + 16 * a + 4 * g + r;
                    if (t < nt && m < M) part[(size_t)m * p.L + l0 + 16 * t + i16] = acc[a][t][r];
                }
    } else {
        const int m0 = mt * XL_MT1;
        xl_f32x4 acc[8][XL_CT];
#pragma unroll
        for (int a = 0; a < 8; ++a)
#pragma unroll
            for (int t = 0; t < XL_CT; ++t) acc[a][t] = xl_f32x4{0.f, 0.f, 0.f, 0.f};
        const int ml = m0 + 8 * i16;                        // the lane's 8 output rows (columns of the delta)
        const int mcnt = M - ml < 0 ? 0 : (M - ml > 8 ? 8 : M - ml);
        for (int k0 = ks; k0 < ke; k0 += 4) {
            const int k = k0 + g;
            const int c = k < ke ? mcnt : 0;
            float d[8], xv[XL_CT];
            xl_delta8(p, c ? (size_t)k * p.cols + ml : 0, c, p.vec && c == 8, d);
#pragma unroll
            for (int t = 0; t < XL_CT; ++t) xv[t] = (t < nt && k < ke) ? p.x[(size_t)k * p.L + l0 + 16 * t + i16] : 0.f;
#pragma unroll
            for (int a = 0; a < 8; ++a)
#pragma unroll
                for (int t = 0; t < XL_CT; ++t)
                    if (t < nt) acc[a][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(d[a], xv[t], acc[a][t], 0, 0, 0);
        }
#pragma unroll
        for (int a = 0; a < 8; ++a)
#pragma unroll
            for (int t = 0; t < XL_CT; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int m = m0 + 8 * (4 * g + r) + a;
                    if (t < nt && m < M) part[(size_t)m * p.L + l0 + 16 * t + i16] = acc[a][t][r];
                }
    }
#else
    // the same chains, one output row at a time: its deltas in chain order once, then a chain per column
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const int MT = p.trans ? XL_MT1 : XL_MT0, m0 = mt * MT, nthr = ex.nthreads();
    const int step = p.trans ? 4 : 32;
    ex.each(st, [&](int tid, EmptyState&) {
        float dk[XL_SEG];
        int kk[XL_SEG];                                     // the k of a chain position, -1: a padding product
        for (int r = tid; r < MT; r += nthr) {
            const int m = m0 + r;
            if (m >= M) continue;
            int n = 0;
            for (int k0 = ks; k0 < ke; k0 += step)
                for (int q = 0; q < step; ++q, ++n) {
                    const int k = p.trans ? k0 + q : k0 + 8 * (q & 3) + (q >> 2);      // trans = 0: j = q >> 2 outside, g = q & 3 inside
                    kk[n] = k < ke ? k : -1;
                    dk[n] = k < ke ? xl_delta(p, p.trans ? (size_t)k * p.cols + m : (size_t)m * p.cols + k) : 0.f;
                }
            for (int l = l0; l < l0 + 16 * nt; ++l) {
                float acc = 0.f;
                for (int i = 0; i < n; ++i) acc = fmaf(dk[i], kk[i] >= 0 ? p.x[(size_t)kk[i] * p.L + l] : 0.f, acc);
                part[(size_t)m * p.L + l] = acc;
            }
        }
    });
#endif
}

struct XlFoldParams {
    const float* part;          // [nseg][n]
    float* out;                 // [n]
    size_t n;
    int nseg;
    uint32_t* flags;            // [0] |= 1 when a result is a NaN or an Inf
};
template <class Ex>
SM_HD void k_xl_fold(Ex& ex, const XlFoldParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    ex.each(st, [&](int tid, EmptyState&) {
        const size_t e = (size_t)ex.bid() * ex.nthreads() + tid;
        if (e >= p.n) return;
        float s = 0.f;
        for (int q = 0; q < p.nseg; ++q) s = s + p.part[(size_t)q * p.n + e];
        p.out[e] = s;
        if (delta_key(s) >= TIES_KEY_INF) ex.global_atomic_or_u32(p.flags, 1u);
    });
}

// ---- the Gram of a panel ----
struct XlGramParams {
    const float* pan;           // [m x L], `pitch` floats from row to row (L, or more: the leading columns of a wider panel)
    int m, L, pitch;
    double* part;               // [nseg][L][L]: the tiles with block row <= block column
};
SM_HD int xl_gram_tiles(int L) { const int nb = L / 8; return nb * (nb + 1) / 2; }
template <class Ex>
SM_HD void k_xl_gram(Ex& ex, const XlGramParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const int ntiles = xl_gram_tiles(p.L), seg = ex.bid() / ntiles;
    int tile = ex.bid() % ntiles, A = 0;
    for (int rowlen = p.L / 8; tile >= rowlen; tile -= rowlen, --rowlen) ++A;
    const int a0 = 8 * A, b0 = 8 * (A + tile);
    double* red = (double*)ex.lds();                        // [4][64]
    const int r0 = seg * XL_GSEG, r1 = r0 + XL_GSEG < p.m ? r0 + XL_GSEG : p.m;
    ex.each(st, [&](int tid, EmptyState&) {
        const int pi = tid & 63, q = tid >> 6;
        const float* ca = p.pan + a0 + (pi >> 3);
        const float* cb = p.pan + b0 + (pi & 7);
        double acc = 0.0;
        for (int r = r0 + q; r < r1; r += 4) acc = acc + (double)ca[(size_t)r * p.pitch] * (double)cb[(size_t)r * p.pitch];
        red[tid] = acc;
    });
    ex.sync();
    for (int s = 2; s > 0; s >>= 1) {
        ex.each(st, [&](int tid, EmptyState&) {
            if ((tid >> 6) < s) red[tid] = red[tid] + red[tid + 64 * s];
        });
        ex.sync();
    }
    ex.each(st, [&](int tid, EmptyState&) {
        if (tid < 64) p.part[(size_t)seg * p.L * p.L + (size_t)(a0 + (tid >> 3)) * p.L + b0 + (tid & 7)] = red[tid];
    });
}
struct XlGramFoldParams {
    const double* part;
    double* G;                  // [L][L], both triangles
    int L, nseg;
};
template <class Ex>
SM_HD void k_xl_gram_fold(Ex& ex, const XlGramFoldParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    ex.each(st, [&](int tid, EmptyState&) {
        const int e = ex.bid() * ex.nthreads() + tid;
        if (e >= p.L * p.L) return;
        const int i = e / p.L, j = e % p.L;
        if (i / 8 > j / 8) return;
        double s = 0.0;
        for (int q = 0; q < p.nseg; ++q) s = s + p.part[(size_t)q * p.L * p.L + e];
        p.G[e] = s;
        if (i / 8 < j / 8) p.G[(size_t)j * p.L + i] = s;
    });
}

// ---- panel . T ----
struct XlPanelMmParams {
    const float* pan;           // [m x L], pan_pitch floats from row to row
    const float* t;             // [L x L2]
    void* out;                  // [m x L2] as columns col0 .. col0 + L2 of rows of out_pitch elements, or [L2 x m] when store_trans
    int m, L, L2;
    int out_dtype;
    int store_trans;
    int pan_pitch, out_pitch, col0;
};
template <class Ex>
SM_HD void k_xl_panel_mm(Ex& ex, const XlPanelMmParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    ex.each(st, [&](int tid, EmptyState&) {
        const size_t e = (size_t)ex.bid() * ex.nthreads() + tid;
        if (e >= (size_t)p.m * p.L2) return;
        const size_t row = e / p.L2;
        const int j = (int)(e % p.L2);
        const float* pr = p.pan + row * p.pan_pitch;
        float acc = 0.f;
        for (int k = 0; k < p.L; ++k) acc = fmaf(pr[k], p.t[(size_t)k * p.L2 + j], acc);
        lora_put(p.out, p.out_dtype, p.store_trans ? (size_t)j * p.m + row : row * p.out_pitch + p.col0 + j, acc);
    });
}

// ---- host: eigenvalues and eigenvectors of a symmetric n x n fp64 matrix, cyclic Jacobi ----
// a [n][n] (both triangles; destroyed), lam [n] descending (ties: the lower original index first), v [n][n] with
// eigenvector i in COLUMN i, its largest-magnitude entry (the first on ties) positive.  Every operation is one rounded
// fp64 operation.  thr = (sum_i |a_ii|, in index order) * 2^-70.  A sweep visits p = 0..n-2, q = p+1..n-1 in order; a pair
// with |a_pq| <= thr is skipped; else theta = (a_qq - a_pp) / (2 a_pq), t = sgn(theta) / (|theta| + sqrt(theta^2 + 1))
// (sgn(0) = +1), c = 1 / sqrt(t^2 + 1), s = t c; row/column p <- c x_p - s x_q, q <- s x_p + c x_q (k != p, q),
// a_pp <- a_pp - t a_pq, a_qq <- a_qq + t a_pq, a_pq <- 0; the columns p, q of v likewise.  The iteration stops after the
// first sweep that rotates nothing, or after XL_EIG_SWEEPS sweeps.  Returns the sweeps run.
inline int xl_sym_eig(int n, double* a, double* lam, double* v) {
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) v[(size_t)i * n + j] = i == j ? 1.0 : 0.0;
    double scale = 0.0;
    for (int i = 0; i < n; ++i) scale = geo_dadd(scale, std::fabs(a[(size_t)i * n + i]));
    const double thr = geo_dmul(scale, 0x1p-70);
    int sweeps = 0;
    std::vector<double> np(n), nq(n);
    while (sweeps < XL_EIG_SWEEPS) {
        ++sweeps;
        bool rotated = false;
        for (int p = 0; p + 1 < n; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = a[(size_t)p * n + q];
                if (!(std::fabs(apq) > thr)) continue;
                rotated = true;
                const double app = a[(size_t)p * n + p], aqq = a[(size_t)q * n + q];
                const double theta = geo_ddiv(geo_dadd(aqq, -app), geo_dmul(2.0, apq));
                const double den = geo_dadd(std::fabs(theta), geo_dsqrt(geo_dadd(geo_dmul(theta, theta), 1.0)));
                const double t = geo_ddiv(theta < 0.0 ? -1.0 : 1.0, den);
                const double c = geo_ddiv(1.0, geo_dsqrt(geo_dadd(geo_dmul(t, t), 1.0)));
                const double s = geo_dmul(t, c);
                double* rp = a + (size_t)p * n;
                double* rq = a + (size_t)q * n;
                for (int k = 0; k < n; ++k) {
                    np[k] = geo_dadd(geo_dmul(c, rp[k]), -geo_dmul(s, rq[k]));
                    nq[k] = geo_dadd(geo_dmul(s, rp[k]), geo_dmul(c, rq[k]));
                }
                for (int k = 0; k < n; ++k) {
                    rp[k] = np[k]; a[(size_t)k * n + p] = np[k];
                    rq[k] = nq[k]; a[(size_t)k * n + q] = nq[k];
                }
                const double tap = geo_dmul(t, apq);
                a[(size_t)p * n + p] = geo_dadd(app, -tap);
                a[(size_t)q * n + q] = geo_dadd(aqq, tap);
                a[(size_t)p * n + q] = 0.0; a[(size_t)q * n + p] = 0.0;
                for (int k = 0; k < n; ++k) {
                    const double vp = v[(size_t)k * n + p], vq = v[(size_t)k * n + q];
                    v[(size_t)k * n + p] = geo_dadd(geo_dmul(c, vp), -geo_dmul(s, vq));
                    v[(size_t)k * n + q] = geo_dadd(geo_dmul(s, vp), geo_dmul(c, vq));
                }
            }
        if (!rotated) break;
    }
    // sort (stable insertion by descending eigenvalue), then the signs
    std::vector<int> ord(n);
    for (int i = 0; i < n; ++i) ord[i] = i;
    for (int i = 1; i < n; ++i) {
        const int o = ord[i];
        int j = i;
        while (j > 0 && a[(size_t)ord[j - 1] * n + ord[j - 1]] < a[(size_t)o * n + o]) { ord[j] = ord[j - 1]; --j; }
        ord[j] = o;
    }
    std::vector<double> vs((size_t)n * n);
    for (int i = 0; i < n; ++i) {
        const int o = ord[i];
        lam[i] = a[(size_t)o * n + o];
        int big = 0;
        for (int k = 1; k < n; ++k)
            if (std::fabs(v[(size_t)k * n + o]) > std::fabs(v[(size_t)big * n + o])) big = k;
        const bool neg = v[(size_t)big * n + o] < 0.0;
        for (int k = 0; k < n; ++k) vs[(size_t)k * n + i] = neg ? -v[(size_t)k * n + o] : v[(size_t)k * n + o];
    }
    for (size_t i = 0; i < (size_t)n * n; ++i) v[i] = vs[i];
    return sweeps;
}

// ---- kernel tags (sm_tag.hpp) and group 9 of smhip_side.hip (smhip_device.hpp) ----
// the Rademacher panel, the delta product on fp32 MFMA (one wave per work-group: 40 or 160 accumulator registers) and its
// fold, the ordered fp64 Gram of a panel and its fold, panel x small matrix
SM_KERNEL_TAG_LB(KXlFill, XlFillParams, "xl_fill", k_xl_fill(ex, p), 256, 4)
SM_KERNEL_TAG_LB(KXlDeltaMm, XlMmParams, "xl_delta_mm", k_xl_delta_mm(ex, p), 64, 2)
SM_KERNEL_TAG_LB(KXlFold, XlFoldParams, "xl_fold", k_xl_fold(ex, p), 256, 4)
SM_KERNEL_TAG_LB(KXlGram, XlGramParams, "xl_gram", k_xl_gram(ex, p), 256, 4)
SM_KERNEL_TAG_LB(KXlGramFold, XlGramFoldParams, "xl_gram_fold", k_xl_gram_fold(ex, p), 256, 4)
SM_KERNEL_TAG_LB(KXlPanelMm, XlPanelMmParams, "xl_panel_mm", k_xl_panel_mm(ex, p), 256, 4)
#define SM_SIDE_KERNELS_9(X) X(KXlFill) X(KXlDeltaMm) X(KXlFold) X(KXlGram) X(KXlGramFold) X(KXlPanelMm)

}  // namespace smhip
